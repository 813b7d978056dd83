#!/usr/bin/env python3
"""tools/plane_rates.py [--calls K] [--repeats R]: pairs and segments per second of the plane queries (include/ezrt_plane.h).

One JSON line.  Scenes: the Bunny scene of C2 (bunny_scene(subdiv=2), 79 820 triangles) and the scene of C5 (mega_scene(), 10^6
triangles).  Planes: 1, 64, 1 000 and 10 000 PARALLEL planes (a slicer's stack: normal +y, evenly spaced over the scene's height) and
as many RANDOM ones (through uniform points of the bounding box, uniform normals).  For each set the count call
(ezrt_query_plane_count_device: the sweep, the row sums and the prefix sum) and the fill call (ezrt_query_plane_section_device, with
segments, capacity = the total) are timed SEPARATELY, each with events around `calls` back-to-back calls on one stream after a warm-up
call: ms per call, Gpairs/s (a pair is one plane against one triangle: every plane is tested against every triangle) and, for the
fill, Msegments/s.  The library's own slicing (`auto`, with the number of slices it picks) stands beside forced 1, 8, 64 and 256 slices;
the answers of all slicings are compared (`equal`: offsets, ids and segments must be the same bits).

`prefix_ms`: the count call with and without `offsets` at 10 000 and 100 000 planes on the Bunny scene -- the difference is the
prefix-sum kernel (one workgroup).  `spread`: one configuration (1 000 parallel planes, Bunny scene, auto) measured `repeats`
times: (max - min) / median of the count and of the fill call.

fp64: the counted fp64 operations per pair are P2's 18 -- 9 products, 6 sums and 3 differences -- in BOTH passes; the division and
the interpolation of P4 run for crossed pairs only and are not counted.  None of them may be fused, so each is one instruction
slot where a fused multiply-add would do two: `fp64_fraction_of_peak` is 18 * pairs/s over HALF of the MI355X's published
78.6 TFLOP/s vector fp64 peak (which counts a fused multiply-add as two), as profiles/r23/winding_rates.txt counts it."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP64_OPS_PER_PAIR = 18
FP64_SLOT_PEAK = 78.6e12 / 2
P = C.c_void_p


def plane_sets(tri, n, rng):
    V = tri[:, :9].reshape(-1, 3)
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    par = np.zeros((n, 4), np.float32)
    par[:, 1] = 1.0
    par[:, 3] = lo[1] + (hi[1] - lo[1]) * (np.arange(n) + 0.5) / n
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts = rng.uniform(lo, hi, (n, 3))
    rnd = np.concatenate([nrm, (nrm * pts).sum(1, keepdims=True)], 1).astype(np.float32)
    return {"parallel": par, "random": rnd}


class Runner:
    def __init__(self, hip, sg, n_tri, dev, calls):
        import torch
        self.t, self.lib, self.sg, self.n_tri, self.dev, self.calls = torch, hip.lib, sg, n_tri, dev, calls
        self.stream = torch.cuda.current_stream(dev)

    def timed(self, fn, calls=None):
        t = self.t
        k = calls or self.calls
        fn()
        t.cuda.synchronize()
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        for _ in range(k):
            fn()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    def run(self, planes, slices, want_rows=True, offsets=True):
        """(result dict, (offsets, ids, seg) tensors) of one set of planes under one slicing"""
        t, lib, sg = self.t, self.lib, self.sg
        n = planes.shape[0]
        S = int(lib.ezrt_plane_slices(n, self.n_tri, slices))
        h = P(self.stream.cuda_stream)
        part = t.empty((n, S), dtype=t.int32, device=self.dev)
        nc = t.empty((n,), dtype=t.int32, device=self.dev)
        off = t.empty((n + 1,), dtype=t.int64, device=self.dev)
        count = lambda: lib.ezrt_query_plane_count_device(sg._h, P(planes.data_ptr()), n, slices, P(part.data_ptr()), P(nc.data_ptr()),
                                                          P(off.data_ptr()) if offsets else None, h)
        assert count() == 0
        ms_count = self.timed(count)
        pairs = n * self.n_tri
        res = {"slices": S, "count_ms": round(ms_count, 4), "count_gpairs_per_s": round(pairs / ms_count / 1e6, 2),
               "count_fp64_fraction_of_peak": round(pairs / (ms_count * 1e-3) * FP64_OPS_PER_PAIR / FP64_SLOT_PEAK, 4)}
        if not (want_rows and offsets):
            return res, None
        total = int(off[n].item())
        ids = t.empty((total,), dtype=t.int32, device=self.dev)
        seg = t.empty((total, 6), dtype=t.float32, device=self.dev)
        fill = lambda: lib.ezrt_query_plane_section_device(sg._h, P(planes.data_ptr()), n, slices, P(part.data_ptr()), P(off.data_ptr()),
                                                           total, P(ids.data_ptr()), P(seg.data_ptr()), h)
        assert fill() == 0
        ms_fill = self.timed(fill)
        res.update({"rows": total, "fill_ms": round(ms_fill, 4), "fill_gpairs_per_s": round(pairs / ms_fill / 1e6, 2),
                    "fill_msegments_per_s": round(total / ms_fill / 1e3, 2),
                    "fill_fp64_fraction_of_peak": round(pairs / (ms_fill * 1e-3) * FP64_OPS_PER_PAIR / FP64_SLOT_PEAK, 4)})
        return res, (off, ids, seg)


def measure(calls, repeats):
    import torch
    from ezrt_amd import scenes, trace
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    out = {"scenes": {}}
    for name, make in (("C2", lambda: scenes.bunny_scene(subdiv=2, hdr="shipped")), ("C5", lambda: scenes.mega_scene())):
        sc = make()
        tri = np.ascontiguousarray(sc.tri, np.float32)
        sg = hip.scene_create(sc.tri, sc.nodes)
        n_tri = int(tri.shape[0])
        run = Runner(hip, sg, n_tri, dev, calls)
        rng = np.random.default_rng(24)
        res = {"triangles": n_tri, "sets": {}}
        for n in (1, 64, 1000, 10000):
            for kind, planes in plane_sets(tri, n, rng).items():
                pt = torch.from_numpy(planes).to(dev)
                row, ref = {}, None
                for way, slices in (("auto", 0), ("one", 1), ("eight", 8), ("many", 64), ("more", 256)):
                    row[way], got = run.run(pt, slices)
                    ref = got if ref is None else ref
                    row["equal"] = bool(row.get("equal", True) and all(torch.equal(a, b) for a, b in zip(got, ref)))
                    del got
                res["sets"]["%d %s" % (n, kind)] = row
                del ref
        if name == "C2":
            pre = {}
            for n in (10000, 100000):
                pt = torch.from_numpy(plane_sets(tri, n, rng)["parallel"]).to(dev)
                a, _ = run.run(pt, 0, want_rows=False)
                b, _ = run.run(pt, 0, want_rows=False, offsets=False)
                pre[str(n)] = {"with_offsets_ms": a["count_ms"], "without_ms": b["count_ms"], "prefix_ms": round(a["count_ms"] - b["count_ms"], 4)}
            res["prefix_ms"] = pre
            pt = torch.from_numpy(plane_sets(tri, 1000, np.random.default_rng(24))["parallel"]).to(dev)
            reps = [run.run(pt, 0)[0] for _ in range(repeats)]
            sp = lambda k: round((max(r[k] for r in reps) - min(r[k] for r in reps)) / float(np.median([r[k] for r in reps])), 4)
            res["spread"] = {"repeats": repeats, "count_ms": [r["count_ms"] for r in reps], "fill_ms": [r["fill_ms"] for r in reps],
                             "count": sp("count_ms"), "fill": sp("fill_ms")}
        out["scenes"][name] = res
        sg.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    from ezrt_amd.srchash import gpu_source_hash
    out = {"tool": "plane_rates", "srchash": gpu_source_hash(), "calls": args.calls, "fp64_ops_per_pair": FP64_OPS_PER_PAIR,
           "fp64_slot_peak_tops": FP64_SLOT_PEAK / 1e12}
    out.update(measure(args.calls, args.repeats))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
