#!/usr/bin/env python3
"""tools/overlap_list_rates.py [--calls K] [--repeats R] [--scenes C2,C5]: the time of the three steps of an overlap list
(include/ezrt_overlap_list.h) for boxes, and ids per second.

One JSON line.  Scenes: the Bunny scene of C2 (bunny_scene(subdiv=2), 79 820 triangles) and the scene of C5 (mega_scene(), 10^6
triangles).  Box sets: cubes around the centroids of random triangles whose half edge is found by bisection on the device so that the
MEDIAN row has about 8, about 64 and about 1 000 ids (4 096, 4 096 and 512 boxes), and one box that holds the whole scene.  For each
set the count call (ezrt_query_box_overlap_device with max_k == 0), the offsets call and the fill call
(ezrt_query_box_overlap_list_device, capacity = the total, with n_found) are timed SEPARATELY, each with events around `calls`
back-to-back calls on one stream after a warm-up call, `repeats` times, the steps interleaved within a repeat: the median ms per call,
and the spread (max - min) / median of the repeats beside it.  `mids_per_s` is the total of ids over count + offsets + fill.
The fill call is the routed fill kernel and, on the walk route, overlap_sort_kernel behind it in the same call: the sort's own time is
the difference to a library built with -DEZRT_OL_SKIP_SORT=1 (never the product: its long rows are unsorted), run by the same tool
in the same job (`label` says which library a line is from).
`le64`: the boxes of the first set whose count is at most 64.  For them the max_k = 64 call returns the same information in ONE
launch and one traversal; it is timed in the same repeats, interleaved, and `ratio` is (count + fill) / that.
`certified`: n_found == the row lengths everywhere; `sorted`: every row ascends (false for a library that skips the sort)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = C.c_void_p
SETS = (("rows~8", 8, 4096), ("rows~64", 64, 4096), ("rows~1000", 1000, 512))


class Runner:
    def __init__(self, hip, sg, tri, dev, calls, repeats):
        import torch
        self.t, self.lib, self.sg, self.dev, self.calls, self.repeats = torch, hip.lib, sg, dev, calls, repeats
        self.stream = torch.cuda.current_stream(dev)
        self.h = P(self.stream.cuda_stream)
        V = tri[:, :9].reshape(-1, 3, 3)
        self.centroid = V.mean(1)
        self.lo, self.hi = V.reshape(-1, 3).min(0), V.reshape(-1, 3).max(0)

    def timed(self, fn, calls):
        t = self.t
        assert fn() == 0
        t.cuda.synchronize()
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        for _ in range(calls):
            fn()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def counts(self, lo, hi):
        t = self.t
        n = lo.shape[0]
        nov = t.empty((n,), dtype=t.int32, device=self.dev)
        assert self.lib.ezrt_query_box_overlap_device(self.sg._h, P(lo.data_ptr()), P(hi.data_ptr()), n, 0, None, P(nov.data_ptr()), self.h) == 0
        return nov

    def boxes(self, target, n, rng):
        """(lo, hi) device tensors: cubes whose median row has about `target` ids"""
        t = self.t
        c = t.from_numpy(self.centroid[rng.integers(0, self.centroid.shape[0], n)].astype(np.float32)).to(self.dev)
        a, b = 1e-5, 1.0                                                # the half edge as a fraction of the scene's size
        size = float(np.max(self.hi - self.lo))
        for _ in range(20):
            m = (a * b) ** 0.5
            med = float(self.counts(c - m * size, c + m * size).float().median())
            a, b = (m, b) if med < target else (a, m)
        m = (a * b) ** 0.5
        return (c - m * size).contiguous(), (c + m * size).contiguous()

    def measure(self, lo, hi, yardstick=False, calls=None, repeats=None):
        calls, repeats = calls or self.calls, repeats or self.repeats
        t, lib, sg, h = self.t, self.lib, self.sg, self.h
        n = lo.shape[0]
        nov = self.counts(lo, hi)
        off = t.empty((n + 1,), dtype=t.int64, device=self.dev)
        nf = t.empty((n,), dtype=t.int32, device=self.dev)
        count = lambda: lib.ezrt_query_box_overlap_device(sg._h, P(lo.data_ptr()), P(hi.data_ptr()), n, 0, None, P(nov.data_ptr()), h)
        offsets = lambda: lib.ezrt_overlap_offsets_device(sg._h, P(nov.data_ptr()), n, P(off.data_ptr()), h)
        assert offsets() == 0
        total = int(off[n].item())
        ids = t.full((max(total, 1),), -1, dtype=t.int32, device=self.dev)
        fill = lambda: lib.ezrt_query_box_overlap_list_device(sg._h, P(lo.data_ptr()), P(hi.data_ptr()), n, P(off.data_ptr()), total,
                                                              P(ids.data_ptr()), P(nf.data_ptr()), h)
        steps = {"count": count, "offsets": offsets, "fill": fill}
        if yardstick:
            rows = t.empty((n, 64), dtype=t.int32, device=self.dev)
            steps["max_k_64"] = lambda: lib.ezrt_query_box_overlap_device(sg._h, P(lo.data_ptr()), P(hi.data_ptr()), n, 64, P(rows.data_ptr()),
                                                                         P(nov.data_ptr()), h)
        ms = {k: [] for k in steps}
        for _ in range(repeats):                                        # interleaved: every step once per repeat
            for k, fn in steps.items():
                ms[k].append(self.timed(fn, calls))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        lens = nov.long()
        first = off[:-1]
        inner = t.ones(total, dtype=t.bool, device=self.dev)
        inner[first[lens > 0]] = False                                  # the first entry of a row has no predecessor in it
        asc = bool(((ids[1:total] > ids[:total - 1]) | ~inner[1:total]).all()) if total > 1 else True
        res = {"boxes": n, "calls": calls, "repeats": repeats, "ids": total, "median_row": float(lens.float().median()), "longest_row": int(lens.max()),
               "certified": bool(t.equal(nf, nov)), "sorted": asc}
        for k in steps:
            res[k + "_ms"] = round(med[k], 4)
            res[k + "_spread"] = round((max(ms[k]) - min(ms[k])) / med[k], 4)
        all3 = med["count"] + med["offsets"] + med["fill"]
        res["mids_per_s"] = round(total / all3 / 1e3, 2)
        if yardstick:
            res["ratio"] = round((med["count"] + med["fill"]) / med["max_k_64"], 3)
        return res, nov


def measure(calls, repeats, names):
    import torch
    from ezrt_amd import scenes, trace
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    out = {}
    makers = {"C2": lambda: scenes.bunny_scene(subdiv=2, hdr="shipped"), "C5": lambda: scenes.mega_scene()}
    for name in names:
        sc = makers[name]()
        tri = np.ascontiguousarray(sc.tri, np.float32)
        sg = hip.scene_create(sc.tri, sc.nodes)
        run = Runner(hip, sg, tri, dev, calls, repeats)
        rng = np.random.default_rng(25)
        res = {"triangles": int(tri.shape[0]), "walk": sg.prune_info()["mode"] != -1, "sets": {}}
        for key, target, n in SETS:
            lo, hi = run.boxes(target, n, rng)
            res["sets"][key], nov = run.measure(lo, hi)
            if target == 8:
                keep = nov <= 64
                res["sets"]["le64"], _ = run.measure(lo[keep].contiguous(), hi[keep].contiguous(), yardstick=True)
        lo = torch.from_numpy(run.lo[None].astype(np.float32)).to(dev)
        hi = torch.from_numpy(run.hi[None].astype(np.float32)).to(dev)
        res["sets"]["whole"], _ = run.measure(lo, hi, calls=1, repeats=3)   # one lane walks every triangle: seconds on C5
        out[name] = res
        sg.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scenes", default="C2,C5")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch  # noqa: F401  (before the library is opened: torch brings its own HIP runtime, which must be the first one loaded)
    from ezrt_amd import _abi
    from ezrt_amd.srchash import gpu_source_hash
    insert_max, tile_max = _abi.overlap_list_limits()
    out = {"tool": "overlap_list_rates", "label": args.label, "srchash": gpu_source_hash(), "calls": args.calls, "repeats": args.repeats,
           "insert_max": insert_max, "tile_max": tile_max, "lib": os.path.basename(os.environ.get("EZRT_HIP_LIB", "") or "libezrt_hip.so")}
    out["scenes"] = measure(args.calls, args.repeats, args.scenes.split(","))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
