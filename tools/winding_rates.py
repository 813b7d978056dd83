#!/usr/bin/env python3
"""tools/winding_rates.py [--calls K] [--most N]: pairs and points per second of the winding-number queries (include/ezrt_winding.h).

One JSON line.  Scene: the Bunny scene of C2 (bunny_scene(subdiv=2)).  Points uniform in the scene's bounding box grown by a tenth:
1 000 (the sliced path: chunks == 0 picks as many slices as 256 triangles each allow), 65 536 (eight slices by the rule), 131 072
(four), 524 288 (the first count at which the rule picks one slice) and `most` (default 1 048 576).  For each count the library's
own choice (`auto`, with the number of slices it picks) beside forced slicings on both sides of the rule (`one`: chunks = 1; `two`,
`eight`, `many`: 2, 8 and 64 slices), as Gpairs/s (a pair is one point against one triangle: every point is summed over every
triangle) and Mpoints/s.

Both ways of reading the triangles are reported: `tile` (a tile of 64 sorted triangles staged through LDS and read as a broadcast:
the library's default) and `scalar` (the triangle index is uniform, the record is read with scalar loads: EZRT_WINDING_SCALAR=1, read
once per process, so the tool runs each variant in a fresh child process of its own).  Each figure is timed with events around `calls`
back-to-back calls on one stream after a warm-up call.  The answers of all slicings and of both variants are compared (`equal`:
the int64 sums must be the same bits); nothing else is checked here (tests/test_gpu_winding.py).

fp64: the counted fp64 operations per pair are W2's 61 -- 9 differences, 32 products and 20 sums of the cross product, det, the
three squared lengths, the three dot products and den -- NOT counting the three square roots, the two divisions, the max and the
absolute values (each of which is itself a sequence of fp64 instructions) or the fp32 ez_atan2.  None of them may be fused, so each
is one instruction slot where a fused multiply-add would do two: `fp64_fraction_of_peak` is 61 * pairs/s over HALF of the MI355X's
published 78.6 TFLOP/s vector fp64 peak (which counts a fused multiply-add as two), `fp64_gops` the numerator."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP64_OPS_PER_PAIR = 61
FP64_SLOT_PEAK = 78.6e12 / 2


def measure(calls, most):
    import torch
    from ezrt_amd import query, scenes, trace
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(1)
    sc = scenes.bunny_scene(subdiv=2, hdr="shipped")
    tri, nodes = sc.tri, sc.nodes
    P = tri[:, :9].reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    pad = 0.1 * (hi - lo)
    sg = hip.scene_create(tri, nodes)
    n_tri = int(tri.shape[0])
    out = {"triangles": n_tri, "counts": {}}
    sums = {}
    for n in (1000, 65536, 131072, 524288, most):
        pts = torch.from_numpy(rng.uniform(lo - pad, hi + pad, (n, 3)).astype(np.float32)).to(dev)
        res = {"auto_slices": int(hip.lib.ezrt_winding_chunks(n, n_tri))}
        ways = {"auto": None, "one": 1, "two": 2, "eight": 8, "many": 64}
        if n >= 1 << 19:
            ways = {"auto": None, "two": 2}
        ref = None
        for name, chunks in ways.items():
            fn = lambda: query.winding_number(sg, pts, fixed=True, chunks=chunks)
            _, f = fn()
            torch.cuda.synchronize()
            k = max(1, calls if n < 1 << 19 else calls // 4)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(k):
                fn()
            e1.record(stream)
            e1.synchronize()
            sec = e0.elapsed_time(e1) * 1e-3 / k
            pairs = n * n_tri / sec
            res[name] = {"ms_per_call": round(sec * 1e3, 4), "gpairs_per_s": round(pairs / 1e9, 3), "mpoints_per_s": round(n / sec / 1e6, 4),
                         "fp64_gops": round(pairs * FP64_OPS_PER_PAIR / 1e9, 1),
                         "fp64_fraction_of_peak": round(pairs * FP64_OPS_PER_PAIR / FP64_SLOT_PEAK, 4)}
            ref = f if ref is None else ref
            res["equal"] = bool(res.get("equal", True) and torch.equal(f, ref))
        sums[n] = int(ref.sum().item()) & 0xFFFFFFFFFFFF
        out["counts"][str(n)] = res
    out["checksum"] = sums
    sg.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--most", type=int, default=1 << 20)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.calls, args.most)))
        return 0
    import torch
    from ezrt_amd.srchash import gpu_source_hash
    out = {"tool": "winding_rates", "srchash": gpu_source_hash(), "calls": args.calls, "fp64_ops_per_pair": FP64_OPS_PER_PAIR,
           "fp64_slot_peak_tops": FP64_SLOT_PEAK / 1e12}
    for variant, flag in (("tile", "0"), ("scalar", "1")):
        env = dict(os.environ, EZRT_WINDING_SCALAR=flag)
        txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--most", str(args.most)],
                             env=env, check=True, capture_output=True, text=True).stdout
        out[variant] = json.loads(txt.strip().splitlines()[-1])
    out["variants_equal"] = out["scalar"]["checksum"] == out["tile"]["checksum"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
