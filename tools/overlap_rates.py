#!/usr/bin/env python3
"""tools/overlap_rates.py [--calls K]: boxes per second of the box-overlap queries (include/ezrt_box_overlap.h).

One JSON line.  Scene: the Bunny scene of C2 (bunny_scene(subdiv=2)).  Boxes: centred on points uniform in the scene's bounding box,
at three sizes --
  leaf     a leaf-sized cell: the median longest side of the triangles' bounding boxes
  eighth   1/8 of the scene's extent per axis
  whole    the scene's bounding box itself (every triangle overlaps: n x n_tri work on both routes, so fewer boxes per call)
and for max_k = 0 (count only), 8 and 64 (with the count).  For each the two routes side by side:
  walk     box_overlap_kernel<true>: the depth-first walk over the 4-wide records (the scene as created)
  sweep    box_overlap_kernel<false>: every triangle, no tree -- the same arrays created with one leaf given a second parent, so that
           the scene does not prune; fewer boxes per call
Each is timed with hipEvents around `calls` back-to-back calls on one stream after a warm-up call; the rate is Mboxes/s.  The two
routes' answers are compared on the sweep's boxes (they must be equal); nothing else is checked here (tests/test_gpu_box_overlap.py)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from closest_point_rates import second_parent  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--boxes", type=int, default=1 << 17)
    args = ap.parse_args()
    import torch
    from ezrt_amd import query, scenes, trace
    from ezrt_amd.srchash import gpu_source_hash
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(1)

    def rate(fn, n, calls):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return round(n * calls / (e0.elapsed_time(e1) * 1e-3) / 1e6, 4)

    sc = scenes.bunny_scene(subdiv=2, hdr="shipped")
    tri, nodes = sc.tri, sc.nodes
    P = tri[:, :9].reshape(-1, 3, 3)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    leaf = float(np.median((P.max(1) - P.min(1)).max(1)))
    walk, swept = hip.scene_create(tri, nodes), hip.scene_create(tri, second_parent(nodes))
    assert walk.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    out = {"tool": "overlap_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mboxes/s", "triangles": int(tri.shape[0]), "sizes": {}}
    few = max(1, args.calls // 5)
    # (half sizes per axis, boxes per call on the walk, on the sweep)
    sizes = {"leaf": (np.full(3, leaf / 2), args.boxes, 1 << 13), "eighth": ((hi - lo) / 16, args.boxes, 1 << 13),
             "whole": ((hi - lo) / 2, 1 << 11, 1 << 11)}
    for name, (half, n_walk, n_sweep) in sizes.items():
        c = rng.uniform(lo, hi, (n_walk, 3)) if name != "whole" else np.tile((lo + hi) / 2, (n_walk, 1))
        bl = torch.from_numpy(np.ascontiguousarray(c - half, np.float32)).to(dev)
        bh = torch.from_numpy(np.ascontiguousarray(c + half, np.float32)).to(dev)
        sl, sh = bl[:n_sweep].contiguous(), bh[:n_sweep].contiguous()
        a, b = query.box_overlap(walk, sl, sh, 64, count=True), query.box_overlap(swept, sl, sh, 64, count=True)
        torch.cuda.synchronize()
        res = {"half_size": [round(float(x), 5) for x in half], "boxes_walk": n_walk, "boxes_sweep": n_sweep,
               "routes_equal": bool(torch.equal(a.tri, b.tri) and torch.equal(a.n_overlap, b.n_overlap)),
               "mean_overlaps": round(float(a.n_overlap.float().mean().item()), 2)}
        for k in (0, 8, 64):
            res["max_k_%d" % k] = {"walk": rate(lambda: query.box_overlap(walk, bl, bh, k, count=True), n_walk, args.calls),
                                   "sweep": rate(lambda: query.box_overlap(swept, sl, sh, k, count=True), n_sweep, few)}
        out["sizes"][name] = res
    walk.close()
    swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
