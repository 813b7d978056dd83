#!/usr/bin/env python3
"""tools/obb_overlap_rates.py [--calls K]: boxes per second of the oriented-box queries (include/ezrt_obb_overlap.h).

One JSON line.  Scene: the Bunny scene of C2 (bunny_scene(subdiv=2)).  Boxes, every one randomly rotated:
  leaf     a leaf-sized cube (half side: half the median longest side of the triangles' bounding boxes) centred on points uniform in
           the scene's bounding box
  thin     a thin box along a random diagonal through a point of the surface: 1/4 of the scene's extent long, 1/40 of that thick
  whole    the scene's bounding box grown by a quarter (every triangle overlaps: n x n_tri work on both routes, so fewer boxes)
and for max_k = 0 (count only), 8 and 64 (with the count).  For each the two routes side by side:
  walk     obb_overlap_kernel<true>: the depth-first walk over the 4-wide records with the hull gate and the face gate
  sweep    obb_overlap_kernel<false>: every triangle, no tree -- the same arrays created with one leaf given a second parent, so that
           the scene does not prune; fewer boxes per call
and beside them `hull`: box_overlap's walk on the same boxes' axis-aligned hulls (tests/obb_overlap_scenes.py: hulls) -- the way of
asking that the oriented query replaces -- with the mean number of candidates per box of each (mean_overlaps, hull_mean_overlaps; a
hull's row is cut off at 64 candidates).  Each is timed with hipEvents around `calls` back-to-back calls on one stream after a
warm-up call; the rate is Mboxes/s.  The two routes' answers are compared on the sweep's boxes (they must be equal); nothing else is
checked here (tests/test_gpu_obb_overlap.py)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from closest_point_rates import second_parent  # noqa: E402
import obb_overlap_scenes as OS  # noqa: E402


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
    extent = float((hi - lo).max())
    walk, swept = hip.scene_create(tri, nodes), hip.scene_create(tri, second_parent(nodes))
    assert walk.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    out = {"tool": "obb_overlap_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mboxes/s", "triangles": int(tri.shape[0]), "kinds": {}}
    few = max(1, args.calls // 5)
    gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    # (half sizes along the box's own axes, boxes per call on the walk, on the sweep)
    kinds = {"leaf": (np.full(3, leaf / 2), args.boxes, 1 << 13), "thin": (np.array([extent / 8, extent / 320, extent / 320]), args.boxes, 1 << 13),
             "whole": ((hi - lo) * 0.625, 1 << 11, 1 << 11)}
    for name, (half, n_walk, n_sweep) in kinds.items():
        if name == "whole":
            c, u = np.tile((lo + hi) / 2, (n_walk, 1)), np.tile(np.diag(half), (n_walk, 1, 1))
        else:
            u = OS._rotations(rng, n_walk) * half[None, :, None]
            if name == "thin":
                t, w = rng.integers(0, P.shape[0], n_walk), rng.dirichlet((1, 1, 1), n_walk)
                c = (P[t] * w[:, :, None]).sum(1)
            else:
                c = rng.uniform(lo, hi, (n_walk, 3))
        c, u = np.ascontiguousarray(c, np.float32), np.ascontiguousarray(u, np.float32)
        hl, hh = OS.hulls(c, u)
        gc, gu, gl, gh = gpu(c), gpu(u), gpu(hl), gpu(hh)
        sc_, su_ = gc[:n_sweep].contiguous(), gu[:n_sweep].contiguous()
        a, b = query.obb_overlap(walk, sc_, su_, 64, count=True), query.obb_overlap(swept, sc_, su_, 64, count=True)
        h = query.box_overlap(walk, gl, gh, 0, count=True)
        full = query.obb_overlap(walk, gc, gu, 0, count=True)
        torch.cuda.synchronize()
        res = {"half_size": [round(float(x), 5) for x in half], "boxes_walk": n_walk, "boxes_sweep": n_sweep,
               "routes_equal": bool(torch.equal(a.tri, b.tri) and torch.equal(a.n_overlap, b.n_overlap)),
               "mean_overlaps": round(float(full.n_overlap.float().mean().item()), 2),
               "hull_mean_overlaps": round(float(h.n_overlap.float().mean().item()), 2),
               "hulls_over_64": round(float((h.n_overlap > 64).float().mean().item()), 4)}
        for k in (0, 8, 64):
            res["max_k_%d" % k] = {"walk": rate(lambda: query.obb_overlap(walk, gc, gu, k, count=True), n_walk, args.calls),
                                   "sweep": rate(lambda: query.obb_overlap(swept, sc_, su_, k, count=True), n_sweep, few),
                                   "hull": rate(lambda: query.box_overlap(walk, gl, gh, k, count=True), n_walk, args.calls)}
        out["kinds"][name] = res
    walk.close()
    swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
