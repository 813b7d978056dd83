#!/usr/bin/env python3
"""tools/tri_overlap_rates.py [--calls K]: query triangles per second of the triangle-overlap queries (include/ezrt_tri_overlap.h).

One JSON line.  Scene: the Bunny scene of C2 (bunny_scene(subdiv=2)).  Query triangles: centred on points uniform in the scene's
bounding box, random orientation, at three sizes --
  leaf     a leaf-sized triangle: the median longest side of the triangles' bounding boxes
  eighth   1/8 of the scene's extent
  whole    one triangle spanning the scene (its bounding box holds the scene: n x n_tri work on both routes, so fewer per call)
and for max_k = 0 (count only), 8 and 64 (with the count).  For each the two routes side by side:
  walk     tri_overlap_kernel<true>: the depth-first walk over the 4-wide records (the scene as created)
  sweep    tri_overlap_kernel<false>: every triangle, no tree -- the same arrays created with one leaf given a second parent, so that
           the scene does not prune; fewer triangles per call
and, in the same run, `box` -- query.box_overlap on the same route with the query triangles' bounding boxes: the same walk with the
same gate, so the difference is the cost of the per-pair rule.  Each is timed with hipEvents around `calls` back-to-back calls on
one stream after a warm-up call; the rate is Mqueries/s.  The two routes' answers are compared on the sweep's triangles (they must be
equal); nothing else is checked here (tests/test_gpu_tri_overlap.py)."""
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
    ap.add_argument("--tris", type=int, default=1 << 17)
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
    out = {"tool": "tri_overlap_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mqueries/s", "triangles": int(tri.shape[0]), "sizes": {}}
    few = max(1, args.calls // 5)
    ext = float(np.max(hi - lo))
    # (circumradius, query triangles per call on the walk, on the sweep)
    sizes = {"leaf": (leaf / 2, args.tris, 1 << 13), "eighth": (ext / 16, args.tris, 1 << 13), "whole": (None, 1 << 11, 1 << 11)}
    for name, (radius, n_walk, n_sweep) in sizes.items():
        if name == "whole":                                           # one triangle through the middle whose bounding box holds the scene
            mid, e = (lo + hi) / 2, hi - lo
            t = np.tile((mid + np.array([[-3, -3, -0.5], [3, -3, 0.5], [0, 4, 0.0]]) * e)[None], (n_walk, 1, 1))
        else:
            c = rng.uniform(lo, hi, (n_walk, 1, 3))
            d = rng.normal(0, 1, (n_walk, 3, 3))
            t = c + radius * d / np.linalg.norm(d, axis=2, keepdims=True)
        tq = torch.from_numpy(np.ascontiguousarray(t.reshape(-1, 9), np.float32)).to(dev)
        bl, bh = tq.view(-1, 3, 3).amin(1).contiguous(), tq.view(-1, 3, 3).amax(1).contiguous()
        ts, sl, sh = tq[:n_sweep].contiguous(), bl[:n_sweep].contiguous(), bh[:n_sweep].contiguous()
        a, b = query.tri_overlap(walk, ts, 64, count=True), query.tri_overlap(swept, ts, 64, count=True)
        box = query.box_overlap(walk, sl, sh, 0, count=True)
        torch.cuda.synchronize()
        res = {"radius": None if radius is None else round(float(radius), 5), "tris_walk": n_walk, "tris_sweep": n_sweep,
               "routes_equal": bool(torch.equal(a.tri, b.tri) and torch.equal(a.n_overlap, b.n_overlap)),
               "mean_overlaps": round(float(a.n_overlap.float().mean().item()), 2),
               "mean_box_overlaps": round(float(box.n_overlap.float().mean().item()), 2)}
        for k in (0, 8, 64):
            res["max_k_%d" % k] = {"walk": rate(lambda: query.tri_overlap(walk, tq, k, count=True), n_walk, args.calls),
                                   "sweep": rate(lambda: query.tri_overlap(swept, ts, k, count=True), n_sweep, few),
                                   "box_walk": rate(lambda: query.box_overlap(walk, bl, bh, k, count=True), n_walk, args.calls),
                                   "box_sweep": rate(lambda: query.box_overlap(swept, sl, sh, k, count=True), n_sweep, few)}
        out["sizes"][name] = res
    walk.close()
    swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
