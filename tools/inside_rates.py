#!/usr/bin/env python3
"""tools/inside_rates.py [--calls K]: points per second of the inside and signed-distance queries (include/ezrt_inside.h).

One JSON line.  Scenes: the Bunny scene of C2 (bunny_scene(subdiv=2)) and the largest BASELINE scene (C5: mega_scene, 10^6 triangles).
Points: uniform in the scene's bounding box.  Axis 0 (+x) unless --axis says otherwise.
  inside.walk        inside_kernel<true>: the depth-first walk over the 4-wide records (the scene as created)
  inside.sweep       inside_kernel<false>: every triangle, no tree -- the same arrays created with one leaf given a second parent, so
                     that the scene does not prune; fewer points per call, it is n x n_tri work
  signed_distance    signed_distance_kernel<true>: the crossing walk and the closest-point walk in one launch
  closest_point      query.closest_point on the same points in the same run: the yardstick, its kernel does not change
Each is timed with hipEvents around `calls` back-to-back calls on one stream after a warm-up call; the rate is Mpoints/s.  The two
routes' answers are compared on the sweep's points (they must be equal); nothing else is checked here (tests/test_gpu_inside.py)."""
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
    ap.add_argument("--points", type=int, default=1 << 18)
    ap.add_argument("--axis", type=int, default=0)
    ap.add_argument("--scenes", default="bunny,mega")
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
        return round(n * calls / (e0.elapsed_time(e1) * 1e-3) / 1e6, 3)

    out = {"tool": "inside_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mpoints/s", "axis": args.axis, "scenes": {}}
    makers = {"bunny": (lambda: scenes.bunny_scene(subdiv=2, hdr="shipped"), 1 << 14), "mega": (lambda: scenes.mega_scene(), 1 << 12)}
    for name in args.scenes.split(","):
        make, n_sweep = makers[name]
        sc = make()
        tri, nodes = sc.tri, sc.nodes
        V = tri[:, :9].reshape(-1, 3)
        lo, hi = V.min(0), V.max(0)
        pts = rng.uniform(lo, hi, (args.points, 3))
        walk, swept = hip.scene_create(tri, nodes), hip.scene_create(tri, second_parent(nodes))
        assert walk.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
        p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
        ps = p[:n_sweep].contiguous()
        a, b = query.inside(walk, ps, args.axis, crossings=True), query.inside(swept, ps, args.axis, crossings=True)
        torch.cuda.synchronize()
        few = max(1, args.calls // 5)
        res = {"triangles": int(tri.shape[0]), "points_walk": args.points, "points_sweep": n_sweep,
               "routes_equal": bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])),
               "inside_fraction": round(float(a[0].float().mean().item()), 4), "mean_crossings": round(float(a[1].float().mean().item()), 3),
               "inside": {"walk": rate(lambda: query.inside(walk, p, args.axis), args.points, args.calls),
                          "sweep": rate(lambda: query.inside(swept, ps, args.axis), n_sweep, few)},
               "signed_distance": rate(lambda: query.signed_distance(walk, p, axis=args.axis), args.points, args.calls),
               "closest_point": rate(lambda: query.closest_point(walk, p), args.points, args.calls)}
        res["inside_vs_closest_point"] = round(res["inside"]["walk"] / res["closest_point"], 3)
        res["signed_distance_vs_sum"] = round(res["signed_distance"] * (1 / res["inside"]["walk"] + 1 / res["closest_point"]), 3)
        out["scenes"][name] = res
        walk.close()
        swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
