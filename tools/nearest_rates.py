#!/usr/bin/env python3
"""tools/nearest_rates.py [--calls K]: points per second of the nearest-K query (include/ezrt_nearest.h) on the Bunny scene.

One JSON line.  Scene: the Bunny scene of C2 (bunny_scene(subdiv=2)).  Points: vertices of the mesh moved by up to 1e-3 of the scene's
size in a random direction (tools/closest_point_rates.py's `near`).  d_max: 5 % of the scene's size, for every point.
  pruned    nearest_kernel<true, .>: the best-first walk over the 4-wide records (the scene as created)
  sweep     nearest_kernel<false, .>: every triangle, no tree -- the same arrays created with one leaf given a second parent, so that
            the scene does not prune; fewer points per call, it is n x n_tri work
for K = 1, 8 and 64, with the count (`count`: the radius stays at d_max) and without it (`list`: the radius shrinks to the K-th entry),
both with that d_max, and `list_unbounded` without any d_max.  closest_point = query.closest_point on the same points in the same run,
with and without the same d_max: the yardstick, its kernel does not change.  vs_closest_point = nearest(K = 1, list) / closest_point.
Each is timed with hipEvents around `calls` back-to-back calls on one stream after a warm-up call; the rate is Mpoints/s.  The two
routes' answers are compared on the sweep's points (they must be equal); nothing else is checked here (tests/test_gpu_nearest.py)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from closest_point_rates import second_parent  # noqa: E402

KS = (1, 8, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--points", type=int, default=1 << 18)
    ap.add_argument("--points-sweep", type=int, default=1 << 14)
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

    sc = scenes.bunny_scene(subdiv=2, hdr="shipped")
    tri, nodes = sc.tri, sc.nodes
    V = tri[:, :9].reshape(-1, 3)
    size = float((V.max(0) - V.min(0)).max())
    d = rng.normal(size=(args.points, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    near = V[rng.integers(0, V.shape[0], args.points)] + d * size * 1e-3 * rng.random((args.points, 1))
    pruned, swept = hip.scene_create(tri, nodes), hip.scene_create(tri, second_parent(nodes))
    assert pruned.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    p = torch.from_numpy(np.ascontiguousarray(near, np.float32)).to(dev)
    ps = p[:args.points_sweep].contiguous()
    dm = torch.full((args.points,), 0.05 * size, dtype=torch.float32, device=dev)
    dms = dm[:args.points_sweep].contiguous()
    out = {"tool": "nearest_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mpoints/s", "scene": "bunny", "triangles": int(tri.shape[0]), "d_max": round(0.05 * size, 5),
           "points_pruned": args.points, "points_sweep": args.points_sweep}
    few = max(1, args.calls // 5)
    out["closest_point"] = {"pruned": rate(lambda: query.closest_point(pruned, p, dm), args.points, args.calls),
                            "pruned_unbounded": rate(lambda: query.closest_point(pruned, p), args.points, args.calls),
                            "sweep": rate(lambda: query.closest_point(swept, ps, dms), args.points_sweep, few)}
    same = True
    within = None
    for k in KS:
        a, b = query.nearest(pruned, ps, k, dms, True), query.nearest(swept, ps, k, dms, True)
        torch.cuda.synchronize()
        same = same and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        within = a.count.float().mean().item()
        out["K=%d" % k] = {
            "pruned": {"list": rate(lambda: query.nearest(pruned, p, k, dm), args.points, args.calls),
                       "count": rate(lambda: query.nearest(pruned, p, k, dm, True), args.points, args.calls),
                       "list_unbounded": rate(lambda: query.nearest(pruned, p, k), args.points, args.calls)},
            "sweep": {"list": rate(lambda: query.nearest(swept, ps, k, dms), args.points_sweep, few),
                      "count": rate(lambda: query.nearest(swept, ps, k, dms, True), args.points_sweep, few)}}
    out["mean_within_d_max"] = round(within, 1)
    out["routes_equal"] = same
    out["vs_closest_point"] = {"pruned": round(out["K=1"]["pruned"]["list"] / out["closest_point"]["pruned"], 3),
                               "pruned_unbounded": round(out["K=1"]["pruned"]["list_unbounded"] / out["closest_point"]["pruned_unbounded"], 3),
                               "sweep": round(out["K=1"]["sweep"]["list"] / out["closest_point"]["sweep"], 3)}
    pruned.close()
    swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
