#!/usr/bin/env python3
"""tools/closest_point_rates.py [--calls K]: points per second of the closest-point query (include/ezrt_closest_point.h), both routes.

One JSON line.  Scenes: the Bunny scene of C2 (bunny_scene(subdiv=2)) and the largest BASELINE scene (C5: mega_scene, 10^6 triangles).
Points: `near` -- vertices of the mesh moved by up to 1e-3 of the scene's size in a random direction -- and `far` -- on a sphere of
10 x the scene's size around its centre.
  pruned    closest_point_kernel<true>: the best-first walk over the 4-wide records (the scene as created)
  sweep     closest_point_kernel<false>: every triangle, no tree -- the same arrays created with one leaf given a second parent, so
            that the scene does not prune (what tests/allhits_scenes.py calls not_nested); fewer points per call, it is n x n_tri work
Each is timed with hipEvents around `calls` back-to-back calls on one stream after a warm-up call; the rate is Mpoints/s, and
pruned_vs_sweep their ratio.  The two routes' answers are compared on the sweep's points (they must be equal); nothing else is
checked here (tests/test_gpu_closest_point.py)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def second_parent(nodes):
    """`nodes` with a leaf referenced by two inner nodes: the boxes are no longer a tree, the scene does not prune"""
    nodes = nodes.copy()
    is_leaf = nodes[:, 3] > 0
    q = next(i for i in range(2, nodes.shape[0]) if not is_leaf[i] and is_leaf[int(nodes[i, 0])])
    nodes[q, 0] = np.float32(next(i for i in range(int(nodes[q, 0]) + 50, nodes.shape[0]) if is_leaf[i]))
    return nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--points", type=int, default=1 << 18)
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
        return n * calls / (e0.elapsed_time(e1) * 1e-3) / 1e6

    out = {"tool": "closest_point_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mpoints/s", "scenes": {}}
    for name, make, n_sweep in (("bunny", lambda: scenes.bunny_scene(subdiv=2, hdr="shipped"), 1 << 14),
                                ("mega", lambda: scenes.mega_scene(), 1 << 12)):
        sc = make()
        tri, nodes = sc.tri, sc.nodes
        V = tri[:, :9].reshape(-1, 3)
        lo, hi = V.min(0), V.max(0)
        size = float((hi - lo).max())
        d = rng.normal(size=(args.points, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        near = V[rng.integers(0, V.shape[0], args.points)] + d * size * 1e-3 * rng.random((args.points, 1))
        far = (lo + hi) / 2 + d * size * 10.0
        pruned, swept = hip.scene_create(tri, nodes), hip.scene_create(tri, second_parent(nodes))
        assert pruned.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
        res = {"triangles": int(tri.shape[0]), "points_pruned": args.points, "points_sweep": n_sweep}
        for what, pts in (("near", near), ("far", far)):
            p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
            ps = p[:n_sweep].contiguous()
            a, b = query.closest_point(pruned, ps), query.closest_point(swept, ps)
            torch.cuda.synchronize()
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
            rp = rate(lambda: query.closest_point(pruned, p), args.points, args.calls)
            rs = rate(lambda: query.closest_point(swept, ps), n_sweep, max(1, args.calls // 5))
            res[what] = {"pruned": round(rp, 3), "sweep": round(rs, 4), "pruned_vs_sweep": round(rp / rs, 1), "routes_equal": same}
        out["scenes"][name] = res
        pruned.close()
        swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
