#!/usr/bin/env python3
"""tools/tri_distance_rates.py [--calls K]: query triangles per second of the triangle-distance queries (include/ezrt_tri_distance.h).

One JSON line.  Scene: the Bunny scene of C2 (bunny_scene(subdiv=2), 79 820 triangles).  Query triangles: leaf-sized (circumradius =
half the median longest side of the triangles' bounding boxes), random orientation, in three placements --
  near     centred within two leaf sizes of a point of the surface: the tool close to the part
  far      centred on points uniform in the scene's bounding box moved out by half its extent: nothing is close, the radius shrinks late
  tight    the near triangles with d_max = a quarter of a leaf size: a clearance check; most queries miss, and the walk starts with
           that radius
For each: `walk` = tri_distance_kernel<true> (the scene as created), `sweep` = tri_distance_kernel<false> (the same arrays created so
that the scene does not prune; fewer triangles per call), `at` = tri_distance_at on the walk's winners, and for scale, in the same
run on the same query triangles, `overlap_walk` = query.tri_overlap(max_k=8, count=True).  Each is timed with hipEvents around `calls`
back-to-back calls on one stream after a warm-up call; the rate is Mqueries/s.  The two routes' answers are compared on the sweep's
triangles (they must be equal); nothing else is checked here (tests/test_gpu_tri_distance.py)."""
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
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--tris", type=int, default=1 << 16)
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
    out = {"tool": "tri_distance_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mqueries/s", "triangles": int(tri.shape[0]), "leaf": round(leaf, 5), "placements": {}}
    n, n_sweep = args.tris, 1 << 11
    few = max(1, args.calls // 5)
    k = rng.integers(0, P.shape[0], n)
    w = rng.dirichlet((1, 1, 1), n)
    on = (P[k] * w[:, :, None]).sum(1)
    d = rng.normal(0, 1, (n, 3, 3))
    shape = 0.5 * leaf * d / np.linalg.norm(d, axis=2, keepdims=True)
    near = on[:, None, :] + rng.normal(0, leaf, (n, 1, 3)) + shape
    far = (rng.uniform(lo, hi, (n, 3)) + 0.5 * (hi - lo))[:, None, :] + shape
    for name, t, dm in (("near", near, None), ("far", far, None), ("tight", near, 0.25 * leaf)):
        tq = torch.from_numpy(np.ascontiguousarray(t.reshape(-1, 9), np.float32)).to(dev)
        ts = tq[:n_sweep].contiguous()
        d_max = None if dm is None else torch.full((n,), dm, dtype=torch.float32, device=dev)
        ds = None if dm is None else d_max[:n_sweep].contiguous()
        a, b = query.tri_distance(walk, tq, d_max), query.tri_distance(swept, ts, ds)
        torch.cuda.synchronize()
        hit = a.tri >= 0
        res = {"tris_walk": n, "tris_sweep": n_sweep, "d_max": None if dm is None else round(dm, 5),
               "routes_equal": bool(all(torch.equal(x[:n_sweep].view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))),
               "hit": round(float(hit.float().mean().item()), 4), "crosses": round(float(a.crosses.float().mean().item()), 4),
               "mean_dist_in_leaves": round(float((a.dist[hit].mean() / leaf).item()), 3) if bool(hit.any()) else None,
               "walk": rate(lambda: query.tri_distance(walk, tq, d_max), n, args.calls),
               "sweep": rate(lambda: query.tri_distance(swept, ts, ds), n_sweep, few),
               "at": rate(lambda: query.tri_distance_at(walk, tq, a.tri), n, args.calls),
               "overlap_walk": rate(lambda: query.tri_overlap(walk, tq, 8, count=True), n, args.calls)}
        out["placements"][name] = res
    walk.close()
    swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
