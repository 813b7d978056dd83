#!/usr/bin/env python3
"""tools/segment_rates.py [--calls K]: queries per second of the segment queries (include/ezrt_segment.h).

One JSON line.  Scene: the Bunny scene of C2 (bunny_scene(subdiv=2), 79 820 triangles).  Segments of 0.1, 1 and 10 leaf sizes (leaf =
the median longest side of the triangles' bounding boxes, as in tools/tri_distance_rates.py), random direction, in two placements --
  near     the middle within two leaf sizes of a point of the surface
  far      the middle uniform in the scene's bounding box moved out by half its extent
and per length and placement: `walk` = segment_distance_kernel<true>, `at` = segment_distance_at on the walk's winners and, on the SAME
segments in the same run, `sliver` = query.tri_distance on the triangles (a, b, midpoint + 1e-3 * length * a normal of the segment) and
`midpoint` = query.closest_point on the midpoints: what the dedicated rule buys over the two detours.  Then, on the near segments of
one leaf size: `tight` = segment_distance with d_max = a quarter of a leaf size; `capsule` = capsule_overlap(max_k=8, count=True) at
radii of 0.1, 1 and 10 leaf sizes (fewer capsules per call at the largest); `sweep` = the two kernels' <false> instances on the same
arrays created so that the scene does not prune, 2 048 queries per call.  Each figure is timed with hipEvents around `calls`
back-to-back calls on one stream after a warm-up call; the rate is Mqueries/s.  The two routes' answers are compared on the sweep's
queries (they must be equal); nothing else is checked here (tests/test_gpu_segment.py)."""
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
    ap.add_argument("--segs", type=int, default=1 << 16)
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

    gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    sc = scenes.bunny_scene(subdiv=2, hdr="shipped")
    tri, nodes = sc.tri, sc.nodes
    P = tri[:, :9].reshape(-1, 3, 3)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    leaf = float(np.median((P.max(1) - P.min(1)).max(1)))
    walk, swept = hip.scene_create(tri, nodes), hip.scene_create(tri, second_parent(nodes))
    assert walk.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    out = {"tool": "segment_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mqueries/s", "triangles": int(tri.shape[0]), "leaf": round(leaf, 5), "distance": {}, "capsule": {}, "sweep": {}}
    n, n_sweep = args.segs, 1 << 11
    few = max(1, args.calls // 5)
    k = rng.integers(0, P.shape[0], n)
    w = rng.dirichlet((1, 1, 1), n)
    on = (P[k] * w[:, :, None]).sum(1)
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    side = np.cross(d, rng.normal(0, 1, (n, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    mid = {"near": on + rng.normal(0, leaf, (n, 3)), "far": rng.uniform(lo, hi, (n, 3)) + 0.5 * (hi - lo)}
    for length in (0.1, 1.0, 10.0):
        for place in ("near", "far"):
            L = length * leaf
            a, b = mid[place] - 0.5 * L * d, mid[place] + 0.5 * L * d
            segs = gpu(np.concatenate([a, b], 1))
            sliver = gpu(np.concatenate([a, b, mid[place] + 1e-3 * L * side], 1))
            points = gpu(mid[place])
            r = query.segment_distance(walk, segs)
            torch.cuda.synchronize()
            hit = r.tri >= 0
            out["distance"]["%g_%s" % (length, place)] = {
                "segs": n, "crosses": round(float(r.crosses.float().mean().item()), 4),
                "mean_dist_in_leaves": round(float((r.dist[hit].mean() / leaf).item()), 3),
                "walk": rate(lambda: query.segment_distance(walk, segs), n, args.calls),
                "at": rate(lambda: query.segment_distance_at(walk, segs, r.tri), n, args.calls),
                "sliver": rate(lambda: query.tri_distance(walk, sliver), n, args.calls),
                "midpoint": rate(lambda: query.closest_point(walk, points), n, args.calls)}
    a, b = mid["near"] - 0.5 * leaf * d, mid["near"] + 0.5 * leaf * d
    segs = gpu(np.concatenate([a, b], 1))
    ss = segs[:n_sweep].contiguous()
    tight = torch.full((n,), 0.25 * leaf, dtype=torch.float32, device=dev)
    r = query.segment_distance(walk, segs, tight)
    torch.cuda.synchronize()
    out["distance"]["1_near_tight"] = {"segs": n, "d_max": round(0.25 * leaf, 5), "hit": round(float((r.tri >= 0).float().mean().item()), 4),
                                       "walk": rate(lambda: query.segment_distance(walk, segs, tight), n, args.calls)}
    for radius in (0.1, 1.0, 10.0):
        m = n if radius < 10 else n // 16
        sm, rad = segs[:m].contiguous(), torch.full((m,), radius * leaf, dtype=torch.float32, device=dev)
        c = query.capsule_overlap(walk, sm, rad, 8, count=True)
        torch.cuda.synchronize()
        out["capsule"]["%g" % radius] = {"capsules": m, "mean_count": round(float(c.n_overlap.float().mean().item()), 2),
                                         "over_max_k": round(float((c.n_overlap > 8).float().mean().item()), 4),
                                         "walk": rate(lambda: query.capsule_overlap(walk, sm, rad, 8, count=True), m, args.calls)}
    rs = torch.full((n_sweep,), leaf, dtype=torch.float32, device=dev)
    wa, sa = query.segment_distance(walk, ss), query.segment_distance(swept, ss)
    wc, sc_ = query.capsule_overlap(walk, ss, rs, 8, count=True), query.capsule_overlap(swept, ss, rs, 8, count=True)
    torch.cuda.synchronize()
    out["sweep"] = {"queries": n_sweep,
                    "routes_equal": bool(all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(tuple(wa) + tuple(wc), tuple(sa) + tuple(sc_)))),
                    "distance": rate(lambda: query.segment_distance(swept, ss), n_sweep, few),
                    "capsule": rate(lambda: query.capsule_overlap(swept, ss, rs, 8, count=True), n_sweep, few)}
    walk.close()
    swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
