#!/usr/bin/env python3
"""tools/sphere_cast_rates.py [--calls K]: queries per second of the sphere-cast queries (include/ezrt_sphere_cast.h).

One JSON line.  Scene: the Bunny scene of C2 (bunny_scene(subdiv=2), 79 820 triangles).  Rays: origins on a shell of 0.7 .. 1.3
extents about the scene, unit directions at points of the surface.  Radii in leaf sizes (the median longest side of the triangles'
bounding boxes): small 0.1, medium 1, large 10.  For each radius --
  unbounded   t_max = NULL
  short       t_max = a tenth of the extent: most queries miss, and the second walk starts with that radius
and, once, `touching`: origins within a medium radius of the surface, where the first walk answers and the second never runs.
For each: `walk` = sphere_cast_kernel<true> (the scene as created), `sweep` = sphere_cast_kernel<false> (the same arrays created so
that the scene does not prune; fewer rays per call), `at` = sphere_cast_at on the walk's winners, and for scale, in the same run on the
same rays and origins, `closest` = query.closest (the ray without thickness) and `closest_point` = query.closest_point(o, d_max = r)
(the first of the two walks alone).  Each is timed with hipEvents around `calls` back-to-back calls on one stream after a warm-up
call; the rate is Mqueries/s.  The two routes' answers are compared on the sweep's rays (they must be equal); nothing else is checked
here (tests/test_gpu_sphere_cast.py)."""
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
    ap.add_argument("--rays", type=int, default=1 << 18)
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
    size = float(np.max(hi - lo))
    leaf = float(np.median((P.max(1) - P.min(1)).max(1)))
    walk, swept = hip.scene_create(tri, nodes), hip.scene_create(tri, second_parent(nodes))
    assert walk.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    out = {"tool": "sphere_cast_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mqueries/s", "triangles": int(tri.shape[0]), "leaf": round(leaf, 5), "extent": round(size, 4), "cases": {}}
    n, n_sweep = args.rays, 1 << 11
    few = max(1, args.calls // 5)
    k = rng.integers(0, P.shape[0], n)
    w = rng.dirichlet((1, 1, 1), n)
    on = (P[k] * w[:, :, None]).sum(1)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = 0.5 * (lo + hi) + u * size * rng.uniform(0.7, 1.3, (n, 1))
    d = on - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = np.concatenate([o, d], 1)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    close = np.concatenate([on + v * leaf * rng.uniform(0, 1, (n, 1)), d], 1)
    cases = [("%s_%s" % (a, b), shell, r * leaf, tm) for a, r in (("small", 0.1), ("medium", 1.0), ("large", 10.0))
             for b, tm in (("unbounded", None), ("short", 0.1 * size))] + [("touching", close, leaf, None)]
    for name, rays, r, tm in cases:
        q = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(dev)
        rad = torch.full((n,), r, dtype=torch.float32, device=dev)
        t_max = None if tm is None else torch.full((n,), tm, dtype=torch.float32, device=dev)
        qs, rs, ts = q[:n_sweep].contiguous(), rad[:n_sweep].contiguous(), None if tm is None else t_max[:n_sweep].contiguous()
        a, b = query.sphere_cast(walk, q, rad, t_max), query.sphere_cast(swept, qs, rs, ts)
        torch.cuda.synchronize()
        pts = q[:, :3].contiguous()
        res = {"rays_walk": n, "rays_sweep": n_sweep, "radius": round(r, 5), "t_max": None if tm is None else round(tm, 5),
               "routes_equal": bool(all(torch.equal(x[:n_sweep].view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))),
               "hit": round(float((a.tri >= 0).float().mean().item()), 4), "touching": round(float(a.touching.float().mean().item()), 4),
               "walk": rate(lambda: query.sphere_cast(walk, q, rad, t_max), n, args.calls),
               "sweep": rate(lambda: query.sphere_cast(swept, qs, rs, ts), n_sweep, few),
               "at": rate(lambda: query.sphere_cast_at(walk, q, rad, a.tri), n, args.calls),
               "closest": rate(lambda: query.closest(walk, q, t_max), n, args.calls),
               "closest_point": rate(lambda: query.closest_point(walk, pts, rad), n, args.calls)}
        out["cases"][name] = res
    walk.close()
    swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
