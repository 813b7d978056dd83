#!/usr/bin/env python3
"""tools/query_rates.py [--calls K]: rays per second of the stream-ordered device queries (include/ezrt_query.h) on the C2 scene.

One JSON line.  Ray sets, each at n = 2^20 and 2^22:
  primary   the C2 camera's primary rays (jittered pixel centres of its 512 x 512 frame, repeated)
  bounce    diffuse (cosine-weighted) bounce rays from the primary hit points, origins offset 1e-3 along the geometric normal
  segment   from those offset hit points to random points above the scene, t_max = the distance (unit directions)
Per set and n: ezrt_query_closest_device and ezrt_query_occluded_device (t_max = None for primary / bounce), each timed with
hipEvents around K back-to-back calls on one stream after a warm-up call; beside them ezrt_query_hits (host arrays: copies,
synchronisation and all, wall clock, no t_max) on the same rays.  Results are not checked here (tests/test_gpu_query_device.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_rays(eye, cam, w, h, n, rng):
    m = np.asarray(cam, np.float64).reshape(4, 4).T
    k = np.arange(n) % (w * h)
    xs, ys = k % w, k // w
    px = (xs + rng.random(n)) / w * 2 - 1
    py = (ys + rng.random(n)) / h * 2 - 1
    d = px[:, None] * m[:3, 0] + py[:, None] * m[:3, 1] - 1.5 * m[:3, 2]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(np.asarray(eye, np.float64), d.shape)
    return np.concatenate([o, d], 1).astype(np.float32)


def hit_points(tri, rays, tri_id, t):
    """offset hit points and geometric normals (facing the incoming ray) of the rays that hit"""
    h = tri_id >= 0
    r, ti, tt = rays[h].astype(np.float64), tri_id[h], t[h].astype(np.float64)
    P = tri[ti, :9].reshape(-1, 3, 3).astype(np.float64)
    N = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    N /= np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-30)
    N = np.where((N * r[:, 3:]).sum(1, keepdims=True) > 0, -N, N)
    p = r[:, :3] + r[:, 3:] * tt[:, None]
    return p + 1e-3 * N, N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    from ezrt_amd import query, scene as S, scenes, trace
    from ezrt_amd.srchash import gpu_source_hash
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    cfg = scenes.CONFIGS["C2"]
    bs = scenes.bunny_scene(subdiv=2, hdr="shipped")          # bench.py's C2 scene
    sg = bs.upload(hip)
    eye, cam = S.camera(*cfg["camera"])
    rng = np.random.default_rng(7)
    stream = torch.cuda.current_stream(dev)
    P = bs.tri[:, :9].reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)

    def rate_device(fn, rays, t_max):
        fn(sg, rays, t_max)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            fn(sg, rays, t_max)
        e1.record(stream)
        e1.synchronize()
        return rays.shape[0] * args.calls / (e0.elapsed_time(e1) * 1e-3)

    def rate_host(rays_np):
        sg.query_hits(rays_np)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            sg.query_hits(rays_np)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return rays_np.shape[0] / best

    out = {"tool": "query_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev),
           "scene": "C2: bunny_scene(subdiv=2), %d triangles, camera %s" % (bs.tri.shape[0], tuple(cfg["camera"])),
           "calls": args.calls, "unit": "rays/s", "rates": {}}
    for logn in (20, 22):
        n = 1 << logn
        prim = camera_rays(eye, cam, cfg["width"], cfg["height"], n, rng)
        g = torch.from_numpy(prim).to(dev)
        tri, t = query.closest(sg, g)
        torch.cuda.synchronize()
        tri, t = tri.cpu().numpy(), t.cpu().numpy()
        o, N = hit_points(bs.tri, prim, tri, t)
        pick = rng.integers(0, o.shape[0], n)                     # n rays from the hit points (with repetition)
        o, N = o[pick], N[pick]
        # cosine-weighted directions about N
        u1, u2 = rng.random(n), rng.random(n)
        a = np.where(np.abs(N[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
        T = np.cross(N, a)
        T /= np.linalg.norm(T, axis=1, keepdims=True)
        B = np.cross(N, T)
        r, phi = np.sqrt(u1)[:, None], 2 * np.pi * u2[:, None]
        d = r * np.cos(phi) * T + r * np.sin(phi) * B + np.sqrt(1 - u1)[:, None] * N
        bounce = np.concatenate([o, d], 1).astype(np.float32)
        tgt = np.stack([rng.uniform(lo[0], hi[0], n), hi[1] + rng.uniform(0.5, 2.0, n), rng.uniform(lo[2], hi[2], n)], 1)
        v = tgt - o
        dist = np.linalg.norm(v, axis=1)
        seg = np.concatenate([o, v / dist[:, None]], 1).astype(np.float32)
        for name, rays_np, tm in (("primary", prim, None), ("bounce", bounce, None), ("segment", seg, dist.astype(np.float32))):
            rays = torch.from_numpy(rays_np).to(dev)
            t_max = torch.from_numpy(tm).to(dev) if tm is not None else None
            occ = query.occluded(sg, rays, t_max)
            torch.cuda.synchronize()
            out["rates"]["%s_2^%d" % (name, logn)] = {
                "closest_device": round(rate_device(query.closest, rays, t_max)),
                "occluded_device": round(rate_device(query.occluded, rays, t_max)),
                "query_hits_host": round(rate_host(rays_np)),
                "occluded_share": round(float(occ.float().mean()), 4),
            }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
