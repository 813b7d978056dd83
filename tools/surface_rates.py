#!/usr/bin/env python3
"""tools/surface_rates.py [--calls K]: rays per second of the surface query (include/ezrt_surface.h) beside the closest-hit query
(include/ezrt_query.h) on the C2 scene.

One JSON line.  Ray sets, each at n = 2^20 and 2^22:
  primary   the C2 camera's primary rays (jittered pixel centres of its 512 x 512 frame, repeated)
  bounce    cosine-weighted rays about the shading normal from the primary hit points, both taken from query.surface itself, origins
            offset 1e-3 along that normal
Per set and n: ezrt_query_closest_device and ezrt_query_surface_device with every output (integrator 50), each timed with
hipEvents around K back-to-back calls on one stream after a warm-up call.  Results are not checked here
(tests/test_gpu_surface_query.py)."""
import argparse
import json
import os
import sys

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

    def rate(fn, rays):
        fn(sg, rays)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            fn(sg, rays)
        e1.record(stream)
        e1.synchronize()
        return rays.shape[0] * args.calls / (e0.elapsed_time(e1) * 1e-3)

    out = {"tool": "surface_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev),
           "scene": "C2: bunny_scene(subdiv=2), %d triangles, camera %s" % (bs.tri.shape[0], tuple(cfg["camera"])),
           "calls": args.calls, "unit": "rays/s", "rates": {}}
    for logn in (20, 22):
        n = 1 << logn
        prim = torch.from_numpy(camera_rays(eye, cam, cfg["width"], cfg["height"], n, rng)).to(dev)
        r = query.surface(sg, prim)
        torch.cuda.synchronize()
        hit = (r.tri >= 0).nonzero().squeeze(1)
        pick = hit[torch.from_numpy(rng.integers(0, hit.numel(), n)).to(dev)]   # n rays from the hit points (with repetition)
        N = r.normal[pick].double()
        o = r.point[pick].double() + 1e-3 * N
        # cosine-weighted directions about the shading normal
        u1 = torch.from_numpy(rng.random(n)).to(dev)[:, None]
        u2 = torch.from_numpy(rng.random(n)).to(dev)[:, None]
        a = torch.where(N[:, :1].abs() > 0.9, torch.tensor([[0.0, 1.0, 0.0]], device=dev, dtype=torch.float64),
                        torch.tensor([[1.0, 0.0, 0.0]], device=dev, dtype=torch.float64))
        T = torch.linalg.cross(N, a)
        T = T / T.norm(dim=1, keepdim=True)
        B = torch.linalg.cross(N, T)
        rr, phi = u1.sqrt(), 2 * np.pi * u2
        d = rr * phi.cos() * T + rr * phi.sin() * B + (1 - u1).sqrt() * N
        bounce = torch.cat([o, d], 1).float().contiguous()
        for name, rays in (("primary", prim), ("bounce", bounce)):
            c = rate(lambda s, x: query.closest(s, x), rays)
            f = rate(lambda s, x: query.surface(s, x), rays)
            hits = float((query.closest(sg, rays)[0] >= 0).float().mean())
            out["rates"]["%s_2^%d" % (name, logn)] = {"closest_device": round(c), "surface_device": round(f),
                                                      "surface_time_over_closest": round(c / f, 3), "hit_share": round(hits, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
