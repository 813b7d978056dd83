#!/usr/bin/env python3
"""tools/shade_rates.py [--calls K]: elements per second of every shading query (include/ezrt_shade.h) on first-hit data of the C2
scene, beside the time per element of the surface query (include/ezrt_surface.h) that produced that data.

One JSON line.  At n = 2^20 and 2^22: the C2 camera's primary rays (jittered pixel centres of its 512 x 512 frame, repeated) go
through query.surface (integrator 50); tri and N are its outputs (misses included: they take the zero path), V = minus the ray
direction, xi uniform random numbers, L for the evaluations = shade.sample(51)'s directions, L for the environment lookups =
shade.env_sample's.  Every call is timed with hipEvents around K back-to-back calls on one stream after a warm-up call; the
yardstick, ezrt_query_surface_device with every output, the same way on the same rays.  Results are not checked here
(tests/test_gpu_shade_query.py)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    from surface_rates import camera_rays
    from ezrt_amd import query, scene as S, scenes, shade, trace
    from ezrt_amd.srchash import gpu_source_hash
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    cfg = scenes.CONFIGS["C2"]
    bs = scenes.bunny_scene(subdiv=2, hdr="shipped", want_cache=True)          # bench.py's C2 scene, with the env cache
    sg = bs.upload(hip)
    eye, cam = S.camera(*cfg["camera"])
    rng = np.random.default_rng(7)
    stream = torch.cuda.current_stream(dev)

    def ns_per_element(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e6 / (n * args.calls)

    out = {"tool": "shade_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev),
           "scene": "C2: bunny_scene(subdiv=2), %d triangles, camera %s" % (bs.tri.shape[0], tuple(cfg["camera"])),
           "calls": args.calls, "unit": "elements/s; ns = nanoseconds per element", "rates": {}}
    for logn in (20, 22):
        n = 1 << logn
        rays = torch.from_numpy(camera_rays(eye, cam, cfg["width"], cfg["height"], n, rng)).to(dev)
        r = query.surface(sg, rays)
        tri, N = r.tri, r.normal
        V = (-rays[:, 3:6]).contiguous()
        xi3 = torch.from_numpy(rng.random((n, 3)).astype(np.float32)).to(dev)
        xi2 = xi3[:, 0:2].contiguous()
        L = shade.sample(sg, tri, xi3, V, N, integrator=51)
        Le = shade.env_sample(sg, xi2)
        torch.cuda.synchronize()
        calls = {"material": lambda: shade.material(sg, tri)}
        for integ in (3, 4, 50, 51, 52):
            calls["evaluate_%d" % integ] = lambda integ=integ: shade.evaluate(sg, tri, V, N, L, integrator=integ)
        calls["evaluate_51_no_pdf"] = lambda: shade.evaluate(sg, tri, V, N, L, integrator=51, want_pdf=False)
        for integ in (50, 51, 52):
            calls["sample_%d" % integ] = lambda integ=integ: shade.sample(sg, tri, xi3, V, N, integrator=integ)
        calls["env_evaluate_colour"] = lambda: shade.env_evaluate(sg, Le, want_pdf=False)
        calls["env_evaluate_pdf"] = lambda: shade.env_evaluate(sg, Le, want_colour=False)
        calls["env_evaluate_both"] = lambda: shade.env_evaluate(sg, Le)
        calls["env_sample"] = lambda: shade.env_sample(sg, xi2)
        surf_ns = ns_per_element(lambda: query.surface(sg, rays), n)
        res = {"hit_share": round(float((tri >= 0).float().mean()), 4), "surface_device_ns": round(surf_ns, 3)}
        for name, fn in calls.items():
            ns = ns_per_element(fn, n)
            res[name] = {"elements_per_s": round(1e9 / ns), "ns": round(ns, 4), "surface_device_ns": round(surf_ns, 3),
                         "time_over_surface": round(ns / surf_ns, 4)}
        out["rates"]["2^%d" % logn] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
