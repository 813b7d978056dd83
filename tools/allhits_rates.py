#!/usr/bin/env python3
"""tools/allhits_rates.py [--calls K]: rays per second of the all-hits query (include/ezrt_multihit.h) on C2, beside query.closest.

One JSON line.  The work is the primary rays of one 512 x 512 frame of the C2 scene from its camera (262 144 rays, from
ezrt_camera_rays_device).
  closest            ezrt_query_closest_device (the render calls' 4-wide kernel and its redo launch: pruned, nearest first)
  all_hits_K         ezrt_query_all_hits_device with max_hits = K for K = 1, 4, 16, 64 (all_hits_kernel: one ray per lane on the
                     binary tree, unpruned, the sorted list kept in the ray's output row of K entries)
Each is timed with hipEvents around `calls` back-to-back calls on one stream after a warm-up call.  Also printed: the mean and the
largest number of crossings per ray.  Results are not checked here (tests/test_gpu_allhits.py)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import torch
    from ezrt_amd import path, query, scene as S, scenes, trace
    from ezrt_amd.srchash import gpu_source_hash
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    cfg = scenes.CONFIGS["C2"]
    bs = scenes.bunny_scene(subdiv=2, hdr="shipped")          # bench.py's C2 scene
    sg = bs.upload(hip)
    eye, cam = S.camera(*cfg["camera"])
    w, h = cfg["width"], cfg["height"]
    n = w * h
    stream = torch.cuda.current_stream(dev)
    ys, xs = np.mgrid[0:h, 0:w]
    xyf = torch.from_numpy(np.stack([xs.ravel(), ys.ravel(), np.zeros(n)], 1).astype(np.int32)).to(dev)
    rays = path.camera_rays(sg, trace.make_params(w, h, eye, cam, cfg["integrator"], cfg["max_bounce"]), xyf)

    def rate(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return n * args.calls / (e0.elapsed_time(e1) * 1e-3)

    count = query.all_hits(sg, rays, 1)[2]
    out = {"tool": "allhits_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev),
           "scene": "C2: bunny_scene(subdiv=2), %d triangles, camera %s, %d x %d primary rays" % (bs.tri.shape[0], tuple(cfg["camera"]), w, h),
           "calls": args.calls, "rays_per_call": n, "unit": "rays/s", "crossings_mean": round(float(count.float().mean()), 3),
           "crossings_max": int(count.max()), "rates": {}}
    out["rates"]["closest"] = round(rate(lambda: query.closest(sg, rays)))
    for K in (1, 4, 16, 64):
        out["rates"]["all_hits_%d" % K] = round(rate(lambda: query.all_hits(sg, rays, K)))
        out["all_hits_%d_vs_closest" % K] = round(out["rates"]["all_hits_%d" % K] / out["rates"]["closest"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
