#!/usr/bin/env python3
"""tools/path_rates.py [--calls K] [--yardstick-lib PATH]: paths per second of the device path queries (include/ezrt_path.h) on C2.

One JSON line.  The work is one 512 x 512 frame of the C2 scene from its camera: 262 144 paths of integrator 50 with 4 bounces.
  camera_rays      ezrt_camera_rays_device for every pixel of the frame
  radiance         ezrt_query_radiance_device along those rays (radiance_query_kernel: one path per lane)
  rays+radiance    both, back to back
  yardstick        ezrt_render_device of the same frame (spp = 1) with option megakernel = 1: trace_kernel, the same bounce loop on
                   the same one-lane schedule, plus its accumulation kernel.  --yardstick-lib names the library whose render call
                   is measured (a build of the parent commit, say); default: the product library itself.
Each is timed with hipEvents around K back-to-back calls on one stream after a warm-up call, frame index k for call k.  The
query adds 48 B of input and output per path (24 B ray + 12 B pixel-sample in, 12 B radiance out) to what the render call moves.
Results are not checked here (tests/test_gpu_path_query.py)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--yardstick-lib", default=None)
    args = ap.parse_args()
    import torch
    from ezrt_amd import _abi, path, scene as S, scenes, trace
    from ezrt_amd.srchash import gpu_source_hash
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    cfg = scenes.CONFIGS["C2"]
    bs = scenes.bunny_scene(subdiv=2, hdr="shipped")          # bench.py's C2 scene
    sg = bs.upload(hip)
    eye, cam = S.camera(*cfg["camera"])
    w, h, integ, mb = cfg["width"], cfg["height"], cfg["integrator"], cfg["max_bounce"]
    n = w * h
    stream = torch.cuda.current_stream(dev)
    ys, xs = np.mgrid[0:h, 0:w]
    xyf = [torch.from_numpy(np.stack([xs.ravel(), ys.ravel(), np.full(n, k)], 1).astype(np.int32)).to(dev) for k in range(args.calls)]
    p = trace.make_params(w, h, eye, cam, integ, mb)

    def rate(fn):
        fn(0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(args.calls):
            fn(k)
        e1.record(stream)
        e1.synchronize()
        return n * args.calls / (e0.elapsed_time(e1) * 1e-3)

    rays = [path.camera_rays(sg, p, x) for x in xyf]
    out = {"tool": "path_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev),
           "scene": "C2: bunny_scene(subdiv=2), %d triangles, camera %s, %d x %d, integrator %d, %d bounces" % (
               bs.tri.shape[0], tuple(cfg["camera"]), w, h, integ, mb),
           "calls": args.calls, "paths_per_call": n, "unit": "paths/s", "rates": {}}
    out["rates"]["camera_rays"] = round(rate(lambda k: path.camera_rays(sg, p, xyf[k])))
    out["rates"]["radiance"] = round(rate(lambda k: path.radiance(sg, rays[k], xyf[k], integrator=integ, max_bounce=mb)))
    out["rates"]["rays+radiance"] = round(rate(lambda k: path.radiance(sg, path.camera_rays(sg, p, xyf[k]), xyf[k], integrator=integ,
                                                                       max_bounce=mb)))
    # the yardstick: a render call of the same frame through the one-lane kernel
    if args.yardstick_lib:
        ylib = trace.TraceLib(_abi.declare_trace_abi(C.CDLL(os.path.abspath(args.yardstick_lib)), strict=True))
        out["yardstick_lib"] = os.path.basename(args.yardstick_lib)
    else:
        ylib = hip
        out["yardstick_lib"] = "the product library"
    sy = bs.upload(ylib)
    sy.set_option("megakernel", 1)
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)

    def render(k):
        q = trace.make_params(w, h, eye, cam, integ, mb, spp=1, frame0=k)
        sy.render_device(q, frame.data_ptr(), stream.cuda_stream)

    out["rates"]["yardstick_render_device_megakernel"] = round(rate(render))
    out["radiance_vs_yardstick"] = round(out["rates"]["radiance"] / out["rates"]["yardstick_render_device_megakernel"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
