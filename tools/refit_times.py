#!/usr/bin/env python3
"""tools/refit_times.py [--refits K]: what a device refit (include/ezrt_refit.h) costs against re-creating the scene.

One JSON line.  Per scene (C2: bench.py's bunny_scene(subdiv=2); C5: mega_scene(), 10^6 triangles), on the scene's arrays rotated
rigidly about the vertical axis:
  refit_first_ms      the first ezrt_scene_refit_device of the scene (uploads the kept topology, sizes the scratch)
  refit_ms            median and min over K later refits (wall clock around the synchronous call; the triangles already on the device)
  create_ms           ezrt_scene_create of the refitted arrays (tri', refit_nodes(tri', nodes)), wall clock, best of 3
  sah_build_ms        ezrt_build_sah of tri' (a new tree for the new positions: wall clock, and the builder's own device time)
  rebuild_ms          sah_build + ezrt_scene_create of its arrays: what a caller without a refit pays per change of geometry
Then one C2 frame (512 x 512, 64 spp, integrator 50, bench.py's camera) after a rigid rotation by 45 degrees: the refitted scene
(the tree built for the old positions) against a scene built and created from scratch for the rotated triangles -- what the kept
topology costs per frame when geometry moves a lot.  Frame times: ezrt_last_render_ms after one warm-up call, best of 3."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rotate(tri, deg, about):
    t = tri.copy()
    th = np.deg2rad(deg)
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    c = np.asarray(about, np.float64)
    P = t[:, :9].reshape(-1, 3, 3).astype(np.float64)
    t[:, :9] = ((P - c) @ R.T + c).reshape(-1, 9).astype(np.float32)
    N = t[:, 9:18].reshape(-1, 3, 3).astype(np.float64)
    t[:, 9:18] = (N @ R.T).reshape(-1, 9).astype(np.float32)
    return t


def wall(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
        del r
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refits", type=int, default=20)
    args = ap.parse_args()
    import torch
    from ezrt_amd import build, refit, scene as S, scenes, trace
    from ezrt_amd.srchash import gpu_source_hash
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    out = {"tool": "refit_times", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "scenes": {}}
    c2 = None
    for name, bs in (("C2", scenes.bunny_scene(subdiv=2, hdr="shipped")), ("C5", scenes.mega_scene())):
        if name == "C2":
            c2 = bs
        P = bs.tri[:, :9].reshape(-1, 3)
        centre = 0.5 * (P.min(0) + P.max(0))
        tri2 = rotate(bs.tri, 30.0, centre)
        nodes2 = refit.refit_nodes(tri2, bs.nodes)
        sg = hip.scene_create(bs.tri, bs.nodes)
        g2, g1 = torch.from_numpy(tri2).to(dev), torch.from_numpy(bs.tri).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        refit.refit(sg, g2)
        first = (time.perf_counter() - t0) * 1e3
        times = []
        for k in range(args.refits):
            g = g1 if k % 2 == 0 else g2
            t0 = time.perf_counter()
            refit.refit(sg, g)
            times.append((time.perf_counter() - t0) * 1e3)
        create = wall(lambda: hip.scene_create(tri2, nodes2), 3)
        raw = tri2.copy()
        dev_ms = []

        def sah():
            t, n, ms = build.build_sah(raw, 8)
            dev_ms.append(ms)
            return t, n
        sah_wall = wall(sah, 3)
        bt, bn = build.build_sah(raw, 8)[:2]
        rebuild = wall(lambda: (build.build_sah(raw, 8), hip.scene_create(bt, bn)), 3)
        out["scenes"][name] = {
            "n_tri": int(bs.tri.shape[0]), "n_nodes": int(bs.nodes.shape[0]),
            "refit_first_ms": round(first, 3), "refit_ms_median": round(statistics.median(times), 3),
            "refit_ms_min": round(min(times), 3), "create_ms": round(create, 2), "sah_build_ms": round(sah_wall, 2),
            "sah_build_device_ms": round(min(dev_ms), 2), "rebuild_ms": round(rebuild, 2),
            "create_over_refit": round(create / statistics.median(times), 1),
            "rebuild_over_refit": round(rebuild / statistics.median(times), 1)}
        del sg
    # one C2 frame after a 45-degree rotation: refitted (old tree) vs built from scratch for the new positions
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    P = c2.tri[:, :9].reshape(-1, 3)
    tri2 = rotate(c2.tri, 45.0, 0.5 * (P.min(0) + P.max(0)))
    bt, bn = build.build_sah(tri2.copy(), 8)[:2]
    p = trace.make_params(cfg["width"], cfg["height"], eye, cam, cfg["integrator"], cfg["max_bounce"], spp=cfg["spp"])
    frames = {}
    for label, make in (("refitted", lambda: c2.upload(hip)), ("fresh_sah", lambda: hip.scene_create(bt, bn))):
        s = make()
        if c2.hdr is not None and label == "fresh_sah":
            s.set_env(c2.hdr, c2.cache, c2.env_filter)
        if label == "refitted":
            refit.refit(s, torch.from_numpy(tri2).to(dev))
        fr = hip.frame(cfg["width"], cfg["height"])
        s.render_device(p, fr.ptr)
        torch.cuda.synchronize()
        best = None
        for _ in range(3):
            s.render_device(p, fr.ptr)
            torch.cuda.synchronize()
            ms = s.last_render_ms()[0]
            best = ms if best is None else min(best, ms)
        frames[label] = {"frame_ms": round(best, 3), "prune": s.prune_info()}
        del s, fr
    frames["refitted_over_fresh"] = round(frames["refitted"]["frame_ms"] / frames["fresh_sah"]["frame_ms"], 3)
    out["c2_frame_after_45deg_rotation"] = frames
    print(json.dumps(out))


if __name__ == "__main__":
    main()
