#!/usr/bin/env python3
"""tools/self_overlap_rates.py [--calls K]: triangles per second of the self-overlap query (include/ezrt_self_overlap.h) over ALL
triangles of the benchmark scenes, beside the route a caller had before it.

One JSON line.  Scenes: the Bunny scene at two sizes (bunny_scene(subdiv=0) and the benchmark's bunny_scene(subdiv=2)).  For max_k =
0 (count only), 8 and 64 (with the count):
  walk     query.self_overlap(scene, None, max_k): self_overlap_kernel<true>, every triangle of the scene as a query
  sweep    self_overlap_kernel<false> on the same arrays created with one leaf given a second parent, so that the scene does not
           prune; the first 8192 triangles only
and `old`, the route without this query: query.tri_overlap of the scene's own triangles (their nine floats, already on the device)
with max_k = 64, then the filter on ids in torch -- the own id dropped from every row.  That route's kernel is tri_overlap_kernel,
which this query leaves as it was (profiles/r18/self_overlap_regs.txt), so the figure is the parent's.  It is NOT the same answer:
its rows hold the vertex neighbours, which fill them before a crossing is seen (mean_old_row is what is left after the filter;
mean_crossings is the true number).  Each is timed with hipEvents around `calls` back-to-back calls on one stream after a warm-up
call; the rate is Mtriangles/s.  The two routes' answers are compared on the sweep's triangles (they must be equal); nothing else is
checked here (tests/test_gpu_self_overlap.py)."""
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
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    from ezrt_amd import query, scenes, trace
    from ezrt_amd.srchash import gpu_source_hash
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    stream = torch.cuda.current_stream(dev)

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

    out = {"tool": "self_overlap_rates", "srchash": gpu_source_hash(), "device": torch.cuda.get_device_name(dev), "calls": args.calls,
           "unit": "Mtriangles/s", "scenes": {}}
    few = max(1, args.calls // 5)
    for subdiv in (0, 2):
        sc = scenes.bunny_scene(subdiv=subdiv, hdr="shipped")
        tri, nodes = sc.tri, sc.nodes
        m = int(tri.shape[0])
        walk, swept = hip.scene_create(tri, nodes), hip.scene_create(tri, second_parent(nodes))
        assert walk.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
        n_sweep = min(m, 1 << 13)
        first = torch.arange(n_sweep, dtype=torch.int32, device=dev)
        own9 = torch.from_numpy(np.ascontiguousarray(tri[:, :9], np.float32)).to(dev)
        me = torch.arange(m, dtype=torch.int32, device=dev)[:, None]

        def old():
            r = query.tri_overlap(walk, own9, 64, count=True)
            keep = r.tri != me                                        # the filter on ids: all a caller without topology can drop
            return torch.where(keep, r.tri, -1), r.n_overlap - 1

        a, b = query.self_overlap(walk, first, 64, count=True), query.self_overlap(swept, first, 64, count=True)
        full = query.self_overlap(walk, None, 0, count=True)
        rows, left = old()
        torch.cuda.synchronize()
        res = {"triangles": m, "tris_sweep": n_sweep,
               "routes_equal": bool(torch.equal(a.tri, b.tri) and torch.equal(a.n_overlap, b.n_overlap)),
               "mean_crossings": round(float(full.n_overlap.float().mean().item()), 3),
               "mean_old_row": round(float(left.float().mean().item()), 2),
               "old": rate(old, m, args.calls)}
        for k in (0, 8, 64):
            res["max_k_%d" % k] = {"walk": rate(lambda: query.self_overlap(walk, None, k, count=True), m, args.calls),
                                   "sweep": rate(lambda: query.self_overlap(swept, first, k, count=True), n_sweep, few)}
        out["scenes"]["bunny_subdiv%d" % subdiv] = res
        walk.close()
        swept.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
