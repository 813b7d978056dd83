#!/usr/bin/env python3
"""tools/topology_rates.py [--calls K] [--repeats R] [--meshes bunny,islands,strip] [--no-host] [--kernel-stats DIR] [--from-json PATH] [--table PATH]:
triangles per second of the mesh topology (include/ezrt_topology.h).

One JSON line, and with --table PATH a text table.  Meshes: `bunny`, the Bunny scene subdivided four times (bunny_scene(subdiv=4),
1 271 808 triangles: the Bunny, its floor and its lamp); `islands`, 10^6 isolated triangles (C == n_tri); `strip`, a strip of 10^6
triangles with shuffled ids (one component whose diameter is the whole mesh: the union-find's worst case here).  The topology reads
no tree: `islands` and `strip` are created under the device builder's tree of the unshuffled triangles.

Timed with device events around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times: the median ms per
call and the spread (max - min) / median of the repeats, for the WHOLE call (every output and the component group) and for the call
without the component group (init, join and rank: twin, edge_class, mult and the summary); `components` is the difference of the two
medians (unite, flatten, scan and scatter).  Mtri/s is the scene's triangles over the median.

The kernels one by one come from a kernel trace, taken in a run of its own (a profiler slows the host): run this tool under the
profiler with --profile-run MESH (a warm-up and `calls` calls of the whole call, nothing else), then pass the directory with the
profiler's *kernel_stats.csv files as --kernel-stats DIR (one sub-directory per mesh): the average time of every topo_* kernel and
of the scan is added.  --from-json PATH takes the timings from an earlier run's JSON line instead of measuring (no GPU needed): the
way to add a kernel trace to the table afterwards.

`host`: the only route without this call -- copy the triangles to the host and build dictionaries (tests/topology_expected.py) --
wall-clock seconds on the same mesh, and whether every array of its answer is the device's."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
P = C.c_void_p
OUTS = ("twin", "edge_class", "mult", "root", "component", "comp_root", "comp_size", "comp_flags", "summary")


def stats(ms):
    med = float(np.median(ms))
    return {"ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)}


def mesh(name, hip):
    """(tri [n, 36], nodes)"""
    import topology_scenes as TS
    from ezrt_amd import build, scenes
    if name == "bunny":
        b = scenes.bunny_scene(subdiv=4)
        return b.tri, b.nodes
    V = TS.islands(10 ** 6) if name == "islands" else TS.strip(10 ** 6, shuffled=False)
    _, nodes, _ = build.build_lbvh(TS.tri36(V), 8)
    if name == "strip":
        V = TS._shuffle(V, TS.SEED + 2)
    return TS.tri36(V), nodes


def buffers(torch, lib, n, dev):
    i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
    u8 = lambda k: torch.empty((k,), dtype=torch.uint8, device=dev)
    b = dict(twin=i32(3 * n), edge_class=u8(3 * n), mult=i32(3 * n), root=i32(n), component=i32(n), comp_root=i32(n), comp_size=i32(n),
             comp_flags=u8(n), summary=torch.zeros((8,), dtype=torch.int64, device=dev))
    wb = int(lib.ezrt_topology_work_bytes(n))
    b["work"] = torch.empty((wb // 8,), dtype=torch.int64, device=dev)
    return b, wb


def call(lib, sg, b, wb, stream, components=True):
    d = lambda k, on=True: P(b[k].data_ptr()) if on else None
    return lambda: lib.ezrt_mesh_topology_device(sg._h, d("twin"), d("edge_class"), d("mult"), d("root", components), d("component", components),
                                                 d("comp_root", components), d("comp_size", components), d("comp_flags", components),
                                                 d("summary"), d("work"), wb, P(stream.cuda_stream))


def timed(torch, stream, fn, calls, repeats):
    assert fn() == 0
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return stats(out)


def kernel_stats(path):
    """{kernel: average microseconds} of the topology's kernels from the profiler's *kernel_stats.csv under path"""
    out = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            for k in ("topo_init", "topo_join", "topo_rank", "topo_unite", "topo_flatten", "topo_scatter", "scan_block"):
                if (k + "_kernel(") in name and row.get("AverageNs"):
                    out[k] = round(float(row["AverageNs"]) / 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--meshes", default="bunny,islands,strip")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--profile-run", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--table", default=None)
    ap.add_argument("--from-json", default=None)
    a = ap.parse_args()
    if a.from_json:
        old = json.loads(open(a.from_json).read().strip().splitlines()[-1])
        a.calls, a.repeats = old["calls"], old["repeats"]
        for name, r in old["topology_rates"].items():
            if a.kernel_stats:
                r["kernels_us"] = kernel_stats(os.path.join(a.kernel_stats, name))
        return report(a, old["topology_rates"])
    import torch
    import topology_expected as TE
    from ezrt_amd import trace
    if not torch.cuda.is_available():
        raise SystemExit("tools/topology_rates.py needs a GPU: there is no CPU route to time")
    hip = trace.hip()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    if a.profile_run:
        tri, nodes = mesh(a.profile_run, hip)
        sg = hip.scene_create(tri, nodes)
        b, wb = buffers(torch, hip.lib, tri.shape[0], dev)
        fn = call(hip.lib, sg, b, wb, stream)
        for _ in range(a.calls + 1):
            assert fn() == 0
        torch.cuda.synchronize()
        return
    res = {}
    for name in a.meshes.split(","):
        tri, nodes = mesh(name, hip)
        n = tri.shape[0]
        sg = hip.scene_create(tri, nodes)
        b, wb = buffers(torch, hip.lib, n, dev)
        r = {"n_tri": n, "work_mib": round(wb / 2 ** 20, 1)}
        r["join_rank"] = timed(torch, stream, call(hip.lib, sg, b, wb, stream, components=False), a.calls, a.repeats)
        r["whole"] = timed(torch, stream, call(hip.lib, sg, b, wb, stream), a.calls, a.repeats)
        r["components_ms"] = round(r["whole"]["ms"] - r["join_rank"]["ms"], 4)
        for k in ("whole", "join_rank"):
            r[k]["mtri_per_s"] = round(n / r[k]["ms"] / 1e3, 1)
        r["summary"] = b["summary"].tolist()
        if a.kernel_stats:
            r["kernels_us"] = kernel_stats(os.path.join(a.kernel_stats, name))
        if not a.no_host:
            got = {k: b[k].cpu().numpy() for k in OUTS}
            t0 = time.time()
            want = TE.topology(np.ascontiguousarray(tri))
            sec = time.time() - t0
            C_ = int(want.summary[6])
            size = {"comp_root": C_, "comp_size": C_, "comp_flags": C_}
            equal = all(np.array_equal(got[k][:size.get(k, got[k].size)], getattr(want, k)) for k in OUTS)
            r["host"] = {"seconds": round(sec, 2), "mtri_per_s": round(n / sec / 1e6, 4), "equal": bool(equal),
                         "device_is_faster_by": round(sec * 1e3 / r["whole"]["ms"], 1)}
        res[name] = r
        del sg, b
        torch.cuda.empty_cache()
    report(a, res)


def report(a, res):
    print(json.dumps({"topology_rates": res, "calls": a.calls, "repeats": a.repeats}))
    if a.table:
        with open(a.table, "w") as f:
            f.write("# tools/topology_rates.py --calls %d --repeats %d: ezrt_mesh_topology_device on one MI355X, device events around %d calls, median of %d\n"
                    "# repeats and their spread (max - min) / median.  whole: every output and the component group; join+rank: without the component\n"
                    "# group (init, join, rank); components: the difference of the two medians.  host: tests/topology_expected.py on the copied\n"
                    "# triangles, wall clock, and whether its answer is the device's.\n" % (a.calls, a.repeats, a.calls, a.repeats))
            f.write("%-8s %9s %9s | %9s %7s %8s | %9s %7s %8s | %10s | %9s %9s %6s %9s\n" % (
                "mesh", "n_tri", "work MiB", "whole ms", "spread", "Mtri/s", "j+r ms", "spread", "Mtri/s", "comp ms", "host s", "Mtri/s", "equal", "dev x"))
            for name, r in res.items():
                h = r.get("host")
                f.write("%-8s %9d %9.1f | %9.4f %7.4f %8.1f | %9.4f %7.4f %8.1f | %10.4f | %s\n" % (
                    name, r["n_tri"], r["work_mib"], r["whole"]["ms"], r["whole"]["spread"], r["whole"]["mtri_per_s"], r["join_rank"]["ms"],
                    r["join_rank"]["spread"], r["join_rank"]["mtri_per_s"], r["components_ms"],
                    "%9.2f %9.4f %6s %9.1f" % (h["seconds"], h["mtri_per_s"], h["equal"], h["device_is_faster_by"]) if h else "not run"))
            for name, r in res.items():
                f.write("%s: summary [live, edges, boundary, manifold, flipped, nonmanifold, components, max m] = %r\n" % (name, r["summary"]))
                if r.get("kernels_us"):
                    ks = r["kernels_us"]
                    f.write("%s: kernel trace, average microseconds per launch: %s\n" % (name, ", ".join("%s %.1f" % kv for kv in ks.items())))
                    parts = {"join": ks.get("topo_join"), "rank": ks.get("topo_rank"),
                             "components": sum(ks.get(k, 0) for k in ("topo_unite", "topo_flatten", "scan_block", "topo_scatter")) or None}
                    f.write("%s: Mtri/s by phase: %s\n" % (name, ", ".join("%s %.0f" % (k, r["n_tri"] / v) for k, v in parts.items() if v)))


if __name__ == "__main__":
    main()
