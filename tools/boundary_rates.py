#!/usr/bin/env python3
"""tools/boundary_rates.py [--calls K] [--repeats R] [--meshes bunny,strip,islands] [--no-host] [--table PATH] [--profile-run MESH]
[--kernel-stats DIR]: milliseconds per call of the boundary loops and of the cap (include/ezrt_boundary.h), beside their yardstick.

One JSON line, and with --table PATH a text table.  Meshes: `bunny`, the Bunny scene subdivided four times (1 271 808 triangles, few
boundary edges), as tools/topology_rates.py makes it; `strip`, a strip of 10^6 triangles with shuffled ids, one loop of 10^6 + 2
half-edges, the ranking's worst case; `islands`, 333 333 separate triangles, every half-edge on a boundary, 333 333 loops.  The calls
read no tree.

Per mesh, device events around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times, the median ms per call
and the spread (max - min) / median:
  boundary     ezrt_mesh_boundary_device alone, with the area group, on the arrays of a topology made before
  no_area      the same without the area group
  topology     ezrt_mesh_topology_device without the component group (what query.mesh_boundary runs first): the yardstick
  cap          ezrt_cap_rows_device on the call's arrays and the scene's own rows
`host`: tests/boundary_expected.py on the copied triangles and the device topology's arrays, wall-clock seconds, and whether every
array of its answer, the cap's included, is the device's.

--profile-run MESH: a topology, then a warm-up and `calls` calls of the loops call and of the cap, nothing else -- what to run under a
profiler's kernel trace, in a run of its own.  --kernel-stats DIR: the launches and average microseconds of the calls' kernels from the
*kernel_stats.csv files of such a run, or from its *_results.db, as a JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
P = C.c_void_p
KERNELS = ("bd_init", "bd_next", "bd_union", "bd_open", "bd_rank_init", "bd_jump", "bd_flag", "bd_number", "bd_scatter", "cap_rows", "scan_tile_sums",
           "scan_block", "scan_tiles", "topo_init", "topo_join", "topo_rank")


def mesh(name, hip):
    """(tri [n, 36], nodes)"""
    import topology_rates as TR
    import topology_scenes as TS
    from ezrt_amd import build
    if name in ("bunny", "strip"):
        return TR.mesh(name, hip)
    assert name == "islands", name
    V = TS.islands(333333)
    _, nodes, _ = build.build_lbvh(TS.tri36(V), 8)
    return TS.tri36(V), nodes


def buffers(torch, lib, n, dev):
    H = 3 * n
    i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
    b = dict(next=i32(H), loop=i32(H), pos=i32(H), order=i32(H), loop_offsets=i32(H + 1), lflags=torch.empty((H,), dtype=torch.uint8, device=dev),
             area2=torch.empty((3 * H,), dtype=torch.int64, device=dev), summary=torch.zeros((8,), dtype=torch.int64, device=dev),
             cap=torch.empty((H, 36), dtype=torch.float32, device=dev), cap_valid=torch.zeros((H,), dtype=torch.uint8, device=dev))
    wb = int(lib.ezrt_boundary_work_bytes(n))
    b["work"] = torch.empty((wb // 8,), dtype=torch.int64, device=dev)
    return b, wb


def call(lib, sg, tb, b, wb, stream, area=True):
    d = lambda k: P(b[k].data_ptr())
    return lambda: lib.ezrt_mesh_boundary_device(sg._h, P(tb["twin"].data_ptr()), P(tb["edge_class"].data_ptr()), d("next"), d("loop"), d("pos"),
                                                 d("order"), d("loop_offsets"), d("lflags"), d("area2") if area else None, d("summary"), d("work"), wb,
                                                 P(stream.cuda_stream))


def setup(torch, hip, name, dev, stream):
    import topology_rates as TR
    from ezrt_amd import _abi
    lib = _abi._declare(hip.lib, _abi.BOUNDARY_ABI)
    _abi._declare(lib, _abi.TOPOLOGY_ABI)
    tri, nodes = mesh(name, hip)
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)
    n = tri.shape[0]
    sg = hip.scene_create(tri, nodes)
    tb, twb = TR.buffers(torch, lib, n, dev)
    topo = TR.call(lib, sg, tb, twb, stream, components=False)
    assert topo() == 0
    b, wb = buffers(torch, lib, n, dev)
    rows = torch.from_numpy(tri).to(dev)
    d = lambda k: P(b[k].data_ptr())
    cap = lambda: lib.ezrt_cap_rows_device(sg._h, P(rows.data_ptr()), n, d("order"), d("loop"), d("pos"), d("loop_offsets"), d("lflags"), d("summary"),
                                           d("cap"), d("cap_valid"), P(stream.cuda_stream))
    return lib, tri, n, sg, tb, topo, b, wb, rows, cap


def measure(torch, hip, name, dev, stream, a, host):
    import topology_rates as TR
    lib, tri, n, sg, tb, topo, b, wb, rows, cap = setup(torch, hip, name, dev, stream)
    r = {"n_tri": n, "work_mib": round(wb / 2 ** 20, 1)}
    r["no_area"] = TR.timed(torch, stream, call(lib, sg, tb, b, wb, stream, area=False), a.calls, a.repeats)
    r["boundary"] = TR.timed(torch, stream, call(lib, sg, tb, b, wb, stream), a.calls, a.repeats)
    r["summary"] = b["summary"].tolist()
    r["topology"] = TR.timed(torch, stream, topo, a.calls, a.repeats)
    r["cap"] = TR.timed(torch, stream, cap, a.calls, a.repeats)
    if host:
        import boundary_expected as BE
        B, L = r["summary"][0], r["summary"][1]
        size = {"next": 3 * n, "loop": 3 * n, "pos": 3 * n, "order": B, "loop_offsets": L + 1, "lflags": L, "area2": 3 * L}
        got = {k: b[k][:s].cpu().numpy() for k, s in size.items()}
        got_cap, got_valid = b["cap"][:B].cpu().numpy(), b["cap_valid"][:B].cpu().numpy()
        twin, cls = tb["twin"].cpu().numpy(), tb["edge_class"].cpu().numpy()
        t0 = time.time()
        want = BE.boundary(tri, twin, cls)
        sec = time.time() - t0
        equal = all(np.array_equal(got[k], getattr(want, k).reshape(-1)) for k in size) and r["summary"] == want.summary.tolist()
        wc, wv = BE.cap(tri, want)
        same = (got_cap.view(np.uint32) == wc.view(np.uint32)) | (np.isnan(got_cap) & np.isnan(wc))   # a NaN is a NaN
        r["host"] = {"seconds": round(sec, 2), "equal": bool(equal), "cap_equal": bool(same.all() and np.array_equal(got_valid, wv)),
                     "n_cap": int(wv.sum()), "device_is_faster_by": round(sec * 1e3 / r["boundary"]["ms"], 1)}
    del sg, tb, b, rows
    torch.cuda.empty_cache()
    return r


def kernel_stats(path):
    """{kernel: [launches, average microseconds]} of the calls' kernels from the profiler's *kernel_stats.csv under path, or, where the
    profiler wrote its database instead (no --output-format csv), from the `kernels` view of the *_results.db files"""
    out = {}
    for f in glob.glob(os.path.join(path, "**", "*_results.db"), recursive=True):
        import sqlite3
        for name, calls, avg in sqlite3.connect(f).execute("select name, count(*), avg(end - start) from kernels group by name"):
            short = ((name or "").split("(")[0].split("::")[-1].split() or [""])[-1]
            if short.endswith("_kernel") and short[:-7] in KERNELS:
                out[short[:-7]] = [int(calls), round(avg / 1e3, 1)]
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            for k in KERNELS:
                if name.startswith(k + "_kernel") or ("::" + k + "_kernel") in name or (" " + k + "_kernel") in name:
                    if row.get("AverageNs"):
                        out[k] = [int(float(row.get("Calls", 0) or 0)), round(float(row["AverageNs"]) / 1e3, 1)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--meshes", default="bunny,strip,islands")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--table", default=None)
    ap.add_argument("--profile-run", default=None)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps({"kernel_stats_us": kernel_stats(a.kernel_stats)}))
        return
    import torch
    from ezrt_amd import trace
    if not torch.cuda.is_available():
        raise SystemExit("tools/boundary_rates.py needs a GPU: there is no CPU route to time")
    hip = trace.hip()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    if a.profile_run:
        lib, tri, n, sg, tb, topo, b, wb, rows, cap = setup(torch, hip, a.profile_run, dev, stream)
        fn = call(lib, sg, tb, b, wb, stream)
        for _ in range(a.calls + 1):
            assert fn() == 0 and cap() == 0
        torch.cuda.synchronize()
        return
    res = {}
    for name in [m for m in a.meshes.split(",") if m]:
        res[name] = measure(torch, hip, name, dev, stream, a, not a.no_host)
    print(json.dumps({"boundary_rates": res, "calls": a.calls, "repeats": a.repeats}))
    if a.table:
        cols = ("boundary", "no_area", "topology", "cap")
        with open(a.table, "w") as f:
            f.write("# tools/boundary_rates.py --calls %d --repeats %d on one MI355X: device events around %d calls, median of %d repeats and their\n"
                    "# spread (max - min) / median.  boundary: ezrt_mesh_boundary_device alone, with the area group; no_area: without it; topology:\n"
                    "# ezrt_mesh_topology_device without the component group, the same mesh; cap: ezrt_cap_rows_device.  host:\n"
                    "# tests/boundary_expected.py on the copied triangles and the device topology's arrays, wall clock, and whether its answer and\n"
                    "# its cap are the device's.\n" % (a.calls, a.repeats, a.calls, a.repeats))
            f.write("%-8s %9s %9s | %s | %s\n" % ("mesh", "n_tri", "work MiB", " | ".join("%9s ms %7s" % (c, "spread") for c in cols),
                                                  "host s  equal  cap eq  dev x"))
            for name, r in res.items():
                h = r.get("host")
                f.write("%-8s %9d %9.1f | %s | %s\n" % (name, r["n_tri"], r["work_mib"], " | ".join("%12.4f %7.4f" % (r[c]["ms"], r[c]["spread"]) for c in cols),
                                                      "%6.2f %6s %7s %6.0f" % (h["seconds"], h["equal"], h["cap_equal"], h["device_is_faster_by"]) if h else "not run"))
            for name, r in res.items():
                f.write("%s: summary [B, L, closed, longest, dead ends, S2, 0, 0] = %r\n" % (name, r["summary"]))


if __name__ == "__main__":
    main()
