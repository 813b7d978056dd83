#!/usr/bin/env python3
"""tools/orient_rates.py [--calls K] [--repeats R] [--meshes bunny,bunny_rev,strip,torus] [--no-host] [--table PATH] [--profile-run MESH]
[--kernel-stats DIR]: milliseconds per call of the mesh orientation (include/ezrt_orient.h), beside its yardsticks.

One JSON line, and with --table PATH a text table.  Meshes: `bunny`, the Bunny scene subdivided four times (1 271 808 triangles), as
tools/topology_rates.py makes it; `bunny_rev`, the same with a seeded random 30 % of its triangles reversed; `strip`, a strip of 10^6
triangles with shuffled ids, one open patch of large diameter; `torus`, a 707 x 707 quad grid, 999 698 triangles with shuffled ids,
one closed patch.  The orientation reads no tree.

Per mesh, device events around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times, the median ms per call
and the spread (max - min) / median:
  orient       ezrt_mesh_orient_device alone, outward = 1, on the arrays of a topology made before
  topology     ezrt_mesh_topology_device without the component group (what query.mesh_orient runs first): the yardstick
  rewind       ezrt_rewind_device with the call's flip, on the scene's own rows
  refit        ezrt_scene_refit_device of the same rows (wall clock around the synchronous call: it is what a frame pays next)
`host`: tests/orient_expected.py on the copied triangles and the device topology's arrays, wall-clock seconds, and whether every
array of its answer is the device's.

The library is the one ezrt_amd loads: EZRT_HIP_LIB=build_ab/libezrt_hip_orient_lane_atomics.so (make
build_ab/libezrt_hip_orient_lane_atomics.so) times the volume launch with one atomic per lane instead of one per run.

--profile-run MESH: a topology, then a warm-up and `calls` calls of the orientation and of the rewind, nothing else -- what to run
under a profiler's kernel trace, in a run of its own.  --kernel-stats DIR: the average microseconds of the orientation's kernels from
the *kernel_stats.csv files of such a run, as a JSON line."""
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
OUTS = ("flip", "patch_root", "patch", "proot", "psize", "pflags", "vol6")
KERNELS = ("orient_init", "orient_union", "orient_flatten", "orient_check", "scan_tile_sums", "scan_block", "scan_tiles", "orient_volume", "orient_finish",
           "rewind")


def mesh(name, hip):
    """(tri [n, 36], nodes)"""
    import orient_scenes as OS
    import topology_rates as TR
    import topology_scenes as TS
    from ezrt_amd import build
    if name in ("bunny", "strip"):
        return TR.mesh(name, hip)
    if name == "bunny_rev":
        tri, nodes = TR.mesh("bunny", hip)
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)
        return OS.reverse_rows(tri, OS.some(tri.shape[0], 0.3, OS.SEED + 5)), nodes
    assert name == "torus", name
    V = TS.torus(707, shuffled=False)
    _, nodes, _ = build.build_lbvh(TS.tri36(V), 8)
    return TS.tri36(TS._shuffle(V, TS.SEED + 1)), nodes


def buffers(torch, lib, n, dev):
    mk = lambda dt: torch.empty((n,), dtype=dt, device=dev)
    b = dict(flip=mk(torch.uint8), patch_root=mk(torch.int32), patch=mk(torch.int32), proot=mk(torch.int32), psize=mk(torch.int32),
             pflags=mk(torch.uint8), vol6=mk(torch.int64), summary=torch.zeros((8,), dtype=torch.int64, device=dev))
    wb = int(lib.ezrt_orient_work_bytes(n))
    b["work"] = torch.empty((wb // 8,), dtype=torch.int64, device=dev)
    return b, wb


def call(lib, sg, tb, b, wb, stream, outward=1):
    d = lambda k: P(b[k].data_ptr())
    return lambda: lib.ezrt_mesh_orient_device(sg._h, P(tb["twin"].data_ptr()), P(tb["edge_class"].data_ptr()), outward, d("flip"), d("patch_root"),
                                               d("patch"), d("proot"), d("psize"), d("pflags"), d("vol6"), d("summary"), d("work"), wb,
                                               P(stream.cuda_stream))


def setup(torch, hip, name, dev, stream):
    import topology_rates as TR
    from ezrt_amd import _abi
    lib = _abi._declare(hip.lib, _abi.ORIENT_ABI)
    _abi._declare(lib, _abi.TOPOLOGY_ABI)
    _abi._declare(lib, _abi.REFIT_ABI)
    tri, nodes = mesh(name, hip)
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)
    n = tri.shape[0]
    sg = hip.scene_create(tri, nodes)
    tb, twb = TR.buffers(torch, lib, n, dev)
    topo = TR.call(lib, sg, tb, twb, stream, components=False)
    assert topo() == 0
    b, wb = buffers(torch, lib, n, dev)
    rows = torch.from_numpy(tri).to(dev)
    rewind = lambda: lib.ezrt_rewind_device(sg._h, P(rows.data_ptr()), n, P(b["flip"].data_ptr()), P(stream.cuda_stream))
    return lib, tri, n, sg, tb, topo, b, wb, rows, rewind


def measure(torch, hip, name, dev, stream, a, host):
    import topology_rates as TR
    import weld_rates as WR
    lib, tri, n, sg, tb, topo, b, wb, rows, rewind = setup(torch, hip, name, dev, stream)
    r = {"n_tri": n, "work_mib": round(wb / 2 ** 20, 1)}
    r["orient"] = TR.timed(torch, stream, call(lib, sg, tb, b, wb, stream), a.calls, a.repeats)
    r["summary"] = b["summary"].tolist()
    r["topology"] = TR.timed(torch, stream, topo, a.calls, a.repeats)
    r["rewind"] = TR.timed(torch, stream, rewind, a.calls + (a.calls + 1) % 2, a.repeats)   # an odd number and the warm-up: the rows as they were
    r["refit"] = WR.walled(torch, lambda: lib.ezrt_scene_refit_device(sg._h, P(rows.data_ptr()), n, P(stream.cuda_stream)), a.calls)
    if host:
        import orient_expected as OE
        got = {k: b[k].cpu().numpy() for k in OUTS}
        twin, cls = tb["twin"].cpu().numpy(), tb["edge_class"].cpu().numpy()
        t0 = time.time()
        want = OE.orient(tri, twin, cls, True)
        sec = time.time() - t0
        k = int(want.summary[1])
        equal = all(np.array_equal(got[o][:n if o in OUTS[:3] else k], getattr(want, o)) for o in OUTS) and r["summary"] == want.summary.tolist()
        r["host"] = {"seconds": round(sec, 2), "equal": bool(equal), "device_is_faster_by": round(sec * 1e3 / r["orient"]["ms"], 1)}
    del sg, tb, b, rows
    torch.cuda.empty_cache()
    return r


def kernel_stats(path):
    """{kernel: [launches, average microseconds]} of the orientation's kernels from the profiler's *kernel_stats.csv under path"""
    out = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            for k in KERNELS + ("topo_init", "topo_join", "topo_rank"):
                if name.startswith(k + "_kernel") or ("::" + k + "_kernel") in name or (" " + k + "_kernel") in name:
                    if row.get("AverageNs"):
                        out[k] = [int(float(row.get("Calls", 0) or 0)), round(float(row["AverageNs"]) / 1e3, 1)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--meshes", default="bunny,bunny_rev,strip,torus")
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
        raise SystemExit("tools/orient_rates.py needs a GPU: there is no CPU route to time")
    hip = trace.hip()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    if a.profile_run:
        lib, tri, n, sg, tb, topo, b, wb, rows, rewind = setup(torch, hip, a.profile_run, dev, stream)
        fn = call(lib, sg, tb, b, wb, stream)
        for _ in range(a.calls + 1):
            assert fn() == 0 and rewind() == 0
        torch.cuda.synchronize()
        return
    res = {}
    for name in [m for m in a.meshes.split(",") if m]:
        res[name] = measure(torch, hip, name, dev, stream, a, not a.no_host)
    print(json.dumps({"orient_rates": res, "calls": a.calls, "repeats": a.repeats, "library": os.environ.get("EZRT_HIP_LIB", "libezrt_hip.so")}))
    if a.table:
        cols = ("orient", "topology", "rewind", "refit")
        with open(a.table, "w") as f:
            f.write("# tools/orient_rates.py --calls %d --repeats %d on one MI355X: device events around %d calls, median of %d repeats and their\n"
                    "# spread (max - min) / median.  orient: ezrt_mesh_orient_device alone, outward = 1; topology: ezrt_mesh_topology_device without\n"
                    "# the component group, the same mesh; rewind: ezrt_rewind_device; refit: ezrt_scene_refit_device of the same rows, wall\n"
                    "# clock.  host: tests/orient_expected.py on the copied triangles and the device topology's arrays, wall clock, and whether\n"
                    "# its answer is the device's.\n" % (a.calls, a.repeats, a.calls, a.repeats))
            f.write("%-10s %9s %9s | %s | %s\n" % ("mesh", "n_tri", "work MiB", " | ".join("%9s ms %7s" % (c, "spread") for c in cols), "host s  equal  dev x"))
            for name, r in res.items():
                h = r.get("host")
                f.write("%-10s %9d %9.1f | %s | %s\n" % (name, r["n_tri"], r["work_mib"], " | ".join("%12.4f %7.4f" % (r[c]["ms"], r[c]["spread"]) for c in cols),
                                                        "%6.2f %6s %6.0f" % (h["seconds"], h["equal"], h["device_is_faster_by"]) if h else "not run"))
            for name, r in res.items():
                f.write("%s: summary [taking part, P, orientable, closed, flips, INWARD, S, 0] = %r\n" % (name, r["summary"]))


if __name__ == "__main__":
    main()
