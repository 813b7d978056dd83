#!/usr/bin/env python3
"""tools/weld_rates.py [--calls K] [--repeats R] [--meshes bunny,strip] [--discs 300,100000] [--no-host] [--table PATH] [--profile-run MESH]:
triangles per second of the vertex weld and the smooth normals (include/ezrt_vertices.h), beside their yardsticks.

One JSON line, and with --table PATH a text table.  Meshes as in tools/topology_rates.py: `bunny`, the Bunny scene subdivided four
times (1 271 808 triangles); `islands`, 10^6 isolated triangles (V == 3 n_tri); `strip`, a strip of 10^6 triangles with shuffled ids.

Per mesh, device events around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times, the median ms per call
and the spread (max - min) / median:
  weld         ezrt_mesh_weld_device, every output           weld_noflags  ... without the flags group (no W4 to W6)
  topology     ezrt_mesh_topology_device, every output: the yardstick for a table-join of this shape, same mesh, same machine
  normals      ezrt_vertex_normals_device on the scene's own rows
  refit        ezrt_scene_refit_device of the same rows (wall clock around the synchronous call: it is what a frame pays next)
`host`: tests/weld_expected.py on the copied triangles -- the dictionaries for the weld, float32 numpy for the normals -- wall-clock
seconds, and whether every array of its answer is the device's (the normals on the bits, a NaN being a NaN).

--profile-run MESH (a mesh name, or disc:K): a warm-up and `calls` calls of the whole weld and of the normals, nothing else -- what to run
under a profiler's kernel trace, in a run of its own, for the kernels one by one.

--discs: the KNOWN LIMIT.  A cone of k triangles round one apex (tests/weld_scenes.py: disc) for every k given: the weld with and
without the flags group, and the normals; a star of valence k costs O(k^2) steps spread over its own k lanes."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
P = C.c_void_p
OUTS = ("vertex", "vert_corner", "star_offsets", "star", "fans", "vert_flags")


def stats(ms):
    med = float(np.median(ms))
    return {"ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)}


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


def walled(torch, fn, calls):
    assert fn() == 0
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def weld_buffers(torch, lib, n, dev):
    i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
    b = dict(vertex=i32(3 * n), vert_corner=i32(3 * n), star_offsets=i32(3 * n + 1), star=i32(3 * n), fans=i32(3 * n),
             vert_flags=torch.empty((3 * n,), dtype=torch.uint8, device=dev), summary=torch.zeros((8,), dtype=torch.int64, device=dev))
    wb = int(lib.ezrt_weld_work_bytes(n))
    b["work"] = torch.empty((wb // 8,), dtype=torch.int64, device=dev)
    return b, wb


def weld_call(lib, sg, b, wb, stream, flags=True):
    d = lambda k, on=True: P(b[k].data_ptr()) if on else None
    return lambda: lib.ezrt_mesh_weld_device(sg._h, d("vertex"), d("vert_corner"), d("star_offsets"), d("star"), d("fans", flags),
                                             d("vert_flags", flags), d("summary"), d("work"), wb, P(stream.cuda_stream))


def normals_call(torch, lib, sg, rows, b, n, dev, stream):
    nb = int(lib.ezrt_vertex_normals_work_bytes(n))
    work = torch.empty((nb // 8,), dtype=torch.int64, device=dev)
    return lambda: lib.ezrt_vertex_normals_device(sg._h, P(rows.data_ptr()), n, P(b["vertex"].data_ptr()), P(b["star_offsets"].data_ptr()),
                                                  P(b["star"].data_ptr()), P(work.data_ptr()), nb, P(stream.cuda_stream)), work


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def measure(torch, hip, tri, nodes, dev, stream, a, host, topology=True):
    import topology_rates as TR
    import weld_expected as WE
    from ezrt_amd import _abi
    lib = _abi._declare(hip.lib, _abi.WELD_ABI)
    _abi._declare(lib, _abi.REFIT_ABI)
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)
    n = tri.shape[0]
    sg = hip.scene_create(tri, nodes)
    b, wb = weld_buffers(torch, lib, n, dev)
    r = {"n_tri": n, "work_mib": round(wb / 2 ** 20, 1)}
    r["weld_noflags"] = timed(torch, stream, weld_call(lib, sg, b, wb, stream, flags=False), a.calls, a.repeats)
    r["weld"] = timed(torch, stream, weld_call(lib, sg, b, wb, stream), a.calls, a.repeats)
    r["summary"] = b["summary"].tolist()
    if topology:
        tb, twb = TR.buffers(torch, lib, n, dev)
        r["topology"] = timed(torch, stream, TR.call(lib, sg, tb, twb, stream), a.calls, a.repeats)
        del tb
    rows = torch.from_numpy(tri).to(dev)
    fn, work = normals_call(torch, lib, sg, rows, b, n, dev, stream)
    r["normals"] = timed(torch, stream, fn, a.calls, a.repeats)
    r["refit"] = walled(torch, lambda: lib.ezrt_scene_refit_device(sg._h, P(rows.data_ptr()), n, P(stream.cuda_stream)), a.calls)
    for k in ("weld", "weld_noflags", "topology", "normals", "refit"):
        if k in r:
            r[k]["mtri_per_s"] = round(n / r[k]["ms"] / 1e3, 1)
    if host:
        got = {k: b[k].cpu().numpy() for k in OUTS}
        got_n = rows.cpu().numpy()[:, 9:18]
        t0 = time.time()
        want = WE.weld(tri)
        sec = time.time() - t0
        L, V = int(want.summary[0]), int(want.summary[1])
        size = {"vertex": 3 * n, "star": L, "star_offsets": V + 1}
        equal = all(np.array_equal(got[k][:size.get(k, V)], getattr(want, k)) for k in OUTS) and r["summary"] == want.summary.tolist()
        t0 = time.time()
        want_n = WE.normals(tri, want.vertex, want.star_offsets, want.star)
        sec_n = time.time() - t0
        r["host"] = {"weld_seconds": round(sec, 2), "weld_equal": bool(equal), "weld_device_is_faster_by": round(sec * 1e3 / r["weld"]["ms"], 1),
                     "normals_seconds": round(sec_n, 3), "normals_equal": same_bits(got_n, want_n),
                     "normals_device_is_faster_by": round(sec_n * 1e3 / r["normals"]["ms"], 1)}
    del sg, b, rows, work
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--meshes", default="bunny,strip")
    ap.add_argument("--discs", default="300,100000")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--table", default=None)
    ap.add_argument("--profile-run", default=None)
    a = ap.parse_args()
    import torch
    import topology_rates as TR
    import weld_scenes as WS
    from ezrt_amd import trace
    if not torch.cuda.is_available():
        raise SystemExit("tools/weld_rates.py needs a GPU: there is no CPU route to time")
    hip = trace.hip()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    if a.profile_run:
        import topology_scenes as TS
        from ezrt_amd import _abi, build
        if a.profile_run.startswith("disc:"):
            k = int(a.profile_run[5:])
            tri, nodes = TS.tri36(WS.disc(k)), build.build_lbvh(TS.tri36(TS.islands(k)), 8)[1]
        else:
            tri, nodes = TR.mesh(a.profile_run, hip)
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)
        lib = _abi._declare(hip.lib, _abi.WELD_ABI)
        sg = hip.scene_create(tri, nodes)
        b, wb = weld_buffers(torch, lib, tri.shape[0], dev)
        rows = torch.from_numpy(tri).to(dev)
        fn, gn = weld_call(lib, sg, b, wb, stream), normals_call(torch, lib, sg, rows, b, tri.shape[0], dev, stream)
        for _ in range(a.calls + 1):
            assert fn() == 0 and gn[0]() == 0
        torch.cuda.synchronize()
        return
    res, discs = {}, {}
    for name in [m for m in a.meshes.split(",") if m]:
        tri, nodes = TR.mesh(name, hip)
        res[name] = measure(torch, hip, tri, nodes, dev, stream, a, not a.no_host)
    for k in [int(x) for x in a.discs.split(",") if x]:
        import topology_scenes as TS
        from ezrt_amd import build
        _, nodes, _ = build.build_lbvh(TS.tri36(TS.islands(k)), 8)             # a tree that neither call reads
        discs[str(k)] = measure(torch, hip, TS.tri36(WS.disc(k)), nodes, dev, stream, a, not a.no_host, topology=False)
    print(json.dumps({"weld_rates": res, "discs": discs, "calls": a.calls, "repeats": a.repeats}))
    if a.table:
        with open(a.table, "w") as f:
            f.write("# tools/weld_rates.py --calls %d --repeats %d on one MI355X: device events around %d calls, median of %d repeats and their\n"
                    "# spread (max - min) / median.  weld: ezrt_mesh_weld_device, every output; no flags: without fans and vert_flags; topology:\n"
                    "# ezrt_mesh_topology_device, every output, the same mesh; normals: ezrt_vertex_normals_device; refit: ezrt_scene_refit_device\n"
                    "# of the same rows, wall clock.  host: tests/weld_expected.py on the copied triangles, wall clock, and whether its answer\n"
                    "# is the device's (the normals on the bits).\n" % (a.calls, a.repeats, a.calls, a.repeats))
            cols = ("weld", "weld_noflags", "topology", "normals", "refit")
            f.write("%-12s %9s %9s | %s | %s\n" % ("mesh", "n_tri", "work MiB", " | ".join("%12s ms %7s" % (c, "spread") for c in cols),
                                                 "host weld s  equal  dev x | host normals s  equal  dev x"))
            for name, r in list(res.items()) + [("disc " + k, v) for k, v in discs.items()]:
                h = r.get("host")
                f.write("%-12s %9d %9.1f | %s | %s\n" % (
                    name, r["n_tri"], r["work_mib"],
                    " | ".join("%15.4f %7.4f" % (r[c]["ms"], r[c]["spread"]) if c in r else "%15s %7s" % ("-", "-") for c in cols),
                    "%11.2f %6s %6.0f | %14.3f %6s %6.0f" % (h["weld_seconds"], h["weld_equal"], h["weld_device_is_faster_by"], h["normals_seconds"],
                                                            h["normals_equal"], h["normals_device_is_faster_by"]) if h else "not run"))
            for name, r in list(res.items()) + [("disc " + k, v) for k, v in discs.items()]:
                f.write("%s: summary [L, V, largest valence, border, edge of >= 3, pinched, 0, 0] = %r; Mtri/s: %s\n" % (
                    name, r["summary"], ", ".join("%s %.1f" % (c, r[c]["mtri_per_s"]) for c in cols if c in r)))


if __name__ == "__main__":
    main()
