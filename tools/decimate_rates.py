#!/usr/bin/env python3
"""tools/decimate_rates.py [--calls K] [--repeats R] [--cases strip_coarse,strip_fine,bunny] [--no-host] [--table PATH]: milliseconds per
call of the decimation (include/ezrt_decimate.h), count and fill apart, beside the fill's yardstick and beside the topology and the weld
of the same rows.

One JSON line, and with --table PATH a text table.  Cases: `strip_coarse`, a strip of 10^6 triangles with shuffled ids under a grid of
cells of 16 x 16 x 16 -- about 100 corners per cell; `strip_fine`, the same strip under a grid of cells of 0.75 -- one vertex per
cell, the fullest table; `strip_ordered`, the coarse grid on the strip in its natural order, where neighbouring lanes share cells (the
runs of the insert); `bunny`, the rows of the Bunny scene subdivided four times (1 272 140 triangles) under a grid of 1 / 256 of its
largest extent.

Per case, device events around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times, the median ms per call
and the spread (max - min) / median; the entries take turns inside every repeat:
  count        ezrt_decimate_count_device with EZRT_DECIMATE_DEDUP: init, insert, flag, scan, cells, classify, keep, scan
  count_all    the same call without the flag: no classify launch
  fill         ezrt_decimate_rows_device on 16-byte aligned rows: the staged fill (the per-lane fill where EZRT_HIP_LIB names the library
               built with -DEZRT_DECIMATE_PER_LANE=1: `make build_ab/libezrt_hip_decimate_per_lane.so`)
  copy         the yardstick: torch's device-to-device copy_ of half the bytes the fill reads plus writes -- 20 per input row (cell,
               offsets) and 264 per output row (three points, the material, the row, src) -- which reads and writes that many
  fill_4       the fill on tri36 and out moved by 4 bytes: the per-lane route in the product library
  topology     ezrt_mesh_topology_device without the component group, on a scene of the rows
  weld         ezrt_mesh_weld_device with the flags group, on the same scene
`host`: tests/decimate_expected.py on the same rows, wall-clock seconds, whether every array of the count and the rows of the fill are
the device's, and whether the two routes of the fill gave the same bits."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
P = C.c_void_p
F = np.float32
CASES = {"strip_coarse": ("strip", [-0.5, -0.5, -0.5, 16.0]), "strip_fine": ("strip", [-0.25, -0.25, -0.25, 0.75]),
         "strip_ordered": ("strip_ordered", [-0.5, -0.5, -0.5, 16.0]), "bunny": ("bunny", None)}
_mesh = {}


def mesh(name, hip):
    import topology_rates as TR
    import topology_scenes as TS
    if name not in _mesh:
        _mesh.clear()                                                          # one mesh at a time: they are large
        if name == "strip_ordered":
            tri, nodes = TR.mesh("strip", hip)
            _mesh[name] = (TS.tri36(TS.strip(10 ** 6, shuffled=False)), nodes)  # (the tree is only there for the scene: nothing reads it)
        else:
            _mesh[name] = TR.mesh(name, hip)
    return _mesh[name]


def measure(torch, hip, case, dev, stream, a, host):
    import clip_rates as CR
    import decimate_expected as DE
    import topology_rates as TR
    from ezrt_amd import _abi
    lib = _abi._declare(hip.lib, _abi.DECIMATE_ABI)
    _abi._declare(hip.lib, _abi.WELD_ABI)
    name, grid = CASES[case]
    tri, nodes = mesh(name, hip)
    R = np.ascontiguousarray(tri, F).reshape(-1, 36)
    n = R.shape[0]
    grid = DE.grid_of(R, 256) if grid is None else F(grid)
    sg = hip.scene_create(R, nodes)
    h = P(stream.cuda_stream)
    d = lambda x: P(x.data_ptr())
    r = {"n_rows": n, "grid": [float(x) for x in grid], "library": os.environ.get("EZRT_HIP_LIB", "product")}
    tb, twb = TR.buffers(torch, lib, n, dev)
    r["topology"] = TR.timed(torch, stream, TR.call(lib, sg, tb, twb, stream, components=False), a.calls, a.repeats)
    del tb
    i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
    wbuf = dict(vertex=i32(3 * n), vert_corner=i32(3 * n), star_offsets=i32(3 * n + 1), star=i32(3 * n), fans=i32(3 * n),
                vert_flags=torch.empty((3 * n,), dtype=torch.uint8, device=dev), summary=torch.zeros((8,), dtype=torch.int64, device=dev))
    wwb = int(lib.ezrt_weld_work_bytes(n))
    wwork = torch.empty((wwb // 8,), dtype=torch.int64, device=dev)
    weld = lambda: lib.ezrt_mesh_weld_device(sg._h, d(wbuf["vertex"]), d(wbuf["vert_corner"]), d(wbuf["star_offsets"]), d(wbuf["star"]),
                                             d(wbuf["fans"]), d(wbuf["vert_flags"]), d(wbuf["summary"]), d(wwork), wwb, h)
    r["weld"] = TR.timed(torch, stream, weld, a.calls, a.repeats)
    del wbuf, wwork
    torch.cuda.empty_cache()
    flat = torch.empty((n * 36 + 4,), dtype=torch.float32, device=dev)         # the rows, and the same rows 4 bytes on
    flat4 = torch.empty((n * 36 + 4,), dtype=torch.float32, device=dev)
    flat[:n * 36] = torch.from_numpy(R).to(dev).reshape(-1)
    flat4[1:n * 36 + 1] = flat[:n * 36]
    d_grid = torch.from_numpy(grid).to(dev)
    cell, corner = i32(3 * n), i32(3 * n)
    point = torch.empty((3 * n, 3), dtype=torch.float32, device=dev)
    offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    summary = torch.zeros((8,), dtype=torch.int64, device=dev)
    wb = int(lib.ezrt_decimate_work_bytes(n))
    work = torch.empty((wb // 8,), dtype=torch.int64, device=dev)
    r["work_mb"] = round(wb / 1e6, 1)
    count = lambda flags: lambda: lib.ezrt_decimate_count_device(sg._h, d(flat), n, d(d_grid), flags, d(cell), d(corner), d(point), d(offsets),
                                                                 d(summary), d(work), wb, h)
    assert count(1)() == 0, lib.ezrt_last_error()
    torch.cuda.synchronize()
    T = int(offsets[n].item())
    r["summary"] = summary.tolist()
    out = torch.empty((T * 36 + 4,), dtype=torch.float32, device=dev)
    src = i32(max(T, 1))
    fill = lambda rows, shift: lambda: lib.ezrt_decimate_rows_device(sg._h, P(rows.data_ptr() + shift), n, d(cell), d(point), d(offsets), T,
                                                                     P(out.data_ptr() + shift) if T else None, d(src) if T else None, h)
    moved = 20 * n + 264 * T
    r["moved_mb"] = round(moved / 1e6, 1)
    a_buf = torch.empty((max(moved // 2, 1),), dtype=torch.uint8, device=dev)
    b_buf = torch.empty((max(moved // 2, 1),), dtype=torch.uint8, device=dev)
    fns = {"count": count(1), "count_all": count(0), "fill": fill(flat, 0), "copy": lambda: b_buf.copy_(a_buf), "fill_4": fill(flat4, 4)}
    for k in ("count", "count_all", "fill", "fill_4"):
        assert fns[k]() == 0, lib.ezrt_last_error()
    assert count(1)() == 0                                                     # (the arrays of the DEDUP count are what the fills read)
    del fns["count_all"]
    r.update(CR.timed_in_turn(torch, stream, fns, a.calls, a.repeats))
    r["count_all"] = TR.timed(torch, stream, count(0), a.calls, a.repeats)
    assert count(1)() == 0
    r["fill_over_copy"] = round(r["fill"]["ms"] / r["copy"]["ms"], 3)
    r["fill_4_over_fill"] = round(r["fill_4"]["ms"] / r["fill"]["ms"], 3)
    r["count_over_weld"] = round(r["count"]["ms"] / r["weld"]["ms"], 3)
    r["count_over_topology"] = round(r["count"]["ms"] / r["topology"]["ms"], 3)
    if host:
        assert fill(flat, 0)() == 0
        torch.cuda.synchronize()
        got = out[:T * 36].cpu().numpy().reshape(-1, 36)
        assert fill(flat4, 4)() == 0
        torch.cuda.synchronize()
        routes = DE.same_rows(out[1:T * 36 + 1].cpu().numpy().reshape(-1, 36), got)
        t0 = time.time()
        want = DE.decimate(R, grid, 1)
        sec = time.time() - t0
        nc = int(want.summary[4])
        equal = (summary.tolist() == want.summary.tolist() and np.array_equal(cell.cpu().numpy(), want.cell)
                 and np.array_equal(corner[:nc].cpu().numpy(), want.cell_corner) and np.array_equal(DE.bits(point[:nc].cpu().numpy()), DE.bits(want.cell_point))
                 and np.array_equal(offsets.cpu().numpy(), want.offsets) and DE.same_rows(got, want.out) and np.array_equal(src[:T].cpu().numpy(), want.src))
        r["host"] = {"seconds": round(sec, 2), "equal": bool(equal), "routes_equal": bool(routes)}
    del sg, flat, flat4, out, a_buf, b_buf, work, cell, corner, point, offsets
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="strip_coarse,strip_fine,strip_ordered,bunny")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    import torch
    from ezrt_amd import trace
    if not torch.cuda.is_available():
        raise SystemExit("tools/decimate_rates.py needs a GPU: there is no CPU route to time")
    hip = trace.hip()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    res = {}
    for case in [m for m in a.cases.split(",") if m]:
        res[case] = measure(torch, hip, case, dev, stream, a, not a.no_host)
        print("%s: count %.3f ms, fill %.3f ms" % (case, res[case]["count"]["ms"], res[case]["fill"]["ms"]), file=sys.stderr, flush=True)
    print(json.dumps({"decimate_rates": res, "calls": a.calls, "repeats": a.repeats}))
    if a.table:
        cols = ("count", "count_all", "fill", "copy", "fill_4", "topology", "weld")
        with open(a.table, "a") as f:
            f.write("# tools/decimate_rates.py --calls %d --repeats %d on one MI355X, library: %s.  Device events around %d calls, median of %d\n"
                    "# repeats and their spread (max - min) / median; count, fill, copy and fill_4 take turns inside every repeat.\n"
                    "# count: ezrt_decimate_count_device with DEDUP, count_all: without; fill: ezrt_decimate_rows_device on 16-byte aligned rows;\n"
                    "# copy: torch's copy_ of half the bytes the fill reads plus writes (MB); fill_4: rows moved by 4 bytes (the per-lane route);\n"
                    "# topology (no component group) and weld (with flags) of the same rows.\n"
                    % (a.calls, a.repeats, os.environ.get("EZRT_HIP_LIB", "the product"), a.calls, a.repeats))
            f.write("%-13s %8s %7s | %s | %9s %8s %8s %8s | %s\n" % ("case", "n_rows", "MB", " | ".join("%9s ms %6s" % (c, "spread") for c in cols),
                                                                  "fill/copy", "f_4/fill", "cnt/weld", "cnt/topo", "host s  equal  routes"))
            for case, r in res.items():
                hst = r.get("host")
                f.write("%-13s %8d %7.1f | %s | %9.3f %8.3f %8.3f %8.3f | %s\n" % (
                    case, r["n_rows"], r["moved_mb"], " | ".join("%12.4f %6.3f" % (r[c]["ms"], r[c]["spread"]) for c in cols),
                    r["fill_over_copy"], r["fill_4_over_fill"], r["count_over_weld"], r["count_over_topology"],
                    "%6.2f %6s %7s" % (hst["seconds"], hst["equal"], hst["routes_equal"]) if hst else "not run"))
            for case, r in res.items():
                f.write("%s: grid %r, work %.1f MB; summary [T, collapsed, duplicates, no part, cells, cells kept, flags, live]: %r\n" % (
                    case, r["grid"], r["work_mb"], r["summary"]))


if __name__ == "__main__":
    main()
