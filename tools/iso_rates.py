#!/usr/bin/env python3
"""tools/iso_rates.py [--calls K] [--repeats R] [--cases sphere128,sphere256,noise128] [--no-host] [--no-offset] [--table PATH]:
milliseconds per call of the isosurface extraction (include/ezrt_isosurface.h), count and fill apart, each beside its yardstick, and the
offset surface end to end.

One JSON line, and with --table PATH a text table.  Cases: `sphere128` and `sphere256`, the distance to a sphere with an off-lattice
centre on a 128^3 and a 256^3 grid (the surface is in a few per cent of the blocks); `noise128`, Gaussian noise on a 128^3 grid (every
block emits, about six rows per cell).

Per case, device events around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times, the median ms per call
and the spread (max - min) / median; a step, its yardstick and the fill on an `out` moved by 4 bytes take turns inside every repeat:
  count        ezrt_iso_count_device: the memset, the classification and the three launches of the prefix sum
  count_copy   its yardstick: torch's device-to-device copy_ of (the bytes of values) / 2 bytes, which reads and writes that many
  fill         ezrt_iso_rows_device with cell, on a 16-byte aligned out: the staged route (the per-lane one where EZRT_HIP_LIB names
               the library built with -DEZRT_ISO_PER_LANE=1: `make build_ab/libezrt_hip_iso_per_lane.so`)
  fill_copy    its yardstick: copy_ of (the bytes of values + the bytes of the rows) / 2 bytes
  fill_4       the fill on an out moved by 4 bytes: the per-lane route in the product library
`host`: tests/iso_expected.py on the same field (sphere128 only: the restatement of 15.4 * 10^6 rows of noise needs gigabytes), wall-clock
seconds, and whether offsets, summary, out and cell are the device's; `routes_equal`, for every case: the rows of the two routes are the
same words.
`offset`: query.grid_points, query.signed_distance of the shipped Bunny mesh (4968 triangles) and query.isosurface_rows at a level of 2 %
of the mesh's diagonal on a 128^3 grid, a host clock around each step ended by a device synchronise, the median of `repeats` runs after a
warm-up run."""
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
MATERIAL = np.arange(1, 19, dtype=np.float64).astype(F) * F(0.25)


def case(name):
    """(values [n, n, n], grid8 [8])"""
    n = int(name[-3:])
    if name.startswith("noise"):
        V = np.random.default_rng(39).standard_normal((n, n, n)).astype(F)
    else:
        a = np.arange(n, dtype=np.float64)
        c = (n - 1) / 2.0
        z, y, x = a[:, None, None], a[None, :, None], a[None, None, :]
        V = (np.sqrt((x - c - 0.13) ** 2 + (y - c + 0.09) ** 2 + (z - c - 0.27) ** 2) - 0.33 * (n - 1)).astype(F)
    h = 2.0 / (n - 1)
    return V, np.array([-1, -1, -1, h, h, h, 0.0, 0.0], np.float64).astype(F)


def measure(torch, hip, name, dev, stream, a, host):
    import clip_rates as CR
    from ezrt_amd import _abi
    lib = _abi._declare(_abi._declare(hip.lib, _abi.ISO_ABI), _abi.ISO_SIZES)
    V, grid = case(name)
    nz, ny, nx = V.shape
    n_cells = (nx - 1) * (ny - 1) * (nz - 1)
    nb = (n_cells + _abi.ISO_BLOCK - 1) // _abi.ISO_BLOCK
    sg = hip.scene_create(*CR.small_scene())
    values = torch.from_numpy(V).to(dev)
    d_grid, d_mat = torch.from_numpy(grid).to(dev), torch.from_numpy(MATERIAL).to(dev)
    offsets = torch.zeros((nb + 1,), dtype=torch.int64, device=dev)
    summary = torch.zeros((8,), dtype=torch.int64, device=dev)
    wb = int(lib.ezrt_iso_work_bytes(nx, ny, nz))
    work = torch.empty((wb // 8,), dtype=torch.int64, device=dev)
    h = P(stream.cuda_stream)
    count = lambda: lib.ezrt_iso_count_device(sg._h, P(values.data_ptr()), nx, ny, nz, P(d_grid.data_ptr()), P(offsets.data_ptr()), P(summary.data_ptr()),
                                              P(work.data_ptr()), wb, h)
    assert count() == 0, lib.ezrt_last_error()
    sm = summary.tolist()
    T = sm[0]
    out = torch.empty((T * 36 + 4,), dtype=torch.float32, device=dev)
    cell = torch.empty((T,), dtype=torch.int32, device=dev)

    def fill(shift):
        return lambda: lib.ezrt_iso_rows_device(sg._h, P(values.data_ptr()), nx, ny, nz, P(d_grid.data_ptr()), P(d_mat.data_ptr()), P(offsets.data_ptr()), T,
                                                P(out.data_ptr() + shift), P(cell.data_ptr()), h)
    count_moved = V.size * 4                                                   # bytes the count must read (its offsets are 8 B per 256 cells)
    fill_moved = V.size * 4 + T * 144                                          # bytes the fill must read plus write: the values once, the rows once
    bufs = [torch.empty((m // 2,), dtype=torch.uint8, device=dev) for m in (count_moved, count_moved, fill_moved, fill_moved)]
    r = {"shape": [nz, ny, nx], "n_cells": n_cells, "n_blocks": nb, "T": T, "summary": sm, "count_mb": round(count_moved / 1e6, 1),
         "fill_mb": round(fill_moved / 1e6, 1), "library": os.environ.get("EZRT_HIP_LIB", "product")}
    r.update(CR.timed_in_turn(torch, stream, {"count": count, "count_copy": lambda: bufs[1].copy_(bufs[0])}, a.calls, a.repeats))
    r.update(CR.timed_in_turn(torch, stream, {"fill": fill(0), "fill_copy": lambda: bufs[3].copy_(bufs[2]), "fill_4": fill(4)}, a.calls, a.repeats))
    r["count_over_copy"] = round(r["count"]["ms"] / r["count_copy"]["ms"], 3)
    r["fill_over_copy"] = round(r["fill"]["ms"] / r["fill_copy"]["ms"], 3)
    r["fill_4_over_fill"] = round(r["fill_4"]["ms"] / r["fill"]["ms"], 3)
    r["fill_gb_s"] = round(fill_moved / r["fill"]["ms"] / 1e6, 1)
    r["fill_copy_gb_s"] = round(fill_moved / r["fill_copy"]["ms"] / 1e6, 1)
    assert fill(0)() == 0
    torch.cuda.synchronize()
    staged = out[:T * 36].view(torch.int32).clone()
    assert fill(4)() == 0
    torch.cuda.synchronize()
    r["routes_equal"] = bool(torch.equal(staged, out[1:T * 36 + 1].view(torch.int32)))
    if host:
        import iso_expected as IE
        t0 = time.time()
        I = IE.iso(V, grid, MATERIAL)
        sec = time.time() - t0
        equal = np.array_equal(offsets.cpu().numpy(), I.offsets) and sm == I.summary.tolist() and np.array_equal(cell.cpu().numpy(), I.cell) and \
            IE.same_rows(staged.view(torch.float32).cpu().numpy().reshape(-1, 36), I.out)
        r["host"] = {"seconds": round(sec, 2), "equal": bool(equal)}
    del staged
    del sg, values, out, bufs
    torch.cuda.empty_cache()
    return r


def offset_surface(torch, hip, dev, a, n=128):
    """the end-to-end offset surface of the shipped Bunny mesh: seconds per step, each ended by a device synchronise"""
    import topology_rates as TR
    from ezrt_amd import query, scenes
    import inside_scenes as INS
    v, f = scenes.mesh("bunny")                                                # the shipped mesh alone, without the scene's floor
    tri, nodes = INS.build(INS.tri36(np.ascontiguousarray(v[f], F)))
    sg = hip.scene_create(tri, nodes)
    Vt = np.asarray(v, np.float64)
    lo, hi = Vt.min(0), Vt.max(0)
    r = 0.02 * float(np.linalg.norm(hi - lo))
    lo, hi = lo - 3 * r, hi + 3 * r
    spacing = [float(x) for x in (hi - lo) / (n - 1)]
    origin = [float(x) for x in lo]
    shape = (n, n, n)
    ms = {"grid_points": [], "signed_distance": [], "isosurface_rows": [], "total": []}
    T = 0
    for it in range(a.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pts = query.grid_points(shape, origin, spacing, dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sd = query.signed_distance(sg, pts)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        got = query.isosurface_rows(sg, sd.dist.reshape(shape), r, origin, spacing)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        T = got.rows.shape[0]
        if it:                                                                 # the first run warms up
            for k, v in (("grid_points", t1 - t0), ("signed_distance", t2 - t1), ("isosurface_rows", t3 - t2), ("total", t3 - t0)):
                ms[k].append(1e3 * v)
    out = {k: TR.stats(v) for k, v in ms.items()}
    out.update({"n_tri": int(f.shape[0]), "shape": list(shape), "level": round(r, 5), "T": T, "summary": got.summary.tolist()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="sphere128,sphere256,noise128")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-offset", action="store_true")
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    import torch
    from ezrt_amd import trace
    if not torch.cuda.is_available():
        raise SystemExit("tools/iso_rates.py needs a GPU: there is no CPU route to time")
    hip = trace.hip()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    res = {}
    for name in [m for m in a.cases.split(",") if m]:
        res[name] = measure(torch, hip, name, dev, stream, a, not a.no_host and name == "sphere128")
    off = None if a.no_offset else offset_surface(torch, hip, dev, a)
    print(json.dumps({"iso_rates": res, "offset_surface": off, "calls": a.calls, "repeats": a.repeats}))
    if a.table:
        cols = ("count", "count_copy", "fill", "fill_copy", "fill_4")
        with open(a.table, "a") as f:
            f.write("# tools/iso_rates.py --calls %d --repeats %d on one MI355X, library: %s.  Device events around %d calls, median of %d\n"
                    "# repeats and their spread (max - min) / median; a step and its yardstick take turns inside every repeat.  count:\n"
                    "# ezrt_iso_count_device; count_copy: torch's copy_ of (bytes of values) / 2 bytes; fill: ezrt_iso_rows_device on a 16-byte\n"
                    "# aligned out; fill_copy: copy_ of (bytes of values + bytes of rows) / 2 bytes; fill_4: the fill on an out moved by 4 bytes\n"
                    "# (the per-lane route).  MB: bytes the fill must read plus write.\n" % (
                        a.calls, a.repeats, os.environ.get("EZRT_HIP_LIB", "the product"), a.calls, a.repeats))
            f.write("%-10s %9s %9s %7s | %s | %10s %9s %11s | %s\n" % ("case", "n_cells", "T", "MB", " | ".join("%10s ms %6s" % (c, "spread") for c in cols),
                                                                        "count/copy", "fill/copy", "fill_4/fill", "routes  host s  equal"))
            for name, r in res.items():
                hst = r.get("host")
                f.write("%-10s %9d %9d %7.1f | %s | %10.3f %9.3f %11.3f | %s\n" % (
                    name, r["n_cells"], r["T"], r["fill_mb"], " | ".join("%13.4f %6.3f" % (r[c]["ms"], r[c]["spread"]) for c in cols),
                    r["count_over_copy"], r["fill_over_copy"], r["fill_4_over_fill"],
                    "%6s  " % r["routes_equal"] + ("%6.2f %6s" % (hst["seconds"], hst["equal"]) if hst else "not run")))
            for name, r in res.items():
                f.write("%s: summary [T, cells that emit, finite cells that emit nothing, non-finite cells, blocks that emit, n_cells, live, 0] = %r; "
                        "fill %.1f GB/s, its copy %.1f GB/s\n" % (name, r["summary"], r["fill_gb_s"], r["fill_copy_gb_s"]))
            if off:
                f.write("offset surface of the shipped Bunny mesh (%d triangles) on a %s grid at level %g, ms per step, a host clock around each step "
                        "ended by a device synchronise, median of %d runs after a warm-up (spread): grid_points %.3f (%.2f), signed_distance %.3f (%.2f), "
                        "isosurface_rows %.3f (%.2f), total %.3f (%.2f); T = %d rows\n" % (
                            off["n_tri"], "x".join(str(x) for x in off["shape"]), off["level"], a.repeats, off["grid_points"]["ms"], off["grid_points"]["spread"],
                            off["signed_distance"]["ms"], off["signed_distance"]["spread"], off["isosurface_rows"]["ms"], off["isosurface_rows"]["spread"],
                            off["total"]["ms"], off["total"]["spread"], off["T"]))


if __name__ == "__main__":
    main()
