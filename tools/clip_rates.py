#!/usr/bin/env python3
"""tools/clip_rates.py [--calls K] [--repeats R] [--meshes bunny,strip_whole,strip_cut] [--no-host] [--table PATH]: milliseconds per
call of the plane clipping (include/ezrt_clip.h), count and fill apart, beside the fill's yardstick.

One JSON line, and with --table PATH a text table.  Cases: `bunny`, the rows of the Bunny scene subdivided four times (1 271 808
triangles) under a plane through the middle of its box (nearly every row is dropped); `strip_whole`, a strip of 10^6 triangles kept whole; `strip_cut`, the
same strip cut in every row (one and two pieces in turn: 1.5 * 10^6 output rows).

Per case, device events around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times, the median ms per call
and the spread (max - min) / median; the fill, its yardstick and the fill on pointers moved by 4 bytes take turns inside every repeat:
  count        ezrt_clip_count_device: the memset, the classification and the three launches of the prefix sum
  fill         ezrt_clip_rows_device with src and cut_edge, on 16-byte aligned rows: the staged route (the per-lane one where
               EZRT_HIP_LIB names the library built with -DEZRT_CLIP_PER_LANE=1: `make build_ab/libezrt_hip_clip_per_lane.so`)
  copy         the yardstick: torch's device-to-device copy_ of (bytes read + bytes written by the fill) / 2 bytes, which reads and
               writes that many
  fill_4       the fill on tri36 and out moved by 4 bytes: the per-lane route in the product library, on unaligned rows
`host`: tests/clip_expected.py on the same rows, wall-clock seconds, and whether offsets, summary, out, src and cut_edge are the
device's."""
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


def case(name):
    """(rows [n, 36], plane [4])"""
    import topology_scenes as TS
    from ezrt_amd import scenes
    if name == "bunny":
        R = np.ascontiguousarray(scenes.bunny_scene(subdiv=4).tri, F).reshape(-1, 36)
        V = R[:, :9].reshape(-1, 3).astype(np.float64)
        nrm = np.array([0.3, 1.0, 0.2])
        return R, np.append(nrm, nrm @ ((V.min(0) + V.max(0)) / 2)).astype(F)  # (the floor makes the box wide: nearly every row is dropped)
    R = TS.tri36(TS.strip(10 ** 6))
    return R, F([0, 0, 1, -1]) if name == "strip_whole" else F([0, 1, 0, 0.5])


def timed_in_turn(torch, stream, fns, calls, repeats):
    """{name: stats}: the functions take turns inside every repeat, each timed by device events around `calls` calls"""
    import topology_rates as TR
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / calls)
    return {k: TR.stats(v) for k, v in ms.items()}


def measure(torch, hip, name, dev, stream, a, host):
    from ezrt_amd import _abi
    lib = _abi._declare(hip.lib, _abi.CLIP_ABI)
    R, plane = case(name)
    n = R.shape[0]
    sg = hip.scene_create(*small_scene())
    flat = torch.empty((n * 36 + 4,), dtype=torch.float32, device=dev)         # the rows, and the same rows 4 bytes on
    flat4 = torch.empty((n * 36 + 4,), dtype=torch.float32, device=dev)
    flat[:n * 36] = torch.from_numpy(R).to(dev).reshape(-1)
    flat4[1:n * 36 + 1] = flat[:n * 36]
    d_plane = torch.from_numpy(plane).to(dev)
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    summary = torch.zeros((8,), dtype=torch.int64, device=dev)
    wb = int(lib.ezrt_clip_work_bytes(n))
    work = torch.empty((wb // 8,), dtype=torch.int64, device=dev)
    h = P(stream.cuda_stream)
    count = lambda: lib.ezrt_clip_count_device(sg._h, P(flat.data_ptr()), n, P(d_plane.data_ptr()), P(offsets.data_ptr()), P(summary.data_ptr()),
                                               P(work.data_ptr()), wb, h)
    assert count() == 0, lib.ezrt_last_error()
    sm = summary.tolist()
    T = sm[0]
    out = torch.empty((T * 36 + 4,), dtype=torch.float32, device=dev)
    src = torch.empty((T,), dtype=torch.int32, device=dev)
    cut = torch.empty((T,), dtype=torch.int8, device=dev)

    def fill(rows, to, shift):
        return lambda: lib.ezrt_clip_rows_device(sg._h, P(rows.data_ptr() + shift), n, P(d_plane.data_ptr()), P(offsets.data_ptr()), T,
                                                 P(to.data_ptr() + shift), P(src.data_ptr()), P(cut.data_ptr()), h)
    moved = (n + T) * 144                                                      # bytes the fill reads plus bytes it writes, rows alone
    a_buf = torch.empty((moved // 2,), dtype=torch.uint8, device=dev)
    b_buf = torch.empty((moved // 2,), dtype=torch.uint8, device=dev)
    r = {"n_rows": n, "T": T, "summary": sm, "moved_mb": round(moved / 1e6, 1), "library": os.environ.get("EZRT_HIP_LIB", "product")}
    import topology_rates as TR
    r["count"] = TR.timed(torch, stream, count, a.calls, a.repeats)
    r.update(timed_in_turn(torch, stream, {"fill": fill(flat, out, 0), "copy": lambda: b_buf.copy_(a_buf), "fill_4": fill(flat4, out, 4)},
                           a.calls, a.repeats))
    r["fill_over_copy"] = round(r["fill"]["ms"] / r["copy"]["ms"], 3)
    r["fill_4_over_fill"] = round(r["fill_4"]["ms"] / r["fill"]["ms"], 3)
    r["copy_gb_s"] = round(moved / r["copy"]["ms"] / 1e6, 1)
    r["fill_gb_s"] = round(moved / r["fill"]["ms"] / 1e6, 1)
    if host:
        import clip_expected as CE
        assert fill(flat, out, 0)() == 0
        torch.cuda.synchronize()
        got = (offsets.cpu().numpy(), out[:T * 36].cpu().numpy().reshape(-1, 36), src.cpu().numpy(), cut.cpu().numpy())
        assert fill(flat4, out, 4)() == 0
        torch.cuda.synchronize()
        got4 = out[1:T * 36 + 1].cpu().numpy().reshape(-1, 36)
        t0 = time.time()
        c = CE.clip(R, plane)
        sec = time.time() - t0
        equal = np.array_equal(got[0], c.offsets) and sm == c.summary.tolist() and CE.same_rows(got[1], c.out) and np.array_equal(got[2], c.src) and \
            np.array_equal(got[3], c.cut_edge)
        r["host"] = {"seconds": round(sec, 2), "equal": bool(equal), "routes_equal": bool(CE.same_rows(got4, c.out))}
    del sg, flat, flat4, out, a_buf, b_buf
    torch.cuda.empty_cache()
    return r


def small_scene():
    """a scene for the device and the error slot: the calls read none of its triangles"""
    import orient_scenes as OS
    return OS.scene("cube_pow2", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--meshes", default="bunny,strip_whole,strip_cut")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    import torch
    from ezrt_amd import trace
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_rates.py needs a GPU: there is no CPU route to time")
    hip = trace.hip()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    res = {}
    for name in [m for m in a.meshes.split(",") if m]:
        res[name] = measure(torch, hip, name, dev, stream, a, not a.no_host)
    print(json.dumps({"clip_rates": res, "calls": a.calls, "repeats": a.repeats}))
    if a.table:
        cols = ("count", "fill", "copy", "fill_4")
        with open(a.table, "a") as f:
            f.write("# tools/clip_rates.py --calls %d --repeats %d on one MI355X, library: %s.  Device events around %d calls, median of %d\n"
                    "# repeats and their spread (max - min) / median; fill, copy and fill_4 take turns inside every repeat.  count:\n"
                    "# ezrt_clip_count_device; fill: ezrt_clip_rows_device on 16-byte aligned rows; copy: torch's copy_ of (bytes read + written\n"
                    "# by the fill) / 2 bytes; fill_4: the fill on rows moved by 4 bytes (the per-lane route).  MB: bytes the fill reads plus\n"
                    "# writes, rows alone.\n" % (a.calls, a.repeats, os.environ.get("EZRT_HIP_LIB", "the product"), a.calls, a.repeats))
            f.write("%-11s %8s %8s %6s | %s | %9s %11s | %s\n" % ("case", "n_rows", "T", "MB", " | ".join("%8s ms %6s" % (c, "spread") for c in cols),
                                                                  "fill/copy", "fill_4/fill", "host s  equal  routes"))
            for name, r in res.items():
                hst = r.get("host")
                f.write("%-11s %8d %8d %6.1f | %s | %9.3f %11.3f | %s\n" % (
                    name, r["n_rows"], r["T"], r["moved_mb"], " | ".join("%11.4f %6.3f" % (r[c]["ms"], r[c]["spread"]) for c in cols),
                    r["fill_over_copy"], r["fill_4_over_fill"], "%6.2f %6s %7s" % (hst["seconds"], hst["equal"], hst["routes_equal"]) if hst else "not run"))
            for name, r in res.items():
                f.write("%s: summary [T, whole, cut, nothing, non-finite, cut edges, live, 0] = %r; copy %.1f GB/s, fill %.1f GB/s\n" % (
                    name, r["summary"], r["copy_gb_s"], r["fill_gb_s"]))


if __name__ == "__main__":
    main()
