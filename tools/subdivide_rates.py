#!/usr/bin/env python3
"""tools/subdivide_rates.py [--calls K] [--repeats R] [--meshes bunny,strip] [--no-host] [--table PATH]: milliseconds per call of the
subdivision (include/ezrt_subdivide.h) in both modes, beside the fill's yardstick and beside the topology and the weld of the same rows.

One JSON line, and with --table PATH a text table.  Meshes: `bunny`, the rows of the Bunny scene subdivided four times (1 272 140
triangles); `strip`, a strip of 10^6 triangles with shuffled ids (every vertex on the border).

Per mesh, device events around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times, the median ms per call
and the spread (max - min) / median; midpoint, loop, the yardstick and midpoint on pointers moved by 4 bytes take turns inside every
repeat:
  midpoint     ezrt_subdivide_rows_device in MIDPOINT mode on 16-byte aligned rows: the memset and the staged fill (the per-lane fill
               where EZRT_HIP_LIB names the library built with -DEZRT_SUBDIV_PER_LANE=1: `make build_ab/libezrt_hip_subdiv_per_lane.so`)
  loop         the same call in LOOP mode: the memset, the vertex pass and the fill (the fill ALONE where EZRT_HIP_LIB names the library
               built with -DEZRT_SUBDIV_SKIP_VERTEX=1, `make build_ab/libezrt_hip_subdiv_no_vertex.so`: its output means nothing)
  copy         the yardstick: torch's device-to-device copy_ of (bytes read + bytes written by the fill) / 2 = 360 bytes per row, which
               reads and writes that many
  midpoint_4   MIDPOINT mode on tri36 and out moved by 4 bytes: the per-lane route in the product library, on unaligned rows
  topology     ezrt_mesh_topology_device without the component group, on a scene of the rows
  weld         ezrt_mesh_weld_device with the flags group, on the same scene
`host`: tests/subdiv_expected.py in MIDPOINT mode on the same rows, wall-clock seconds, whether out and summary are the device's, and
whether the two routes gave the same bits in both modes."""
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
MIDPOINT, LOOP = 0, 1


def measure(torch, hip, name, dev, stream, a, host):
    import clip_rates as CR
    import topology_rates as TR
    from ezrt_amd import _abi
    lib = _abi._declare(hip.lib, _abi.SUBDIVIDE_ABI)
    _abi._declare(hip.lib, _abi.WELD_ABI)
    tri, nodes = TR.mesh(name, hip)
    R = np.ascontiguousarray(tri, F).reshape(-1, 36)
    n = R.shape[0]
    sg = hip.scene_create(R, nodes)
    h = P(stream.cuda_stream)
    d = lambda x: P(x.data_ptr())
    # the topology and the weld of the rows: timed, and Loop mode's arrays
    tb, twb = TR.buffers(torch, lib, n, dev)
    topology = TR.call(lib, sg, tb, twb, stream, components=False)
    i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
    wbuf = dict(vertex=i32(3 * n), vert_corner=i32(3 * n), star_offsets=i32(3 * n + 1), star=i32(3 * n), fans=i32(3 * n),
                vert_flags=torch.empty((3 * n,), dtype=torch.uint8, device=dev), summary=torch.zeros((8,), dtype=torch.int64, device=dev))
    wwb = int(lib.ezrt_weld_work_bytes(n))
    wwork = torch.empty((wwb // 8,), dtype=torch.int64, device=dev)
    weld = lambda: lib.ezrt_mesh_weld_device(sg._h, d(wbuf["vertex"]), d(wbuf["vert_corner"]), d(wbuf["star_offsets"]), d(wbuf["star"]),
                                             d(wbuf["fans"]), d(wbuf["vert_flags"]), d(wbuf["summary"]), d(wwork), wwb, h)
    r = {"n_rows": n, "moved_mb": round(n * 720 / 1e6, 1), "library": os.environ.get("EZRT_HIP_LIB", "product")}
    r["topology"] = TR.timed(torch, stream, topology, a.calls, a.repeats)
    r["weld"] = TR.timed(torch, stream, weld, a.calls, a.repeats)
    del tb["work"], wwork
    torch.cuda.empty_cache()
    arrays = [tb["twin"], tb["edge_class"], wbuf["vertex"], wbuf["star_offsets"], wbuf["star"], wbuf["vert_flags"]]
    flat = torch.empty((n * 36 + 4,), dtype=torch.float32, device=dev)         # the rows, and the same rows 4 bytes on
    flat4 = torch.empty((n * 36 + 4,), dtype=torch.float32, device=dev)
    flat[:n * 36] = torch.from_numpy(R).to(dev).reshape(-1)
    flat4[1:n * 36 + 1] = flat[:n * 36]
    out = torch.empty((4 * n * 36 + 4,), dtype=torch.float32, device=dev)
    summary = torch.zeros((8,), dtype=torch.int64, device=dev)
    wb = int(lib.ezrt_subdivide_work_bytes(n, LOOP))
    work = torch.zeros((wb // 8,), dtype=torch.int64, device=dev)

    def sub(mode, rows, shift):
        arr = [d(x) for x in arrays] if mode == LOOP else [None] * 6
        return lambda: lib.ezrt_subdivide_rows_device(sg._h, P(rows.data_ptr() + shift), n, mode, *arr, P(out.data_ptr() + shift), d(summary), d(work),
                                                      wb, h)
    a_buf = torch.empty((n * 360,), dtype=torch.uint8, device=dev)
    b_buf = torch.empty((n * 360,), dtype=torch.uint8, device=dev)
    for fn in (sub(MIDPOINT, flat, 0), sub(LOOP, flat, 0), sub(MIDPOINT, flat4, 4)):
        assert fn() == 0, lib.ezrt_last_error()
    r.update(CR.timed_in_turn(torch, stream, {"midpoint": sub(MIDPOINT, flat, 0), "loop": sub(LOOP, flat, 0), "copy": lambda: b_buf.copy_(a_buf),
                                              "midpoint_4": sub(MIDPOINT, flat4, 4)}, a.calls, a.repeats))
    r["midpoint_over_copy"] = round(r["midpoint"]["ms"] / r["copy"]["ms"], 3)
    r["loop_over_copy"] = round(r["loop"]["ms"] / r["copy"]["ms"], 3)
    r["midpoint_4_over_midpoint"] = round(r["midpoint_4"]["ms"] / r["midpoint"]["ms"], 3)
    r["copy_gb_s"] = round(n * 720 / r["copy"]["ms"] / 1e6, 1)
    r["midpoint_gb_s"] = round(n * 720 / r["midpoint"]["ms"] / 1e6, 1)
    if host:
        import subdiv_expected as SE
        got = {}
        for mode in (MIDPOINT, LOOP):
            assert sub(mode, flat, 0)() == 0
            torch.cuda.synchronize()
            got[mode] = (out[:4 * n * 36].cpu().numpy().reshape(-1, 36), summary.tolist())
            assert sub(mode, flat4, 4)() == 0
            torch.cuda.synchronize()
            got[mode] += (SE.same_rows(out[1:4 * n * 36 + 1].cpu().numpy().reshape(-1, 36), got[mode][0]) and summary.tolist() == got[mode][1],)
        t0 = time.time()
        want = SE.subdivide(R, SE.MIDPOINT)
        sec = time.time() - t0
        r["summary_midpoint"], r["summary_loop"] = got[MIDPOINT][1], got[LOOP][1]
        r["host"] = {"seconds": round(sec, 2), "equal": bool(SE.same_rows(got[MIDPOINT][0], want[0]) and got[MIDPOINT][1] == want[1].tolist()),
                     "routes_equal": bool(got[MIDPOINT][2] and got[LOOP][2])}
    del sg, flat, flat4, out, a_buf, b_buf, work, arrays, tb, wbuf
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--meshes", default="bunny,strip")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    import torch
    from ezrt_amd import trace
    if not torch.cuda.is_available():
        raise SystemExit("tools/subdivide_rates.py needs a GPU: there is no CPU route to time")
    hip = trace.hip()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    res = {}
    for name in [m for m in a.meshes.split(",") if m]:
        res[name] = measure(torch, hip, name, dev, stream, a, not a.no_host)
    print(json.dumps({"subdivide_rates": res, "calls": a.calls, "repeats": a.repeats}))
    if a.table:
        cols = ("midpoint", "loop", "copy", "midpoint_4", "topology", "weld")
        with open(a.table, "a") as f:
            f.write("# tools/subdivide_rates.py --calls %d --repeats %d on one MI355X, library: %s.  Device events around %d calls, median of %d\n"
                    "# repeats and their spread (max - min) / median; midpoint, loop, copy and midpoint_4 take turns inside every repeat.\n"
                    "# midpoint, loop: ezrt_subdivide_rows_device on 16-byte aligned rows (loop: with the vertex pass, unless the library is the\n"
                    "# no_vertex variant); copy: torch's copy_ of 360 bytes per row; midpoint_4: rows moved by 4 bytes (the per-lane route);\n"
                    "# topology (no component group) and weld (with flags) of the same rows.  MB: 720 bytes per row.\n"
                    % (a.calls, a.repeats, os.environ.get("EZRT_HIP_LIB", "the product"), a.calls, a.repeats))
            f.write("%-6s %8s %6s | %s | %8s %9s %8s | %s\n" % ("mesh", "n_rows", "MB", " | ".join("%10s ms %6s" % (c, "spread") for c in cols),
                                                             "mid/copy", "loop/copy", "m_4/mid", "host s  equal  routes"))
            for name, r in res.items():
                hst = r.get("host")
                f.write("%-6s %8d %6.1f | %s | %8.3f %9.3f %8.3f | %s\n" % (
                    name, r["n_rows"], r["moved_mb"], " | ".join("%13.4f %6.3f" % (r[c]["ms"], r[c]["spread"]) for c in cols),
                    r["midpoint_over_copy"], r["loop_over_copy"], r["midpoint_4_over_midpoint"],
                    "%6.2f %6s %7s" % (hst["seconds"], hst["equal"], hst["routes_equal"]) if hst else "not run"))
            for name, r in res.items():
                f.write("%s: copy %.1f GB/s, midpoint %.1f GB/s; summary [4 n, S5, S6, S7, interior, midpoint, mode, 0]: loop %r\n" % (
                    name, r["copy_gb_s"], r["midpoint_gb_s"], r.get("summary_loop")))


if __name__ == "__main__":
    main()
