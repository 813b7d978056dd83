#!/usr/bin/env python3
"""tools/smooth_rates.py [--calls K] [--repeats R] [--meshes bunny,strip] [--table PATH]: milliseconds per call and per step of the mesh
smoothing (include/ezrt_smooth.h), beside a copy of the bytes one step moves and beside the topology and the weld of the same rows.

One JSON line, and with --table PATH a text table.  Meshes: `bunny`, the rows of the Bunny scene subdivided four times (1 272 140
triangles); `strip`, a strip of 10^6 triangles with shuffled ids (every vertex on the border); and `tile`, the test pool at
tile_rows_max rows (tests/subdiv_scenes.py: sized), for the two routes of the steps.

Per mesh, device events around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times, the median ms per call
and the spread (max - min) / median; the variants take turns inside every repeat:
  steps_1, steps_10   ezrt_smooth_rows_device with Taubin's pair on 16-byte aligned rows, global route: the memset, the plan, the steps
                      and the staged fill; step = (steps_10 - steps_1) / 9, the time of one step's launch
  copy                the yardstick: torch's device-to-device copy_ of half the bytes one step reads plus writes by the header's count,
                      36 V + 32 K for V moving vertices (vert_flags 0 or 1) with K star corners
  topology, weld      ezrt_mesh_topology_device without the component group and ezrt_mesh_weld_device with the flags group
  tile: lds_100, global_100   100 steps at tile_rows_max rows with tile_rows = 0 (one launch for all steps) and tile_rows = 1 (100 launches),
                      and whether the two gave the same bits"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
P = C.c_void_p
F = np.float32
LAM, MU = 0.5, -0.53


def measure(torch, hip, name, dev, stream, a):
    import clip_rates as CR
    import topology_rates as TR
    from ezrt_amd import _abi
    lib = _abi._declare(hip.lib, {**_abi.SMOOTH_ABI, **_abi.SMOOTH_SIZES})
    _abi._declare(hip.lib, _abi.WELD_ABI)
    tile_max = _abi.smooth_limits()
    if name == "tile":
        import boundary_scenes as BS
        import subdiv_scenes as SS
        tri, nodes = np.array(SS.sized(tile_max)), BS.proxy_nodes(tile_max)
    else:
        tri, nodes = TR.mesh(name, hip)
    R = np.ascontiguousarray(tri, F).reshape(-1, 36)
    n = R.shape[0]
    sg = hip.scene_create(R, nodes)
    h = P(stream.cuda_stream)
    d = lambda x: P(x.data_ptr())
    tb, twb = TR.buffers(torch, lib, n, dev)
    topology = TR.call(lib, sg, tb, twb, stream, components=False)
    i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
    wbuf = dict(vertex=i32(3 * n), vert_corner=i32(3 * n), star_offsets=i32(3 * n + 1), star=i32(3 * n), fans=i32(3 * n),
                vert_flags=torch.empty((3 * n,), dtype=torch.uint8, device=dev), summary=torch.zeros((8,), dtype=torch.int64, device=dev))
    wwb = int(lib.ezrt_weld_work_bytes(n))
    wwork = torch.empty((wwb // 8,), dtype=torch.int64, device=dev)
    weld = lambda: lib.ezrt_mesh_weld_device(sg._h, d(wbuf["vertex"]), d(wbuf["vert_corner"]), d(wbuf["star_offsets"]), d(wbuf["star"]),
                                             d(wbuf["fans"]), d(wbuf["vert_flags"]), d(wbuf["summary"]), d(wwork), wwb, h)
    r = {"n_rows": n, "library": os.environ.get("EZRT_HIP_LIB", "product"), "tile_rows_max": tile_max}
    r["topology"] = TR.timed(torch, stream, topology, a.calls, a.repeats)
    r["weld"] = TR.timed(torch, stream, weld, a.calls, a.repeats)
    torch.cuda.synchronize()
    nv = int(wbuf["summary"][1].item())
    k = np.diff(wbuf["star_offsets"][:nv + 1].cpu().numpy().astype(np.int64))
    moving = wbuf["vert_flags"][:nv].cpu().numpy() <= 1
    V, K = int(moving.sum()), int(k[moving].sum())
    step_bytes = 36 * V + 32 * K
    r.update(vertices=nv, moving=V, star_corners=K, step_mb=round(step_bytes / 1e6, 2))
    rows = torch.from_numpy(R).to(dev)
    out = torch.empty_like(rows)
    out2 = torch.empty_like(rows)
    summary = torch.zeros((8,), dtype=torch.int64, device=dev)
    wb = int(lib.ezrt_smooth_work_bytes(n))
    assert wb <= wwb
    work = wwork                                                               # the weld's buffer, handed on

    def smooth(steps, tile_rows, dst=out):
        return lambda: lib.ezrt_smooth_rows_device(sg._h, d(rows), n, d(tb["edge_class"]), d(wbuf["vertex"]), d(wbuf["star_offsets"]), d(wbuf["star"]),
                                                   d(wbuf["vert_flags"]), steps, LAM, MU, 0, tile_rows, d(dst), d(summary), d(work), wb, h)
    a_buf = torch.empty((max(step_bytes // 2, 8),), dtype=torch.uint8, device=dev)
    b_buf = torch.empty_like(a_buf)
    copy = lambda: b_buf.copy_(a_buf)
    if name == "tile":
        assert smooth(100, 0)() == 0 and smooth(100, 1, out2)() == 0, lib.ezrt_last_error()
        torch.cuda.synchronize()
        r["routes_equal"] = bool((out.view(torch.int32) == out2.view(torch.int32)).all())
        r.update(CR.timed_in_turn(torch, stream, {"lds_100": smooth(100, 0), "global_100": smooth(100, 1), "lds_1": smooth(1, 0),
                                                  "global_1": smooth(1, 1), "copy": copy}, a.calls, a.repeats))
        r["global_over_lds_100"] = round(r["global_100"]["ms"] / r["lds_100"]["ms"], 2)
    else:
        assert smooth(1, 0)() == 0 and smooth(10, 0)() == 0, lib.ezrt_last_error()
        r.update(CR.timed_in_turn(torch, stream, {"steps_1": smooth(1, 0), "steps_10": smooth(10, 0), "copy": copy}, a.calls, a.repeats))
        r["step_ms"] = round((r["steps_10"]["ms"] - r["steps_1"]["ms"]) / 9, 4)
        r["step_over_copy"] = round(r["step_ms"] / r["copy"]["ms"], 2)
        r["step_gb_s"] = round(step_bytes / r["step_ms"] / 1e6, 1)
        r["copy_gb_s"] = round(step_bytes / r["copy"]["ms"] / 1e6, 1)
    torch.cuda.synchronize()
    r["summary"] = summary.tolist()
    del sg, rows, out, out2, work, wwork, tb, wbuf, a_buf, b_buf
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--meshes", default="bunny,strip,tile")
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    import torch
    from ezrt_amd import trace
    if not torch.cuda.is_available():
        raise SystemExit("tools/smooth_rates.py needs a GPU: there is no CPU route to time")
    hip = trace.hip()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    res = {}
    for name in [m for m in a.meshes.split(",") if m]:
        res[name] = measure(torch, hip, name, dev, stream, a)
    print(json.dumps({"smooth_rates": res, "calls": a.calls, "repeats": a.repeats}))
    if a.table:
        with open(a.table, "a") as f:
            f.write("# tools/smooth_rates.py --calls %d --repeats %d on one MI355X, library: %s.  Device events around %d calls, median of %d\n"
                    "# repeats and their spread (max - min) / median; the variants of a mesh take turns inside every repeat.  Taubin's pair.\n"
                    "# steps_1, steps_10: ezrt_smooth_rows_device, global route, staged fill; step = (steps_10 - steps_1) / 9; copy: torch's copy_\n"
                    "# of half of 36 V + 32 K bytes (V moving vertices, K their star corners): what one step reads plus writes; topology (no\n"
                    "# component group) and weld (with flags) of the same rows.  tile: 100 steps and 1 step on the two routes at tile_rows_max rows.\n"
                    % (a.calls, a.repeats, os.environ.get("EZRT_HIP_LIB", "the product"), a.calls, a.repeats))
            for name, r in res.items():
                cols = ("lds_100", "global_100", "lds_1", "global_1", "copy", "topology", "weld") if name == "tile" else (
                    "steps_1", "steps_10", "copy", "topology", "weld")
                f.write("%-6s n_rows %8d  V %8d  moving %8d  K %9d  step MB %8.2f | %s\n" % (
                    name, r["n_rows"], r["vertices"], r["moving"], r["star_corners"], r["step_mb"],
                    " | ".join("%s %.4f ms %.3f" % (c, r[c]["ms"], r[c]["spread"]) for c in cols)))
                if name == "tile":
                    f.write("%-6s global_100 / lds_100 %.2f, routes equal: %s, summary %r\n" % (name, r["global_over_lds_100"], r["routes_equal"], r["summary"]))
                else:
                    f.write("%-6s step %.4f ms, %.2f times its copy (%.1f GB/s beside %.1f GB/s), summary %r\n" % (
                        name, r["step_ms"], r["step_over_copy"], r["step_gb_s"], r["copy_gb_s"], r["summary"]))


if __name__ == "__main__":
    main()
