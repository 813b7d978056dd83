#!/usr/bin/env python3
"""tools/plane_loops_rates.py [--calls K] [--repeats R] [--scenes C2,C5] [--planes 1,64,1000,10000] [--tiles 0,8] [--single ROWS,..] [--host-seconds S]: segments per
second of the plane loops (include/ezrt_plane_loops.h) beside the plane queries' count and fill calls (include/ezrt_plane.h).

One JSON line, and with --table PATH a text table.  Scenes: the Bunny scene of C2 (bunny_scene(subdiv=2), 79 820 triangles) and the
scene of C5 (mega_scene(), 10^6 triangles).  Planes: 1, 64, 1 000 and 10 000 PARALLEL planes (a slicer's stack: normal +y, evenly
spaced over the scene's height) and as many RANDOM ones, tools/plane_rates.py's sets.  For each set the count call, the fill call
(with segments, capacity = the total) and the loops call (ezrt_plane_loops_device on the fill's rows: capacity = the total,
loop_capacity = the total, next and closed wanted, tile_rows the library's choice) are timed SEPARATELY, each with device events
around `calls` back-to-back calls on one stream after a warm-up call, `repeats` times: the median ms per call, and the spread
(max - min) / median of the repeats.  Msegments/s is rows over the median; `loops_to_fill` is the ratio of the two medians.
`lds_share` is the share of the rows that lie in planes of at most tile_rows_max rows (chained in LDS; the others in work memory),
`loops`, `closed` and `chained_rows` are read back from the answer.  `tile8`: the loops call with tile_rows = 8 (nearly every plane
on the global route) on the same rows; its answer must be the same bits (`equal`).

`single_plane`: ONE plane of 10^5 and of 10^6 rows (the section of a prism wall with shuffled triangles, computed on the host and
uploaded: one closed loop; on the scenes with at least that many triangles) -- a plane is one workgroup however long it is.

`host`: the only route without this call -- copy offsets and seg to the host and chain them with the dictionary restatement
(tests/plane_loops_expected.py) -- wall-clock seconds, on the parallel sets in ascending rows for as long as the time per row of the
set before predicts less than --host-seconds (the restatement is linear in the rows), and whether its answer is the device's."""
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


def stats(ms):
    med = float(np.median(ms))
    return {"ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)}


class Runner:
    def __init__(self, hip, sg, n_tri, dev, calls, repeats, tiles=(0, 8)):
        import torch
        self.tiles = tiles
        self.t, self.lib, self.sg, self.n_tri, self.dev, self.calls, self.repeats = torch, hip.lib, sg, n_tri, dev, calls, repeats
        self.stream = torch.cuda.current_stream(dev)

    def timed(self, fn):
        t = self.t
        assert fn() == 0
        t.cuda.synchronize()
        out = []
        for _ in range(self.repeats):
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record(self.stream)
            for _ in range(self.calls):
                fn()
            e1.record(self.stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / self.calls)
        return stats(out)

    def run(self, planes, tile_max):
        """(result dict, (offsets, seg, answer) as numpy or None)"""
        t, lib, sg, dev = self.t, self.lib, self.sg, self.dev
        n = planes.shape[0]
        S = int(lib.ezrt_plane_slices(n, self.n_tri, 0))
        h = P(self.stream.cuda_stream)
        part = t.empty((n, S), dtype=t.int32, device=dev)
        nc = t.empty((n,), dtype=t.int32, device=dev)
        off = t.empty((n + 1,), dtype=t.int64, device=dev)
        count = lambda: lib.ezrt_query_plane_count_device(sg._h, P(planes.data_ptr()), n, 0, P(part.data_ptr()), P(nc.data_ptr()), P(off.data_ptr()), h)
        res = {"count": self.timed(count)}
        total = int(off[n].item())
        ids = t.empty((total,), dtype=t.int32, device=dev)
        seg = t.empty((total, 6), dtype=t.float32, device=dev)
        fill = lambda: lib.ezrt_query_plane_section_device(sg._h, P(planes.data_ptr()), n, 0, P(part.data_ptr()), P(off.data_ptr()), total,
                                                           P(ids.data_ptr()), P(seg.data_ptr()), h)
        res["fill"] = self.timed(fill)
        kept = self.chain(off, seg, res, tile_max)
        res["slices"] = S
        res["fill"]["msegments_per_s"] = round(total / res["fill"]["ms"] / 1e3, 2)
        res["loops_to_fill"] = round(res["loops"]["ms"] / res["fill"]["ms"], 2)
        return res, kept

    def chain(self, off, seg, res, tile_max):
        """the loops call on the rows (off int64 [n + 1], seg float32 [total, 6]) at every tile_rows of self.tiles, into res; the rows and the answer"""
        t, lib, sg, dev = self.t, self.lib, self.sg, self.dev
        n, total = off.shape[0] - 1, seg.shape[0]
        h = P(self.stream.cuda_stream)
        wb = int(lib.ezrt_plane_loops_work_bytes(total))
        work = t.empty((wb // 8 + 1,), dtype=t.int64, device=dev)
        outs = []
        for tile_rows in self.tiles:
            nxt = t.full((total,), -1, dtype=t.int64, device=dev)
            order = t.full((total,), -1, dtype=t.int64, device=dev)
            pl = t.zeros((n + 1,), dtype=t.int64, device=dev)
            lo = t.full((total + 1,), -1, dtype=t.int64, device=dev)
            cl = t.zeros((max(total, 1),), dtype=t.uint8, device=dev)
            loops = lambda: lib.ezrt_plane_loops_device(sg._h, P(off.data_ptr()), n, P(seg.data_ptr()) if total else None, total, tile_rows,
                                                        P(nxt.data_ptr()) if total else None, P(order.data_ptr()) if total else None,
                                                        P(pl.data_ptr()), total, P(lo.data_ptr()), P(cl.data_ptr()), P(work.data_ptr()), wb, h)
            key = "loops" if tile_rows == 0 else "tile%d" % tile_rows
            res[key] = self.timed(loops)
            outs.append((nxt, order, pl, lo, cl))
            res[key]["equal"] = bool(all(t.equal(a, b) for a, b in zip(outs[0], outs[-1])))
        nxt, order, pl, lo, cl = outs[0]
        L = int(pl[n].item())
        rows = (off[1:] - off[:-1])
        res.update({"rows": total, "work_mib": round(wb / 2**20, 1), "loops_n": L, "closed": int(cl[:L].sum().item()),
                    "chained_rows": int(lo[L].item()), "lds_share": round(float(rows[rows <= tile_max].sum().item()) / max(total, 1), 4),
                    "longest_plane": int(rows.max().item())})
        for k in [k for k in res if k == "loops" or k.startswith("tile")]:
            res[k]["msegments_per_s"] = round(total / res[k]["ms"] / 1e3, 2)
        return (off, seg, nxt, order, pl, lo[:L + 1], cl[:L])


def ring_section(rows, seed=27):
    """(offsets int64 [2], seg float32 [rows, 2, 3]): the section z = 0.5 of the wall of a prism of rows / 2 sides between z = 0 and
    z = 1, its triangles shuffled -- ONE plane whose rows are one closed loop in an order unrelated to the rows'"""
    import plane_expected as PE
    n = rows // 2
    th = 2 * np.pi * np.arange(n) / n
    xy = np.stack([np.cos(th), np.sin(th)], 1).astype(np.float32)
    b = np.concatenate([xy, np.zeros((n, 1), np.float32)], 1)
    t = np.concatenate([xy, np.ones((n, 1), np.float32)], 1)
    b1, t1 = np.roll(b, -1, 0), np.roll(t, -1, 0)
    V = np.stack([np.stack([b, b1, t1], 1), np.stack([b, t1, t], 1)], 1).reshape(-1, 3, 3)
    off, ids, seg, _ = PE.section(np.float32([[0, 0, 1, 0.5]]), V[np.random.default_rng(seed).permutation(V.shape[0])])
    return off, seg


def host_route(kept, n_tri):
    """the dictionary restatement on the host copy of the rows, wall clock; (seconds, equal)"""
    import plane_loops_expected as LE
    off, seg, nxt, order, pl, lo, cl = kept
    t0 = time.perf_counter()
    on, sn = off.cpu().numpy(), seg.cpu().numpy()                            # the copy is part of the route
    t1 = time.perf_counter()
    w = LE.loops(on, sn, n_tri)
    t2 = time.perf_counter()
    same = (np.array_equal(w.next, nxt.cpu().numpy()) and np.array_equal(w.order, order.cpu().numpy()[:w.order.size])
            and np.array_equal(w.plane_loops, pl.cpu().numpy()) and np.array_equal(w.loop_offsets, lo.cpu().numpy())
            and np.array_equal(w.closed, cl.cpu().numpy()))
    return {"copy_s": round(t1 - t0, 4), "chain_s": round(t2 - t1, 3), "equal": bool(same)}


def measure(args):
    import torch
    from ezrt_amd import _abi, scenes, trace
    from plane_rates import plane_sets
    dev = torch.device("cuda", 0)
    hip = trace.hip()
    tile_max = _abi.plane_loops_limits()
    out = {"tile_rows_max": tile_max, "scenes": {}}
    makers = {"C2": lambda: scenes.bunny_scene(subdiv=2, hdr="shipped"), "C5": lambda: scenes.mega_scene()}
    for name in args.scenes.split(","):
        sc = makers[name]()
        tri = np.ascontiguousarray(sc.tri, np.float32)
        sg = hip.scene_create(sc.tri, sc.nodes)
        n_tri = int(tri.shape[0])
        run = Runner(hip, sg, n_tri, dev, args.calls, args.repeats, [int(x) for x in args.tiles.split(",")])
        rng = np.random.default_rng(24)
        res = {"triangles": n_tri, "sets": {}}
        s_per_row = 0.0                                                       # of the restatement, from the set before
        for n in [int(x) for x in args.planes.split(",")]:
            for kind, planes in plane_sets(tri, n, rng).items():
                row, kept = run.run(torch.from_numpy(planes).to(dev), tile_max)
                if kind == "parallel" and s_per_row * row["rows"] < args.host_seconds:
                    row["host"] = host_route(kept, n_tri)
                    s_per_row = row["host"]["chain_s"] / max(row["rows"], 1)
                    row["host"]["msegments_per_s"] = round(row["rows"] / max(row["host"]["chain_s"] + row["host"]["copy_s"], 1e-9) / 1e6, 4)
                res["sets"]["%d %s" % (n, kind)] = row
                del kept
                torch.cuda.empty_cache()
        single = {}
        for rows in [int(x) for x in args.single.split(",") if x]:                # ONE plane of that many rows: one workgroup
            if rows > n_tri:
                continue                                                      # (L2: no plane of this scene has more rows than triangles)
            off, seg = ring_section(rows)
            row = {}
            kept = run.chain(torch.from_numpy(off).to(dev), torch.from_numpy(seg.reshape(-1, 6)).to(dev), row, tile_max)
            if s_per_row * rows < args.host_seconds:
                row["host"] = host_route(kept, n_tri)
            single[str(rows)] = row
            del kept
        res["single_plane"] = single
        out["scenes"][name] = res
        sg.close()
    return out


def table(out):
    lines = ["# plane loops: median ms per call of `calls` = %d back-to-back calls, %d repeats, spread = (max - min) / median; tile_rows_max = %d"
             % (out["calls"], out["repeats"], out["tile_rows_max"]),
             "%-5s %-16s %10s %9s %9s | %9s %6s | %9s %6s %9s | %9s %6s %5s | %6s %8s %8s %6s | %s" %
             ("scene", "planes", "rows", "longest", "lds_share", "fill ms", "sprd", "loops ms", "sprd", "Mseg/s", "tile8 ms", "sprd", "equal",
              "ratio", "loops", "closed", "MiB", "host: copy s, chain s, Mseg/s, equal")]
    for name, sc in out["scenes"].items():
        for key, r in sc["sets"].items():
            h = r.get("host")
            lines.append("%-5s %-16s %10d %9d %9.4f | %9.4f %6.3f | %9.4f %6.3f %9.2f | %9.4f %6.3f %5s | %6.2f %8d %8d %6.0f | %s" %
                         (name, key, r["rows"], r["longest_plane"], r["lds_share"], r["fill"]["ms"], r["fill"]["spread"], r["loops"]["ms"],
                          r["loops"]["spread"], r["loops"]["msegments_per_s"], r["tile8"]["ms"], r["tile8"]["spread"], r["tile8"]["equal"],
                          r["loops_to_fill"], r["loops_n"], r["closed"], r["work_mib"],
                          "%.4f %.3f %.4f %s" % (h["copy_s"], h["chain_s"], h["msegments_per_s"], h["equal"]) if h else "-"))
    for name, sc in out["scenes"].items():
        for key, r in sc.get("single_plane", {}).items():
            h = r.get("host")
            lines.append("%-5s one plane, a shuffled ring of %8d rows: loops %9.4f ms (spread %.3f, %.2f Mseg/s), %d loop(s), %d closed, %d rounds x 3 | %s"
                         % (name, r["rows"], r["loops"]["ms"], r["loops"]["spread"], r["loops"]["msegments_per_s"], r["loops_n"], r["closed"],
                            int(np.ceil(np.log2(max(r["rows"], 2)))), "host: copy %.4f s, chain %.3f s, equal %s" % (h["copy_s"], h["chain_s"], h["equal"]) if h else "-"))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scenes", default="C2,C5")
    ap.add_argument("--planes", default="1,64,1000,10000")
    ap.add_argument("--host-seconds", type=float, default=60.0)
    ap.add_argument("--tiles", default="0,8", help="tile_rows values to time; 0 (the library's choice) first, and 8 for the table")
    ap.add_argument("--single", default="100000,1000000", help="rows of single-plane rings (on the scenes with that many triangles)")
    ap.add_argument("--table", default=None)
    args = ap.parse_args()
    from ezrt_amd.srchash import gpu_source_hash
    out = {"tool": "plane_loops_rates", "srchash": gpu_source_hash(), "calls": args.calls, "repeats": args.repeats}
    out.update(measure(args))
    print(json.dumps(out))
    if args.table:
        with open(args.table, "w") as f:
            f.write(table(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
