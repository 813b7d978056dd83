#!/usr/bin/env python3
"""tools/segment_host_check.py: the pair rule of the segment queries (closest_point_abc, segment_segment_closest, tri_distance_box,
seg_meets, segment_pair, segment_query, segment_gate, segment_candidate of ezrt_amd/csrc/hip/ezrt_device.h) compiled for the HOST into
a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, and held against tests/segment_expected.py on every pair
of the GPU test's segments x all triangles of the voxel solid, the adversarial scene and the Bunny scene: candidate, dist2, (x, y) and
crosses of every pair on the bits, lb <= dist2 for the triangle's own bounding box, and every query's answer -- the winner, dist2, both
points and crosses without and with d_max, and the capsule's row and count.  Needs no GPU; nothing loaded into python is sanitized.

The rule's sections of ezrt_device.h (closest-point, triangle-overlap with self-overlap, triangle-distance with segment, each from its
"----" comment to the next section) are cut out as they stand into a temporary directory together with the inputs and the
restatement's answers; tools/segment_host_check.cpp includes them behind a few lines that stand in for the HIP types.  Compiler: $CXX,
default g++.  Exit status 0: equal everywhere, no report."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("voxel_solid", "nasty", "bunny")
QUERIES = {"voxel_solid": None, "nasty": 500, "bunny": 300}        # of each scene's: 0.65 + 1.41 + 1.59 million pairs
K = 8


def cut(src, start, end):
    i = src.index(start)
    return src[i:src.index(end, i)]


def main():
    import segment_expected as SX
    import segment_scenes as SS
    import tri_overlap_expected as TE
    from ezrt_amd import scenes
    src = open(os.path.join(ROOT, "ezrt_amd", "csrc", "hip", "ezrt_device.h")).read()
    rule = (cut(src, "// ---- closest-point queries", "\n// ---- inside queries") + "\n" +
            cut(src, "// ---- triangle-overlap queries", "\n// hitBVH") + "\n" +
            cut(src, "// ---- triangle-distance queries", "\n// ------"))
    bunny_small = scenes.bunny_scene(subdiv=0, want_cache=True)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "segment_rule.inc"), "w").write(rule)
        for name in NAMES:
            tri, nodes, segs, d_max, radius = SS.host_case(name, bunny_small)
            n = QUERIES[name] or segs.shape[0]
            segs, d_max, radius = segs[:n], d_max[:n], radius[:n]
            V = TE.vertices(tri)
            m = V.shape[0]
            cols = [[] for _ in range(6)]
            step = max(1, (1 << 18) // m)
            for i0 in range(0, n, step):                               # every pair, with its points: no pruning here
                s = segs[i0:i0 + step]
                for c, a in zip(cols, SX.pairs(np.repeat(s, m, 0), np.tile(V, (s.shape[0], 1, 1)))):
                    c.append(a)
            cand, d2, x, y, cross, sub = [np.concatenate(c) for c in cols]
            table = (cand.reshape(n, m), d2.reshape(n, m), cross.reshape(n, m).astype(bool), sub.reshape(n, m))
            out = lambda what, a, t: np.ascontiguousarray(a, t).tofile(os.path.join(d, "%s_%s.bin" % (name, what)))
            out("tri", V.reshape(-1, 9), np.float32)
            out("q", segs, np.float32)
            out("dmax", d_max, np.float32)
            out("radius", radius, np.float32)
            out("cand", cand, np.uint8)
            out("d2", d2, np.float32)
            out("x", x, np.float32)
            out("y", y, np.float32)
            out("cross", cross, np.uint8)
            r = np.arange(n)
            for tag, dm in (("free", None), ("lim", d_max)):
                win, dist, wx, wy, wc, _ = SX.query(segs, tri, dm, table)
                out(tag + "_win", win, np.int32)
                out(tag + "_wd2", np.where(win >= 0, table[1][r, np.maximum(win, 0)], np.inf), np.float32)
                out(tag + "_wx", wx, np.float32)
                out(tag + "_wy", wy, np.float32)
                out(tag + "_wc", wc, np.uint8)
            rows, count = SX.capsule(segs, radius, tri, K, table)
            out("rows", rows, np.int32)
            out("count", count, np.int32)
        exe = os.path.join(d, "segment_host_check")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "include"), "-I", d, "-o", exe,
                               os.path.join(ROOT, "tools", "segment_host_check.cpp")])
        return subprocess.call([exe, d, str(K)] + list(NAMES))


if __name__ == "__main__":
    sys.exit(main())
