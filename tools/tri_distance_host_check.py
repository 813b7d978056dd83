#!/usr/bin/env python3
"""tools/tri_distance_host_check.py: the pair rule of the triangle-distance queries (closest_point_abc, segment_segment_closest,
tri_distance_box, tri_distance_pair, tri_distance_candidate of ezrt_amd/csrc/hip/ezrt_device.h, with tri_query and tri_overlaps)
compiled for the HOST into a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, and held against
tests/tri_distance_expected.py on every pair of the GPU test's query triangles x all triangles of the voxel solid, the adversarial
scene and the Bunny scene: candidate, dist2 and crosses of every pair on the bits, lb <= dist2 for the triangle's own bounding box, and
the answer of every query (winner, dist2, both points, crosses).  Needs no GPU; nothing loaded into python is sanitized.

The rule's sections of ezrt_device.h (closest-point, triangle-overlap and triangle-distance, each from its "----" comment to the next
section) are cut out as they stand into a temporary directory together with the inputs and the restatement's answers;
tools/tri_distance_host_check.cpp includes them behind a few lines that stand in for the HIP types.  Compiler: $CXX, default g++.
Exit status 0: equal everywhere, no report."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("voxel_solid", "nasty", "bunny")
BUNNY_QUERIES = 600                                                 # of the Bunny scene's: 3.2 of the 9.6 million pairs


def cut(src, start, end):
    i = src.index(start)
    return src[i:src.index(end, i)]


def main():
    import tri_distance_expected as TD
    import tri_distance_scenes as DS
    import tri_overlap_expected as TE
    from ezrt_amd import scenes
    src = open(os.path.join(ROOT, "ezrt_amd", "csrc", "hip", "ezrt_device.h")).read()
    rule = (cut(src, "// ---- closest-point queries", "\n// ---- inside queries") + "\n" +
            cut(src, "// ---- triangle-overlap queries", "\n// hitBVH") + "\n" +
            cut(src, "// ---- triangle-distance queries", "\n// ------"))
    bunny_small = scenes.bunny_scene(subdiv=0, want_cache=True)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "tri_distance_rule.inc"), "w").write(rule)
        for name in NAMES:
            tri, nodes, q = DS.host_case(name, bunny_small)[:3]
            if name == "bunny":
                q = q[:BUNNY_QUERIES]
            table = TD.dist2_all(q, tri)
            win, dist, x, y, crosses = TD.query(q, tri, table=table)
            out = lambda what, a, t: np.ascontiguousarray(a, t).tofile(os.path.join(d, "%s_%s.bin" % (name, what)))
            out("tri", TE.vertices(tri).reshape(-1, 9), np.float32)
            out("q", q, np.float32)
            out("cand", table[0], np.uint8)
            out("d2", table[1], np.float32)
            out("cross", table[2], np.uint8)
            out("win", win, np.int32)
            r = np.arange(q.shape[0])
            out("wd2", np.where(win >= 0, table[1][r, np.maximum(win, 0)], np.inf), np.float32)
            out("wx", x, np.float32)
            out("wy", y, np.float32)
            out("wc", crosses, np.uint8)
        exe = os.path.join(d, "tri_distance_host_check")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "include"), "-I", d, "-o", exe,
                               os.path.join(ROOT, "tools", "tri_distance_host_check.cpp")])
        return subprocess.call([exe, d] + list(NAMES))


if __name__ == "__main__":
    sys.exit(main())
