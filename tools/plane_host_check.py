#!/usr/bin/env python3
"""tools/plane_host_check.py: the rule of the plane queries (plane_load, plane_side, plane_tri, plane_crossed, plane_point and
plane_segment of ezrt_amd/csrc/hip/ezrt_device.h) compiled for the HOST into a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, and held against tests/plane_expected.py on every pair of the GPU test's planes x all triangles of the
voxel solid, the open solid, the adversarial scene and the Bunny scene -- which pairs cross, every count and every row (q0, q1), on the
bits.  Needs no GPU; nothing loaded into python is sanitized.

The rule's section of ezrt_device.h (from its "----" comment to the next section) is cut out as it stands into a temporary directory
together with the inputs and the restatement's answers; tools/plane_host_check.cpp includes it behind a few lines that stand in for
the HIP types.  Compiler: $CXX, default g++.  Exit status 0: equal everywhere, no report."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("voxel_solid", "open_solid", "nasty", "bunny")


def cut(src, start, end):
    i = src.index(start)
    return src[i:src.index(end, i)]


def main():
    import plane_scenes as PS
    import plane_expected as PE
    from ezrt_amd import scenes
    src = open(os.path.join(ROOT, "ezrt_amd", "csrc", "hip", "ezrt_device.h")).read()
    rule = cut(src, "// ---- plane queries", "\n// ---- box-overlap queries")
    bunny_small = scenes.bunny_scene(subdiv=0, want_cache=True)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "plane_rule.inc"), "w").write(rule)
        for name in NAMES:
            tri, nodes, planes, kind = PS.inputs(name, bunny_small)
            offsets, ids, seg, _ = PE.section(planes, tri)
            out = lambda what, a, t: np.ascontiguousarray(a, t).tofile(os.path.join(d, "%s_%s.bin" % (name, what)))
            out("tri", PE.vertices(tri).reshape(-1, 9), np.float32)
            out("planes", planes, np.float32)
            out("offsets", offsets, np.int64)
            out("ids", ids, np.int32)
            out("seg", seg.view(np.uint32), np.uint32)
        exe = os.path.join(d, "plane_host_check")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "include"), "-I", d, "-o", exe,
                               os.path.join(ROOT, "tools", "plane_host_check.cpp")])
        return subprocess.call([exe, d] + list(NAMES))


if __name__ == "__main__":
    sys.exit(main())
