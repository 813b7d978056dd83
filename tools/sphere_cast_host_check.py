#!/usr/bin/env python3
"""tools/sphere_cast_host_check.py: the pair rule of the sphere-cast queries (sphere_cast_live, sphere_cast_slab, sphere_cast_pair,
sphere_cast_candidate, sphere_cast_at of ezrt_amd/csrc/hip/ezrt_device.h, with closest_point_candidate) compiled for the HOST into a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, and held against tests/sphere_cast_expected.py on every pair
of the GPU test's queries x all triangles of the voxel solid, the adversarial scene and the Bunny scene: gate, tnear, candidate, t,
sub-candidate and contact point of every pair on the bits, tnear <= t, and the answer of every query (winner, t, point, touching).  Needs no GPU; nothing
loaded into python is sanitized.

The rule's sections of ezrt_device.h (closest-point and sphere-cast, each from its "----" comment to the next section) are cut out as
they stand into a temporary directory together with the inputs and the restatement's answers; tools/sphere_cast_host_check.cpp
includes them behind a few lines that stand in for the HIP types.  Compiler: $CXX, default g++.  Exit status 0: equal everywhere, no
report."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("voxel_solid", "nasty", "bunny")


def cut(src, start, end):
    i = src.index(start)
    return src[i:src.index(end, i)]


def main():
    import sphere_cast_expected as SE
    import sphere_cast_scenes as SS
    from ezrt_amd import scenes
    src = open(os.path.join(ROOT, "ezrt_amd", "csrc", "hip", "ezrt_device.h")).read()
    rule = (cut(src, "// ---- closest-point queries", "\n// ---- inside queries") + "\n" +
            cut(src, "// ---- sphere-cast queries", "\n// ---- triangle-distance queries"))
    bunny_small = scenes.bunny_scene(subdiv=0, want_cache=True)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "sphere_cast_rule.inc"), "w").write(rule)
        for name in NAMES:
            tri, nodes, rays, radius = SS.host_case(name, bunny_small)
            cand, t, sub, gate, tnear, px = SE.swept_all(rays, radius, tri, points=True)
            win, wt, wx, wtouch, _ = SE.query(rays, radius, tri, table=(cand, t, sub))
            out = lambda what, a, ty: np.ascontiguousarray(a, ty).tofile(os.path.join(d, "%s_%s.bin" % (name, what)))  # noqa: E731
            out("tri", SE.vertices(tri).reshape(-1, 9), np.float32)
            out("ray", rays, np.float32)
            out("rad", radius, np.float32)
            out("gate", gate, np.uint8)
            out("tnear", tnear, np.float32)
            out("cand", cand, np.uint8)
            out("t", t, np.float32)
            out("sub", sub, np.int8)
            out("px", px, np.float32)
            out("win", win, np.int32)
            out("wt", wt, np.float32)
            out("wx", wx, np.float32)
            out("wtouch", wtouch, np.uint8)
        exe = os.path.join(d, "sphere_cast_host_check")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "include"), "-I", d, "-o", exe,
                               os.path.join(ROOT, "tools", "sphere_cast_host_check.cpp")])
        return subprocess.call([exe, d] + list(NAMES))


if __name__ == "__main__":
    sys.exit(main())
