#!/usr/bin/env python3
"""tools/self_overlap_host_check.py: the per-pair rule of the self-overlap queries (self_crosses of ezrt_amd/csrc/hip/ezrt_device.h,
with tri_query, tri_overlaps and seg_meets below it) compiled for the HOST into a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, and held against tests/self_overlap_expected.py on every pair of triangles of the voxel solid, the
defect scene, the adversarial scene, and of random small-integer triangles that share vertices by construction.  Needs no GPU;
nothing loaded into python is sanitized.

The rules' sections of ezrt_device.h (from the "---- triangle-overlap queries" comment to the next section: the self-overlap rule
follows the triangle rule) are cut out as they stand into a temporary directory together with the inputs and the restatement's
answers; tools/self_overlap_host_check.cpp includes them behind a few lines that stand in for the HIP types.  Compiler: $CXX,
default g++.  Exit status 0: equal everywhere, no report."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("voxel_solid", "defects", "nasty", "lattice")


def main():
    import allhits_scenes as A
    import inside_scenes as IS
    import self_overlap_expected as SE
    import self_overlap_scenes as SS
    import tri_overlap_expected as TE
    from ezrt_amd import scenes
    src = open(os.path.join(ROOT, "ezrt_amd", "csrc", "hip", "ezrt_device.h")).read()
    start = src.index("// ---- triangle-overlap queries")
    rule = src[start:src.index("\n// hitBVH", start)]
    assert "self_crosses" in rule
    bunny_small = scenes.bunny_scene(subdiv=0, want_cache=True)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "tri_rule.inc"), "w").write(rule)
        for name in NAMES:
            if name == "voxel_solid":
                tri = IS.voxel_solid()["tri"]
            elif name == "defects":
                tri = SS.defect_scene()["tri"]
            elif name == "lattice":                                   # 1 500 triangles on a 3^3 lattice: every s, many of them not live
                tri = np.random.default_rng(3).integers(-1, 2, (1500, 9)).astype(np.float32)
                tri[::50, 4] = np.nan
            else:
                tri = A.scene(name, bunny_small)[0]
            np.ascontiguousarray(TE.vertices(tri).reshape(-1, 9), np.float32).tofile(os.path.join(d, name + "_tri.bin"))
            SE.crosses(tri).astype(np.uint8).tofile(os.path.join(d, name + "_cross.bin"))
        exe = os.path.join(d, "self_overlap_host_check")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "include"), "-I", d, "-o", exe,
                               os.path.join(ROOT, "tools", "self_overlap_host_check.cpp")])
        return subprocess.call([exe, d] + list(NAMES))


if __name__ == "__main__":
    sys.exit(main())
