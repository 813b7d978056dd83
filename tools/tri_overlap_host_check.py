#!/usr/bin/env python3
"""tools/tri_overlap_host_check.py: the per-pair rule of the triangle-overlap queries (tri_live, tri_query, tri_overlaps of
ezrt_amd/csrc/hip/ezrt_device.h) compiled for the HOST into a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, and held against tests/tri_overlap_expected.py on every pair of the GPU test's query triangles x all
triangles of the voxel solid, the Bunny scene and the adversarial scene.  Needs no GPU; nothing loaded into python is sanitized.

The rule's section of ezrt_device.h (from its "---- triangle-overlap queries" comment to the next section) is cut out as it stands
into a temporary directory together with the inputs and the restatement's answers; tools/tri_overlap_host_check.cpp includes it
behind a few lines that stand in for the HIP types.  Compiler: $CXX, default g++.  Exit status 0: equal everywhere, no report."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = 900                                                          # tests/test_gpu_tri_overlap.py
NAMES = ("voxel_solid", "bunny", "nasty")


def main():
    import allhits_scenes as A
    import inside_scenes as IS
    import tri_overlap_expected as TE
    import tri_overlap_scenes as TS
    from ezrt_amd import scenes
    src = open(os.path.join(ROOT, "ezrt_amd", "csrc", "hip", "ezrt_device.h")).read()
    start = src.index("// ---- triangle-overlap queries")
    rule = src[start:src.index("\n// hitBVH", start)]
    bunny_small = scenes.bunny_scene(subdiv=0, want_cache=True)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "tri_rule.inc"), "w").write(rule)
        for i, name in enumerate(NAMES):
            if name == "voxel_solid":
                v = IS.voxel_solid()
                tri, nodes = v["tri"], v["nodes"]
            else:
                tri, nodes, _ = A.scene(name, bunny_small)
            q = TS.tris_for(tri, nodes, SEED + i)
            np.ascontiguousarray(TE.vertices(tri).reshape(-1, 9), np.float32).tofile(os.path.join(d, name + "_tri.bin"))
            q.tofile(os.path.join(d, name + "_q.bin"))
            TE.overlaps(q, tri).astype(np.uint8).tofile(os.path.join(d, name + "_over.bin"))
        exe = os.path.join(d, "tri_overlap_host_check")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "include"), "-I", d, "-o", exe,
                               os.path.join(ROOT, "tools", "tri_overlap_host_check.cpp")])
        return subprocess.call([exe, d] + list(NAMES))


if __name__ == "__main__":
    sys.exit(main())
