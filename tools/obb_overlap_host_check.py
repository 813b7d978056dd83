#!/usr/bin/env python3
"""tools/obb_overlap_host_check.py: the rule of the oriented-box queries (obb_query, obb_hull_gate, obb_face_gate, obb_overlaps of
ezrt_amd/csrc/hip/ezrt_device.h) compiled for the HOST into a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, and held against tests/obb_overlap_expected.py on every pair of the GPU test's boxes x all triangles of the
voxel solid, the adversarial scene and the Bunny scene: liveness, overlaps of every pair, every box's row and count -- and the two
gates against every node box of the caller's tree: each gate on the bits of the restatement's (which compares the fp64 hull, where the
kernel compares the hull rounded inward), and no overlapping triangle below a rejected node.  Needs no GPU; nothing loaded into python
is sanitized.

The rule's section of ezrt_device.h (from its "----" comment to the next section) is cut out as it stands into a temporary directory
together with the inputs and the restatement's answers; tools/obb_overlap_host_check.cpp includes it behind a few lines that stand in
for the HIP types.  Compiler: $CXX, default g++.  Exit status 0: equal everywhere, no report."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("voxel_solid", "nasty", "bunny")
SEEDS = {"voxel_solid": 2200, "bunny": 2201, "nasty": 2202}           # tests/test_gpu_obb_overlap.py: SEED + NAMES.index(name)
K = 8


def cut(src, start, end):
    i = src.index(start)
    return src[i:src.index(end, i)]


def below(nodes):
    """(start int32 [nodes + 1], ids int32): the triangles below every node of the caller's tree, as one run of ids per node (a node
    that the root does not reach has none)"""
    N = np.asarray(nodes).reshape(-1, 12)
    runs = [np.zeros(0, np.int32)] * N.shape[0]
    order, stack = [], [1]
    while stack:
        i = stack.pop()
        order.append(i)
        if not N[i, 3] > 0:
            stack += [int(N[i, 0]), int(N[i, 1])]
    for i in reversed(order):                                          # children before parents
        if N[i, 3] > 0:
            runs[i] = np.arange(int(N[i, 4]), int(N[i, 4]) + int(N[i, 3]), dtype=np.int32)
        else:
            runs[i] = np.concatenate([runs[int(N[i, 0])], runs[int(N[i, 1])]])
    start = np.concatenate([[0], np.cumsum([r.size for r in runs])]).astype(np.int32)
    return start, np.concatenate(runs).astype(np.int32)


def main():
    import allhits_scenes as A
    import inside_scenes as IS
    import obb_overlap_expected as OE
    import obb_overlap_scenes as OS
    from ezrt_amd import scenes
    src = open(os.path.join(ROOT, "ezrt_amd", "csrc", "hip", "ezrt_device.h")).read()
    rule = cut(src, "// ---- oriented-box queries", "\n// ---- triangle-overlap queries")
    bunny_small = scenes.bunny_scene(subdiv=0, want_cache=True)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "obb_rule.inc"), "w").write(rule)
        for name in NAMES:
            if name == "voxel_solid":
                v = IS.voxel_solid()
                tri, nodes = v["tri"], v["nodes"]
            else:
                tri, nodes, _ = A.scene(name, bunny_small)
            c, u, _ = OS.boxes_for(tri, nodes, SEEDS[name])
            over = OE.overlaps(c, u, tri)
            rows, count = OE.lowest(over, K)
            N = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12)
            B = OE.Boxes(c, u)
            hull, face = np.zeros((c.shape[0], N.shape[0]), np.uint8), np.zeros((c.shape[0], N.shape[0]), np.uint8)
            for i in range(1, N.shape[0]):
                lo, hi = np.tile(N[i, 6:9], (c.shape[0], 1)), np.tile(N[i, 9:12], (c.shape[0], 1))
                hull[:, i] = OE.hull_passes(B, lo, hi)
                face[:, i] = B.live & OE.face_passes(B, lo, hi)
            start, ids = below(nodes)
            out = lambda what, a, t: np.ascontiguousarray(a, t).tofile(os.path.join(d, "%s_%s.bin" % (name, what)))
            out("tri", OE.vertices(tri).reshape(-1, 9), np.float32)
            out("centre", c, np.float32)
            out("axes", u, np.float32)
            out("live", B.live, np.uint8)
            out("over", over, np.uint8)
            out("rows", rows, np.int32)
            out("count", count, np.int32)
            out("nodebox", N[:, 6:12], np.float32)
            out("hull", hull, np.uint8)
            out("face", face, np.uint8)
            out("start", start, np.int32)
            out("ids", ids, np.int32)
        exe = os.path.join(d, "obb_overlap_host_check")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "include"), "-I", d, "-o", exe,
                               os.path.join(ROOT, "tools", "obb_overlap_host_check.cpp")])
        return subprocess.call([exe, d, str(K)] + list(NAMES))


if __name__ == "__main__":
    sys.exit(main())
