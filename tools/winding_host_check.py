#!/usr/bin/env python3
"""tools/winding_host_check.py: the rule of the winding-number queries (winding_tri, winding_term, winding_pair, winding_of of
ezrt_amd/csrc/hip/ezrt_device.h) compiled for the HOST into a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, and held against tests/winding_expected.py on every pair of the GPU test's points x all triangles of the
voxel solid, the open solid, the adversarial scene and the Bunny scene -- every term q_k, every sum and every float, on the bits.
Needs no GPU; nothing loaded into python is sanitized.

The rule's section of ezrt_device.h (from its "----" comment to the next section) is cut out as it stands into a temporary directory
together with the inputs and the restatement's answers; tools/winding_host_check.cpp includes it behind a few lines that stand in for
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
    import winding_scenes as WS
    import winding_expected as WE
    from ezrt_amd import scenes
    src = open(os.path.join(ROOT, "ezrt_amd", "csrc", "hip", "ezrt_device.h")).read()
    rule = cut(src, "// ---- winding-number queries", "\n// ---- box-overlap queries")
    bunny_small = scenes.bunny_scene(subdiv=0, want_cache=True)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "winding_rule.inc"), "w").write(rule)
        for name in NAMES:
            tri, nodes, pts = WS.inputs(name, bunny_small)
            q = WE.terms(pts, tri)
            S = q.sum(1)
            out = lambda what, a, t: np.ascontiguousarray(a, t).tofile(os.path.join(d, "%s_%s.bin" % (name, what)))
            out("tri", WE.vertices(tri).reshape(-1, 9), np.float32)
            out("points", pts, np.float32)
            out("terms", q, np.int64)
            out("fixed", S, np.int64)
            out("winding", WE.winding_of(S).view(np.uint32), np.uint32)
        exe = os.path.join(d, "winding_host_check")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "include"), "-I", d, "-o", exe,
                               os.path.join(ROOT, "tools", "winding_host_check.cpp")])
        return subprocess.call([exe, d] + list(NAMES))


if __name__ == "__main__":
    sys.exit(main())
