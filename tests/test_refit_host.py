"""The host definition of a refit (ezrt::refitBVH, ezrt_host_refit_nodes, ezrt_amd.refit.refit_nodes) and the declarations of the
device refit (include/ezrt_refit.h) -- no GPU needed.

* Identity: refitting the unchanged triangles of every fixture scene gives the builder's own node arrays, bit for bit.
* On deformed triangles (signed zeros on shared planes, coordinates beyond the builder's +-1145141919 start value, a NaN vertex) the
  C++ refit equals a plain-Python restatement of the fold: glm::min / glm::max from the start value over a leaf's range in index
  order, unions left then right for inner nodes.
"""
import os
import re

import numpy as np
import pytest

from ezrt_amd import _abi, refit, scenes
from ezrt_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START = np.float32(1145141919)


def _bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def _gmin(x, y):
    return y if y < x else x


def _gmax(x, y):
    return y if x < y else x


def _python_refit(tri, nodes):
    """the fold, restated one float at a time (np.float32 scalars: comparisons as in C++, NaN never compares)"""
    out = nodes.copy()
    P = tri[:, :9].reshape(-1, 3, 3)
    for i in range(nodes.shape[0] - 1, 0, -1):
        left, right, n, index = int(nodes[i, 0]), int(nodes[i, 1]), int(nodes[i, 3]), int(nodes[i, 4])
        if n > 0:
            lo = [START] * 3
            hi = [-START] * 3
            for k in range(index, index + n):
                for c in range(3):
                    p1, p2, p3 = P[k, 0, c], P[k, 1, c], P[k, 2, c]
                    lo[c] = _gmin(lo[c], _gmin(p1, _gmin(p2, p3)))
                    hi[c] = _gmax(hi[c], _gmax(p1, _gmax(p2, p3)))
        else:
            lo = [_gmin(out[left, 6 + c], out[right, 6 + c]) for c in range(3)]
            hi = [_gmax(out[left, 9 + c], out[right, 9 + c]) for c in range(3)]
        out[i, 6:9] = lo
        out[i, 9:12] = hi
    return out


def _fixture(name):
    if name == "cornell":
        return scenes.cornell_scene()
    if name == "bunny_sah":
        return scenes.bunny_scene(subdiv=0)
    if name == "bunny_median":
        return scenes.bunny_scene(subdiv=0, sah=False)
    if name == "disney_grid":
        return scenes.disney_grid_scene(subdiv=1)
    if name == "bunny_sub1":
        return scenes.bunny_scene(subdiv=1)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["cornell", "bunny_sah", "bunny_median", "disney_grid", "bunny_sub1"])
def test_identity_refit_gives_the_builders_arrays(name, monkeypatch):
    monkeypatch.setenv("EZRT_GPU_BUILD", "0")  # the host builder: the arrays a GPU-free host makes
    bs = _fixture(name)
    out = refit.refit_nodes(bs.tri, bs.nodes)
    assert _bits_equal(out, bs.nodes), name
    assert _bits_equal(S.refitBVH(bs.tri.ravel(), bs.nodes.ravel()), bs.nodes)  # flat arrays are accepted too


@pytest.mark.parametrize("method", [0, 1])
def test_identity_refit_of_both_builders_on_random_triangles(method):
    rng = np.random.default_rng(3 + method)
    T = np.zeros((700, 36), np.float32)
    c = rng.uniform(-3, 3, (700, 1, 3))
    T[:, :9] = (c + rng.uniform(-0.2, 0.2, (700, 3, 3))).reshape(700, 9)
    T[:, 18:36] = S.Material.disney().to18()
    hs = S.HostScene()
    hs.addTriangles(T)
    (hs.buildBVH if method == 0 else hs.buildBVHwithSAH)(4)
    tri, nodes = hs.encode()
    assert _bits_equal(refit.refit_nodes(tri, nodes), nodes)


def _small_scene(seed, n=160, leaf=4):
    rng = np.random.default_rng(seed)
    T = np.zeros((n, 36), np.float32)
    c = rng.uniform(-2, 2, (n, 1, 3))
    T[:, :9] = (c + rng.uniform(-0.3, 0.3, (n, 3, 3))).reshape(n, 9)
    T[:, 9:18] = np.tile([0, 1, 0], 3)
    T[:, 18:36] = S.Material.disney().to18()
    hs = S.HostScene()
    hs.addTriangles(T)
    hs.buildBVHwithSAH(leaf)
    return hs.encode()


def _deformations(tri, rng):
    out = {}
    P = tri[:, :9].reshape(-1, 3, 3).astype(np.float64)
    t = tri.copy()
    th = 0.7
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    t[:, :9] = (P @ R.T + np.array([0.5, -1.0, 2.0])).reshape(-1, 9)
    out["rigid"] = t
    # signed zeros: snap every vertex near the planes x = 0 / y = 0 onto them, with -0.0 and +0.0 mixed
    t = tri.copy()
    Q = t[:, :9].reshape(-1, 3, 3)
    for ax in (0, 1):
        near = np.abs(Q[:, :, ax]) < 0.6
        Q[:, :, ax][near] = np.where(rng.random(int(near.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    out["signed_zeros"] = t
    # coordinates beyond the start value (the cap of the fold) on a few triangles, both signs
    t = tri.copy()
    Q = t[:, :9].reshape(-1, 3, 3)
    k = rng.choice(Q.shape[0], 9, replace=False)
    Q[k[:3], 0, 0] = np.float32(3.0e9)
    Q[k[3:6], 1, 1] = np.float32(-2.0e9)
    Q[k[6:], :, 2] = np.float32(1.2e9)
    out["beyond_start"] = t
    # a NaN vertex (in first, middle and last vertex position of three triangles)
    t = tri.copy()
    Q = t[:, :9].reshape(-1, 3, 3)
    k = rng.choice(Q.shape[0], 3, replace=False)
    Q[k[0], 0, 0] = np.nan
    Q[k[1], 1, 1] = np.nan
    Q[k[2], 2, :] = np.nan
    out["nan"] = t
    # collapsed to a point
    t = tri.copy()
    Q = t[:, :9].reshape(-1, 3, 3)
    Q[::5] = Q[::5, :1]
    out["collapsed"] = t
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_refit_equals_the_python_fold_on_deformed_triangles(seed):
    tri, nodes = _small_scene(seed)
    rng = np.random.default_rng(100 + seed)
    for what, t in _deformations(tri, rng).items():
        got = refit.refit_nodes(t, nodes)
        want = _python_refit(t, nodes)
        assert _bits_equal(got, want), what
        assert _bits_equal(got[0], nodes[0]), what                        # the sentinel is kept
        assert np.array_equal(got[:, :6].view(np.uint32), nodes[:, :6].view(np.uint32)), what  # topology kept
    # a fold over the whole range: the root of the deformed scene's refit (SAH arrays are index-ordered ranges)
    t = _deformations(tri, rng)["signed_zeros"]
    root = refit.refit_nodes(t, nodes)[1]
    assert _bits_equal(root, _python_refit(t, nodes)[1])


def test_signed_zero_tie_keeps_the_first_operand():
    # two triangles in one leaf and the same two in two leaves: -0.0 first, +0.0 second, on the x = 0 plane
    T = np.zeros((2, 36), np.float32)
    T[0, :9] = [-0.0, 0, 0, -0.0, 1, 0, -0.0, 0, 1]
    T[1, :9] = [0.0, 2, 0, 0.0, 3, 0, 0.0, 2, 1]
    one_leaf = np.zeros((2, 12), np.float32)
    one_leaf[1, 3], one_leaf[1, 4] = 2, 0
    out = refit.refit_nodes(T, one_leaf)
    assert np.signbit(out[1, 6]) and np.signbit(out[1, 9])                # min keeps -0 (first), max keeps -0 (first)
    two_leaves = np.zeros((4, 12), np.float32)
    two_leaves[1, :2] = [2, 3]
    two_leaves[2, 3], two_leaves[2, 4] = 1, 0
    two_leaves[3, 3], two_leaves[3, 4] = 1, 1
    out2 = refit.refit_nodes(T, two_leaves)
    assert _bits_equal(out2[1, 6:], out[1, 6:])                           # the union equals the fold over the range
    assert _bits_equal(out2, _python_refit(T, two_leaves))


def test_refit_rejects_bad_topology():
    T = np.zeros((2, 36), np.float32)
    bad = np.zeros((3, 12), np.float32)
    bad[1, :2] = [1, 2]                                                   # a child that is not below its parent
    with pytest.raises(RuntimeError, match="children"):
        refit.refit_nodes(T, bad)
    bad = np.zeros((2, 12), np.float32)
    bad[1, 3], bad[1, 4] = 3, 0                                           # a leaf range past the triangle array
    with pytest.raises(RuntimeError, match="range"):
        refit.refit_nodes(T, bad)


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ezrt_[a-z0-9_]+)\s*\(", src)))


def test_declarations_match_the_binding_tables():
    assert "ezrt_host_refit_nodes" in _declared("ezrt_scene_c.h")
    assert set(_declared("ezrt_scene_c.h")) == set(_abi.HOST_ABI)
    names = _declared("ezrt_refit.h")
    assert names == ["ezrt_scene_refit_device"]
    assert set(names) == set(_abi.REFIT_ABI)
    assert not set(names) & set(_abi.TRACE_ABI)                           # ezrt.h (and with it the oracle's ABI) is unchanged
    host = _abi.load_host()
    assert host.ezrt_host_refit_nodes.argtypes == _abi.HOST_ABI["ezrt_host_refit_nodes"][1]


def test_hip_library_exports_the_refit_entry_point():
    hip = _abi.load_hip()  # dlopen only
    assert hip.ezrt_scene_refit_device.argtypes == _abi.REFIT_ABI["ezrt_scene_refit_device"][1]
    from ezrt_amd import progressive
    assert callable(progressive.ProgressiveRenderer.set_geometry) and callable(refit.refit)
