"""The three device builders (include/ezrt_build.h) on degenerate input: tests/build_edge_scenes.py's cases, which
tests/test_build_edge_scenes.py holds against their own claims on the CPU.  Every comparison is on the bits.

* `ezrt_build_sah` and `ezrt_build_median` equal the host builder (HostScene.buildBVHwithSAH / buildBVH + encode) -- triangles,
  nodes, shape -- on every case without NaN centroids: any depth (`dup_chain` and `line` peel one triangle per level; `dup_chain`
  is 4193 levels deep, beyond the 4096 the SAH builder once stopped at while reporting success), +-0, subnormals, +-inf, coordinates
  beyond the INF = 114514 cost cap and beyond new_node's start value 1145141919, and the sizes where rocPRIM's sorts and scans
  change shape.
* `ezrt_build_lbvh` keeps its own contract on all of them and with NaN vertices: a well-formed tree with exact boxes
  (tests/test_gpu_lbvh.py's `_check_tree`), GPU trace == CPU oracle on the same arrays, and == brute force where rays can hit.
* Each builder gives the same bits when called again, also after a build of another size.
* The C ABI's error paths, which `build._build` (capacity 2 n always) never reaches.

Measured on an MI355X (each build prints its device ms and wall time): the SAH builder on `dup_chain`, 4200 triangles and 4193
levels, takes 1.49 s on the device and 1.71 s wall (leaf_n = 1, 4200 levels: 1.48 s); the whole file 11 s.  DESIGN.md section 8,
"The device builders on degenerate input"."""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import build_edge_scenes as B  # noqa: E402
from test_gpu_lbvh import _check_tree  # noqa: E402

from ezrt_amd import _abi, build  # noqa: E402
from ezrt_amd import scene as S  # noqa: E402

pytestmark = pytest.mark.gpu

EZRT_ERR_INVALID, EZRT_ERR_UNSUPPORTED = -1, -3        # include/ezrt.h
ENTRIES = ("ezrt_build_sah", "ezrt_build_median", "ezrt_build_lbvh")
PARITY = {"sah": (build.build_sah, True), "median": (build.build_median, False)}
N_RAYS = 600
# GPU == oracle only: their triangles cannot be hit, or the brute-force pointer tree is not their reference
ORACLE_ONLY = ("inf", "overflow_centroid", "nan_vertex", "dup_chain", "line", "near_flt_max")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _host(name, sah, leaf_n):
    """the reference arrays: computed once per (case, builder, leaf size), read-only"""
    hs = S.HostScene()
    hs.addTriangles(B.case(name))
    (hs.buildBVHwithSAH if sah else hs.buildBVH)(leaf_n)
    tri, nodes = hs.encode()
    tri.setflags(write=False)
    nodes.setflags(write=False)
    return tri, nodes


@functools.lru_cache(maxsize=None)
def _rays(name):
    r = B.rays_at(B.case(name), N_RAYS, B.SEED)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _brute(name):
    """chapter 2's brute force over the whole array: (vertices of the hit triangle [n, 9], hit mask, t)"""
    tri9, idx, t = S.p2Query(B.case(name)[:, :9], _rays(name), use_bvh=False)
    return tri9[np.maximum(idx, 0)], idx >= 0, t


def _assert_equals_host(builder, name, leaf_n):
    fn, sah = PARITY[builder]
    tri_h, nodes_h = _host(name, sah, leaf_n)
    t0 = time.time()
    tri_g, nodes_g, ms = fn(B.case(name), leaf_n)
    wall = time.time() - t0
    print("%s %s leaf_n %d: %d triangles, %d nodes (host %d), device %.1f ms, wall %.2f s"
          % (builder, name, leaf_n, tri_g.shape[0], nodes_g.shape[0], nodes_h.shape[0], ms, wall))
    assert tri_g.shape == tri_h.shape and np.array_equal(_bits(tri_g), _bits(tri_h))
    assert nodes_g.shape == nodes_h.shape and np.array_equal(_bits(nodes_g), _bits(nodes_h))


@pytest.mark.parametrize("leaf_n", [8, 1])
@pytest.mark.parametrize("builder", ["sah", "median"])
@pytest.mark.parametrize("name", B.PARITY_NAMES)
def test_sah_and_median_equal_the_host_builder(hip, name, builder, leaf_n):
    """`dup_chain` with the SAH builder is the regression test of the level cap: 4193 (leaf 8) and 4200 (leaf 1) levels"""
    _assert_equals_host(builder, name, leaf_n)


@pytest.mark.parametrize("builder", ["sah", "median"])
@pytest.mark.parametrize("name,leaf_n", [("size_9", 2), ("size_9", 8), ("size_9", 9), ("size_9", 14), ("flat", 128)])
def test_leaf_sizes_around_the_triangle_count(hip, name, builder, leaf_n):
    """9 triangles at leaf_n = 2, n - 1 (a root with two leaves), n and n + 5 (the root is a leaf); 128 on `flat`"""
    _assert_equals_host(builder, name, leaf_n)
    if name == "size_9" and leaf_n >= 8:               # (sentinel included)
        assert _host(name, PARITY[builder][1], leaf_n)[1].shape[0] == {8: 4, 9: 2, 14: 2}[leaf_n]


@pytest.mark.parametrize("leaf_n", [8, 1, 128])
@pytest.mark.parametrize("name", B.ALL_NAMES)
def test_lbvh_keeps_its_contract(hip, oracle, name, leaf_n):
    T = B.case(name)
    tri, nodes, ms = build.build_lbvh(T, leaf_n)
    if name == "nan_vertex":       # NaN coordinates do not enter the boxes: the minNum / maxNum fold
        _check_tree(T, tri, nodes, leaf_n, np.fmin, np.fmax)
        assert not np.isnan(nodes[:, 6:12]).any()
    else:
        _check_tree(T, tri, nodes, leaf_n)
    rays = _rays(name)
    tg, dg = hip.scene_create(tri, nodes).query_hits(rays)
    to, do = oracle.scene_create(tri, nodes).query_hits(rays)
    hit = tg >= 0
    print("lbvh %s leaf_n %d: %d nodes, device %.2f ms, %d of %d rays hit" % (name, leaf_n, nodes.shape[0], ms, hit.sum(), N_RAYS))
    assert np.array_equal(tg, to) and np.array_equal(_bits(dg), _bits(do))
    if name in ORACLE_ONLY or name not in B.HITTABLE:
        return
    tri9_b, hit_b, t_b = _brute(name)
    floor = int(hit_b.sum())                            # the floor is the brute-force count itself
    assert (floor == 0) if name in B.UNHITTABLE else (floor > 0)
    assert np.array_equal(hit, hit_b) and int(hit.sum()) == floor
    assert np.array_equal(_bits(dg[hit]), _bits(t_b[hit]))
    if name not in ("flat", "signed0") and not name.startswith("ties_"):
        # the same triangle, by its vertices -- not in one plane or on the half-integer grids, where distinct coplanar triangles
        # overlap and which of two hits at the very same t is reported depends on the order of the walk
        assert np.array_equal(_bits(tri[tg[hit], :9]), _bits(tri9_b[hit]))


@pytest.mark.parametrize("entry", ["build_sah", "build_median", "build_lbvh"])
def test_builds_are_deterministic(hip, entry):
    fn = getattr(build, entry)
    T = B.case("signed0")
    tri_a, nodes_a, _ = fn(T, 8)
    tri_b, nodes_b, _ = fn(T, 8)
    fn(B.case("size_1025"), 8)                          # a build of another size in between
    tri_c, nodes_c, _ = fn(T, 8)
    for tri, nodes in ((tri_b, nodes_b), (tri_c, nodes_c)):
        assert np.array_equal(_bits(tri), _bits(tri_a))
        assert nodes.shape == nodes_a.shape and np.array_equal(_bits(nodes), _bits(nodes_a))


# ---- the C ABI, called directly
CANARY = np.uint32(0xDEADBEEF)


class _Call:
    """one entry point with its buffers for 9 triangles; call(**overrides) -> return code"""

    def __init__(self, entry):
        self.lib = _abi.load_hip()
        self.fn = getattr(self.lib, entry)
        self.tri = np.array(B.case("size_9"))
        self.n = self.tri.shape[0]
        self.tri_out = np.zeros_like(self.tri)
        self.cap = 2 * self.n
        self.nodes = np.zeros((self.cap + 8, 12), np.float32)
        self.n_nodes = C.c_int(0)
        self.ms = C.c_float(0.0)

    def call(self, leaf_n=8, **kw):
        fp = lambda a: a.ctypes.data_as(_abi.c_float_p)
        self.nodes.view(np.uint32)[:] = CANARY
        self.n_nodes.value = -7
        a = dict(tri=fp(self.tri), n_tri=self.n, tri_out=fp(self.tri_out), nodes_out=fp(self.nodes), cap=self.cap,
                 n_nodes=C.byref(self.n_nodes), ms=C.byref(self.ms))
        a.update(kw)
        return self.fn(a["tri"], a["n_tri"], leaf_n, a["tri_out"], a["nodes_out"], a["cap"], a["n_nodes"], a["ms"])

    def error(self):
        return self.lib.ezrt_last_error().decode()

    def good_build(self, leaf_n=1):
        """a normal build after an error: (tri, nodes)"""
        assert self.call(leaf_n) == 0, self.error()
        m = self.n_nodes.value
        assert 2 <= m <= self.cap and np.all(self.nodes.view(np.uint32)[m:] == CANARY)
        return self.tri_out.copy(), self.nodes[:m].copy()


def _assert_still_builds(c, entry):
    tri, nodes = c.good_build(1)
    if entry == "ezrt_build_lbvh":
        _check_tree(c.tri, tri, nodes, 1)
        t2, n2, _ = build.build_lbvh(c.tri, 1)
        assert np.array_equal(_bits(tri), _bits(t2)) and np.array_equal(_bits(nodes), _bits(n2))
    else:
        tri_h, nodes_h = _host("size_9", entry == "ezrt_build_sah", 1)
        assert np.array_equal(_bits(tri), _bits(tri_h))
        assert nodes.shape == nodes_h.shape and np.array_equal(_bits(nodes), _bits(nodes_h))


@pytest.mark.parametrize("entry", ENTRIES)
def test_abi_capacity_one_short_is_refused_and_nothing_is_written_past_it(hip, entry):
    c = _Call(entry)
    _, nodes = c.good_build(1)
    need = nodes.shape[0]
    assert need == 2 * c.n                              # leaf_n = 1: 2 n - 1 nodes and the sentinel
    assert c.call(1, cap=need - 1) == EZRT_ERR_INVALID
    assert "nodes_capacity" in c.error()
    assert np.all(c.nodes.view(np.uint32)[need - 1:] == CANARY)        # nothing past nodes_capacity records
    assert c.call(1, cap=need) == 0 and c.n_nodes.value == need        # exactly enough is enough
    _assert_still_builds(c, entry)


@pytest.mark.parametrize("entry", ENTRIES)
def test_abi_bad_arguments(hip, entry):
    c = _Call(entry)
    null_f = C.cast(None, _abi.c_float_p)
    bad = [dict(n_tri=0), dict(n_tri=-3), dict(leaf_n=0), dict(leaf_n=-1), dict(tri=null_f), dict(tri_out=null_f),
           dict(nodes_out=null_f), dict(n_nodes=C.cast(None, C.POINTER(C.c_int)))]
    if entry == "ezrt_build_lbvh":
        bad.append(dict(leaf_n=129))
    for kw in bad:
        assert c.call(**kw) == EZRT_ERR_INVALID, kw
        assert c.error()
        assert np.all(c.nodes.view(np.uint32) == CANARY), kw
        _assert_still_builds(c, entry)
    assert c.call(ms=C.cast(None, _abi.c_float_p)) == 0                 # build_ms is optional
    # 2^24 triangles: refused before anything is allocated or read (the buffers are the small ones)
    assert c.call(n_tri=1 << 24) == EZRT_ERR_UNSUPPORTED
    assert "2^24" in c.error() and np.all(c.nodes.view(np.uint32) == CANARY)
    _assert_still_builds(c, entry)
    if entry != "ezrt_build_lbvh":                       # leaf_n = 129 is legal for the parity builders: the root is a leaf
        assert c.call(129) == 0 and c.n_nodes.value == 2
