"""The sizes of the mesh processing's `work` buffers (ezrt_amd/csrc/hip/ezrt_mesh.hip) against their formulas, written out here.

Each ezrt_*_work_bytes runs its family's one layout function over a null pointer (ezrt_work_carver.h), the same function that cuts
the caller's buffer into the kernels' arrays: a size that moved would be a layout that moved.  The values of n are where the pieces
step -- c(x) = ceil(x / 2048), the tiles of a scan: 3 n passes 2048 at 683 and 4096 at 1366, n at 2049; T, the power of two >=
max(8, 6 n): at 2, 3, 6, 86, 683, 1366; T2, the power of two >= max(8, 2 n): at 5, 2049 -- with odd n for the boundary loops' rounding
and each call's own row limit.  Needs no GPU: the library is only opened, and these functions do no device work."""
import pytest

from ezrt_amd import _abi

I32 = 2 ** 31 - 1
NS = [-1, 0, 1, 2, 3, 5, 6, 85, 86, 682, 683, 1365, 1366, 2047, 2048, 2049, 10 ** 6, 2 ** 24]


def c(x):
    return (x + 2047) // 2048


def r8(x):
    return (x + 7) // 8 * 8


def pow2(least):
    t = 8
    while t < least:
        t *= 2
    return t


def T(n):
    return pow2(6 * n)


def T2(n):
    return pow2(2 * n)


# name -> (the call's row limit, the formula for n >= 1, the arguments behind n)
FAMILIES = {
    "ezrt_topology_work_bytes": (I32 // 3, lambda n: r8(8 * (n + 1) + 8 * T(n) + 36 * n), ()),
    "ezrt_weld_work_bytes": (I32 // 3, lambda n: r8(16 * (3 * n + 1) + 8 * (c(3 * n) + 1) + 4 * T(n) + 72 * n), ()),
    "ezrt_vertex_normals_work_bytes": (I32 // 3, lambda n: r8(12 * n), ()),
    "ezrt_orient_work_bytes": (I32 // 3, lambda n: 32 * n + 8 * c(n) + 24, ()),
    "ezrt_boundary_work_bytes": (I32 // 3, lambda n: 132 * n + 4 * (n & 1) + 8 * c(3 * n) + 56, ()),
    "ezrt_clip_work_bytes": (I32 // 2, lambda n: 8 * c(n) + 8, ()),
    "ezrt_subdivide_work_bytes": (I32 // 12, lambda n: 48 * n + 8, (_abi.SUBDIVIDE_LOOP,)),
    "ezrt_subdivide_work_bytes/midpoint": (I32 // 12, lambda n: 8, (_abi.SUBDIVIDE_MIDPOINT,)),
    "ezrt_decimate_work_bytes": (I32 // 3, lambda n: 40 * n + 8 * c(3 * n) + 64 * T(n) + 4 * T2(n) + 16, ()),
}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_work_bytes_equal_the_formula(name):
    limit, formula, rest = FAMILIES[name]
    f = getattr(_abi.load_hip(), name.split("/")[0])                          # dlopen only
    ns = NS + [limit]
    got = [f(n, *rest) for n in ns]
    assert got == [f(n, *rest) for n in ns]                                   # pure
    assert got == [formula(n) if n >= 1 else 8 for n in ns]
    assert all(g % 8 == 0 and g >= 8 for g in got)
    assert all(b >= a for a, b in zip(got, got[1:]))                          # monotone: NS ascends, and the limit is its largest


def test_every_work_bytes_of_the_mesh_unit_is_covered():
    names = {k for t in dir(_abi) if t.endswith("_ABI") and isinstance(getattr(_abi, t), dict) for k in getattr(_abi, t) if k.endswith("_work_bytes")}
    assert names - {"ezrt_plane_loops_work_bytes"} == {k.split("/")[0] for k in FAMILIES} and len(names) == 9
    assert all(limit > NS[-1] for limit, _, _ in FAMILIES.values())
