"""Stream-ordered mesh smoothing on device tensors (include/ezrt_smooth.h): `query.smooth_rows`, which is where callers find it.

    fair = query.smooth_rows(scene, tri36, topo, weld, steps=6, lam=0.5, mu=-0.53)

The wrapper goes through the one call path of query.py (`_scene_lib`, `_OnStream`, its `scratch`, `call` and `done`) and lives in a
module of its own: query.py's own functions and named tuples are a pinned list (tests/test_python_api.py)."""
import collections
import math

import torch

from . import _abi

SmoothRows = collections.namedtuple("SmoothRows", "rows summary n_rows")


def smooth_rows(scene, tri36, topo, weld, steps=1, lam=0.5, mu=None, pin_border=False, out=None, tile_rows=0, stream=None):
    """SmoothRows(rows float32 [n, 36], summary int64 [8], n_rows int): the caller's triangle rows `tri36` (a contiguous float32
    [n, 36] GPU tensor: p1 p2 p3, n1 n2 n3, material -- the rows a scene is made of) after `steps` relaxation steps: every vertex
    moves towards the mean of its neighbours, x + w (mean - x), with w = lam in even steps and mu in odd ones.  mu=None means mu = lam,
    the plain umbrella operator, which shrinks a closed mesh; lam=0.5, mu=-0.53 is Taubin's pair, which largely does not.  Interior
    vertices average over their star, border vertices over their two border neighbours (pin_border=True keeps them where they are),
    vertices on a non-manifold edge or pinched stay.  Every row keeps its winding and its material and gets its face normal at all
    three corners (for smooth ones: a scene of `rows`, mesh_weld, vertex_normals).  It requires `topo`, a MeshTopology, and `weld`, a
    MeshWeld made with flags=True, of a scene of these rows (or any objects with edge_class and vertex, star_offsets, star,
    vert_flags); both are taken by value and still describe the output.  out=None allocates the result; out=tri36 smooths in place;
    any other contiguous float32 [n, 36] tensor of the same device that does not overlap tri36 is written and returned.  tile_rows picks
    the route of the steps (0: the library's choice; rows up to _abi.smooth_limits() can run all steps in LDS, in one launch): it
    changes the time, never the answer.  summary is [n, corners smoothed, corners on a border, corners kept, active vertices, steps,
    flags, 0], and all zero for n = 0, where nothing is launched.  `scene` supplies the library and the device only.  Does not synchronise.  MEMORY besides the result: the library's
    scratch, ezrt_smooth_work_bytes(n) -- about 135 B per row -- freed to torch's allocator when the stream is done with it.  The
    definition: include/ezrt_smooth.h."""
    from .query import _OnStream, _scene_lib, _tensor, _weld_array   # (query imports this module at its end)
    lib = _scene_lib(scene, {**_abi.SMOOTH_ABI, **_abi.SMOOTH_SIZES})
    _tensor("tri36", tri36, torch.float32, last=36)
    if tri36.dim() != 2:
        raise ValueError("tri36 must have shape [n, 36], not %s" % (tuple(tri36.shape),))
    n = tri36.shape[0]
    if n > (2**31 - 1) // 3:
        raise ValueError("at most (2^31 - 1) / 3 rows per call")
    if not isinstance(steps, int) or isinstance(steps, bool) or not 1 <= steps <= _abi.SMOOTH_STEPS_MAX:
        raise ValueError("steps must be an int in 1 .. %d" % _abi.SMOOTH_STEPS_MAX)
    lam = float(lam)
    mu = lam if mu is None else float(mu)
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError("lam and mu must be finite")
    if not isinstance(tile_rows, int) or isinstance(tile_rows, bool) or tile_rows < 0 or tile_rows > 2**31 - 1:
        raise ValueError("tile_rows must be an int >= 0")
    dev = tri36.device
    if out is not None and out is not tri36:
        _tensor("out", out, torch.float32, shape=(n, 36), device=dev)
        a0, b0 = tri36.data_ptr(), out.data_ptr()
        if a0 != b0 and a0 < b0 + 144 * n and b0 < a0 + 144 * n:
            raise ValueError("out must be tri36 itself or must not overlap it")
    if topo is None or weld is None or getattr(weld, "vert_flags", None) is None:
        raise ValueError("smooth_rows needs topo, a MeshTopology, and weld, a MeshWeld made with flags=True")
    q = _OnStream(scene, tri36, stream)
    cls = _tensor("topo.edge_class", topo.edge_class, torch.uint8, device=dev)
    if cls.numel() != 3 * n:
        raise ValueError("topo.edge_class must have 3 * n = %d entries, not %d" % (3 * n, cls.numel()))
    vertex = _weld_array("weld.vertex", weld.vertex, 3 * n, dev, q)
    if vertex.numel() != 3 * n:
        raise ValueError("weld.vertex must have 3 * n = %d entries, not %d" % (3 * n, vertex.numel()))
    offsets = _weld_array("weld.star_offsets", weld.star_offsets, 3 * n + 1, dev, q)
    star = _weld_array("weld.star", weld.star, 3 * n, dev, q)
    vflags = _weld_array("weld.vert_flags", weld.vert_flags, 3 * n, dev, q, torch.uint8)
    flags = _abi.SMOOTH_PIN_BORDER if pin_border else 0
    work_bytes = int(lib.ezrt_smooth_work_bytes(n))
    work, summary = q.scratch(dev, work_bytes)
    rows = out if out is not None else torch.empty((n, 36), dtype=torch.float32, device=dev)
    if n > 0:                                                        # (no rows: the C call writes nothing, and the summary stays zero)
        q.call(lib.ezrt_smooth_rows_device, tri36, n, cls, vertex, offsets, star, vflags, steps, lam, mu, flags, tile_rows, rows, summary, work,
               work_bytes)
    q.done(tri36, rows, summary, cls, vertex, offsets, star, vflags)
    return SmoothRows(rows, summary, n)
