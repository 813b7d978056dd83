"""Stream-ordered ray and point queries on device tensors (include/ezrt_query.h, include/ezrt_surface.h, include/ezrt_multihit.h,
include/ezrt_closest_point.h, include/ezrt_nearest.h, include/ezrt_inside.h, include/ezrt_box_overlap.h,
include/ezrt_tri_overlap.h, include/ezrt_self_overlap.h, include/ezrt_tri_distance.h, include/ezrt_sphere_cast.h,
include/ezrt_segment.h, include/ezrt_obb_overlap.h, include/ezrt_winding.h, include/ezrt_plane.h, include/ezrt_plane_loops.h,
include/ezrt_overlap_list.h, include/ezrt_topology.h, include/ezrt_vertices.h, include/ezrt_orient.h, include/ezrt_boundary.h,
include/ezrt_clip.h, include/ezrt_subdivide.h, include/ezrt_smooth.h).

    tri, t = query.closest(scene, rays)               # the reference's closest hit of every ray
    tri, t = query.closest(scene, rays, t_max)        # ... if it lies below t_max, else a miss
    hit = query.occluded(scene, rays, t_max)          # is anything in the way before t_max?  (bool)
    tri, t, point, normal, inside = query.surface(scene, rays)   # closest hit + hit point, shading normal, side (include/ezrt_surface.h)
    tri, t, count = query.all_hits(scene, rays, max_hits)        # every triangle the ray crosses, nearest first (include/ezrt_multihit.h)
    point, normal, inside = query.surface_at(scene, rays, tri, t)   # the surface attributes of hits already held: every layer's
    tri, point, dist, bary = query.closest_point(scene, points)  # the nearest triangle, point and distance (include/ezrt_closest_point.h)
    tri, dist, count = query.nearest(scene, points, k, d_max, count=True)   # the k nearest triangles in order, and how many lie within d_max
    tri, point, dist, bary = query.closest_point_at(scene, points, tri)     # ... their nearest points and barycentrics (include/ezrt_nearest.h)
    inside = query.inside(scene, points, axis=0)                 # is the point inside the mesh?  (bool; include/ezrt_inside.h)
    inside, crossings = query.inside(scene, points, axis, crossings=True)   # ... and the number of triangles its axis ray crosses
    tri, point, dist, bary, inside = query.signed_distance(scene, points)   # closest_point with dist negative inside the mesh
    tri, n_overlap = query.box_overlap(scene, lo, hi, max_k=8)   # the triangles each box [lo, hi] touches (include/ezrt_box_overlap.h)
    touches = query.box_overlap_at(scene, lo, hi, tri)           # ... the same test for pairs already held  (bool)
    tri, n_overlap = query.tri_overlap(scene, tris, max_k=8)     # the triangles each triangle crosses (include/ezrt_tri_overlap.h)
    crosses = query.tri_overlap_at(scene, tris, tri)             # ... the same test for pairs already held  (bool)
    tri, n_overlap = query.self_overlap(scene, max_k=8)          # where the mesh crosses itself (include/ezrt_self_overlap.h)
    crosses = query.self_overlap_at(scene, a, b)                 # ... the same test for pairs of triangle ids already held  (bool)
    tri, dist, point_query, point_scene, crosses = query.tri_distance(scene, tris, d_max)   # how close each triangle comes to the mesh
    tri, dist, point_query, point_scene, crosses = query.tri_distance_at(scene, tris, tri)  # ... for pairs already held (include/ezrt_tri_distance.h)
    tri, t, point, touching = query.sphere_cast(scene, rays, radius, t_max)   # first contact of a sphere moving along each ray
    tri, t, point, touching = query.sphere_cast_at(scene, rays, radius, tri)  # ... for pairs already held (include/ezrt_sphere_cast.h)
    tri, dist, point_query, point_scene, crosses = query.segment_distance(scene, segs, d_max)   # how close each segment comes to the mesh
    tri, dist, point_query, point_scene, crosses = query.segment_distance_at(scene, segs, tri)  # ... for pairs already held
    tri, n_overlap = query.capsule_overlap(scene, segs, radius, max_k=8)      # the triangles each capsule touches (include/ezrt_segment.h)
    tri, n_overlap = query.obb_overlap(scene, centre, axes, max_k=8)          # the triangles each rotated box touches (include/ezrt_obb_overlap.h)
    touches = query.obb_overlap_at(scene, centre, axes, tri)                  # ... the same test for pairs already held  (bool)
    w = query.winding_number(scene, points)                                   # how often the mesh wraps each point: 1 inside, 0 outside
    w, fixed = query.winding_number(scene, points, fixed=True)                # ... and the exact int64 sum behind it (include/ezrt_winding.h)
    w, fixed = query.winding_number_at(scene, points, tri)                    # ... the term of single triangles, for pairs already held
    n_cross = query.plane_count(scene, planes)                                # how many triangles each plane a x + b y + c z = d crosses
    offsets, tri, seg = query.plane_section(scene, planes)                    # ... and all of them with their segments, CSR (include/ezrt_plane.h)
    crosses, side, seg = query.plane_section_at(scene, planes, tri)           # ... the same rule for pairs already held
    plane_loops, loop_offsets, closed, row, tri, seg = query.plane_loops(scene, planes)   # ... chained into polylines (include/ezrt_plane_loops.h)
    loops = query.plane_loops_of(scene, offsets, seg)                         # ... for a section already held: next, order, CSR of the loops
    length, area = query.loop_measures(loops, planes)                         # ... perimeter and signed area of every loop (float64)
    offsets, tri, n_found = query.box_overlap_list(scene, lo, hi)             # EVERY triangle each box touches, CSR (include/ezrt_overlap_list.h)
    ... and obb_overlap_list, tri_overlap_list, self_overlap_list, capsule_overlap_list: the inputs of the max_k call, all ids
    topo = query.mesh_topology(scene)                                         # twins, edge classes, components; topo.closed, topo.oriented
    shared, opposite = query.mesh_topology_at(scene, tri_a, edge_a, tri_b)    # ... the same rule for pairs already held (include/ezrt_topology.h)
    weld = query.mesh_weld(scene)                                             # the indexed mesh: vertex of every corner, stars, fans, flags
    same = query.mesh_weld_at(scene, corner_a, corner_b)                      # ... the same rule for pairs already held (include/ezrt_vertices.h)
    tri36 = query.vertex_normals(scene, tri36, weld)                          # smooth normals of moved rows, into floats 9-17, before a refit
    positions, faces = query.indexed_mesh(weld, tri36)                        # ... what every other tool takes
    chi = query.euler_characteristic(weld, topo)                              # V - E + F
    orient = query.mesh_orient(scene, topo)                                   # which triangles to reverse, patches, signed volumes
    tri36 = query.rewind(scene, tri36, orient)                                # ... reverse the marked rows, before a refit (include/ezrt_orient.h)
    volume = query.patch_volume(orient)                                       # ... the signed volume of every patch (float64)
    boundary = query.mesh_boundary(scene, topo)                               # the holes of the mesh as ordered loops of half-edges
    points = query.boundary_points(boundary, tri36)                           # ... their points in order; query.loop_area(boundary) their area vectors
    cap = query.cap_rows(scene, tri36, boundary)                              # ... the triangles that close them (include/ezrt_boundary.h)
    clip = query.clip_rows(scene, tri36, plane)                               # the rows of tri36 on the side a x + b y + c z >= d of a plane
    seg = query.cut_segments(clip)                                            # ... the edges the cut made, start to end (include/ezrt_clip.h)
    sub = query.subdivide_rows(scene, tri36, "loop", topo, weld)              # four rows per row, by midpoints or Loop's scheme (include/ezrt_subdivide.h)
    fair = query.smooth_rows(scene, tri36, topo, weld, steps=6, lam=0.5, mu=-0.53)   # Laplacian / Taubin fairing, many steps in one call (include/ezrt_smooth.h)

`scene` is a `trace.Scene` of the HIP library, `rays` a contiguous float32 GPU tensor of shape [..., 6] (origin, direction) and
`t_max` (optional) a float32 GPU tensor of shape rays.shape[:-1]; `points` is a contiguous float32 GPU tensor of shape [..., 3] and
`d_max` (optional) a float32 GPU tensor of shape points.shape[:-1] (tris.shape[:-1] for `tri_distance`); `lo` and `hi` are contiguous float32 GPU tensors of one shape
[..., 3], the corners of axis-aligned boxes; `tris` is a contiguous float32 GPU tensor of shape [..., 9] (p1 p2 p3).  The outputs
keep the leading dimensions.  The work is enqueued on
`stream` (a torch.cuda.Stream or a raw hipStream_t handle; default: the current stream of the rays' device) and the functions
return without waiting for it.  `axis` (0..5: +x, -x, +y, -y, +z, -z) is the direction of the ray whose crossings decide `inside`;
on a closed mesh every axis gives the same answer, on an open one (the Bunny has holes) they may differ: vote over several.
There is no t_min: a triangle is accepted at t >= 0.0005 only, so a ray leaving a surface needs its
origin offset by the caller.  A miss is (-1, 114514.0): ezrt_query_hits' miss (the reference's INF).
`sphere_cast` is not the reference's rule: `radius` is a float32 GPU tensor of shape rays.shape[:-1] in world units, the direction
need not have unit length and t is in units of it (the centre at time t is o + d*t), a contact is accepted from t = 0 on, and a
miss is the point queries' (-1, +inf, zeros, False).
`segs` is a contiguous float32 GPU tensor of shape [..., 6] that holds THE TWO END POINTS a, b of every segment -- not an origin and a
direction, as every `rays` above does: the segment of a ray up to t is (o, o + d*t).
`centre` is a contiguous float32 GPU tensor of shape [..., 3] and `axes` one of shape [..., 3, 3] whose rows are the three HALF-axis
vectors u0 u1 u2 of the box c + s0 u0 + s1 u1 + s2 u2, |s_j| <= 1; they need not be unit or orthogonal.
"""
import collections

import torch

from . import _abi, trace


Surface = collections.namedtuple("Surface", "tri t point normal inside")
ClosestPoint = collections.namedtuple("ClosestPoint", "tri point dist bary")
Nearest = collections.namedtuple("Nearest", "tri dist count")
SignedDistance = collections.namedtuple("SignedDistance", "tri point dist bary inside")
BoxOverlap = collections.namedtuple("BoxOverlap", "tri n_overlap")
TriOverlap = collections.namedtuple("TriOverlap", "tri n_overlap")
SelfOverlap = collections.namedtuple("SelfOverlap", "tri n_overlap")
TriDistance = collections.namedtuple("TriDistance", "tri dist point_query point_scene crosses")
SphereCast = collections.namedtuple("SphereCast", "tri t point touching")
SegmentDistance = collections.namedtuple("SegmentDistance", "tri dist point_query point_scene crosses")
CapsuleOverlap = collections.namedtuple("CapsuleOverlap", "tri n_overlap")
ObbOverlap = collections.namedtuple("ObbOverlap", "tri n_overlap")
OverlapList = collections.namedtuple("OverlapList", "offsets tri n_found")
PlaneLoops = collections.namedtuple("PlaneLoops", "plane_loops loop_offsets closed row tri seg")
PlaneLoopsOf = collections.namedtuple("PlaneLoopsOf", "next order plane_loops loop_offsets closed")
MeshTopology = collections.namedtuple("MeshTopology", "twin edge_class neighbours mult root component comp_root comp_size comp_flags summary closed oriented")
MeshWeld = collections.namedtuple("MeshWeld", "vertex vert_corner star_offsets star fans vert_flags summary n_vert manifold_vertices")
MeshOrient = collections.namedtuple("MeshOrient", "flip patch_root patch proot psize pflags vol6 summary n_patch orientable scale")
MeshBoundary = collections.namedtuple("MeshBoundary", "next loop pos order loop_offsets lflags area2 summary n_boundary n_loops closed scale")
ClipRows = collections.namedtuple("ClipRows", "rows src cut_edge summary n_rows")
SubdivRows = collections.namedtuple("SubdivRows", "rows summary n_rows")
DecimatedRows = collections.namedtuple("DecimatedRows", "rows src cell cell_point summary n_rows")
IsoRows = collections.namedtuple("IsoRows", "rows cell summary shape")


def _scene_lib(scene, abi):
    """The library of an open scene of the HIP product, with the entry points of `abi` declared."""
    if not isinstance(scene, trace.Scene) or not scene._h:
        raise TypeError("scene must be an open trace.Scene")
    lib = scene._tl.lib
    try:
        if not scene._tl.backend().startswith("hip:"):
            raise AttributeError
        _abi._declare(lib, abi)
    except AttributeError:
        raise TypeError("device queries need a scene of the HIP library (backend %r)" % scene._tl.backend()) from None
    return lib


def _check(scene, rays, t_max):
    lib = _scene_lib(scene, _abi.QUERY_ABI)
    return lib, _check_rays(rays, t_max)


def _tensor(name, x, dtype, shape=None, last=None, device=None, max_numel=None):
    """x, after the checks every entry point makes of a tensor operand, in this order: a GPU tensor, of `dtype`, on `device`, of
    `shape` or with `last` as its last dimension, contiguous, of at most `max_numel` elements.  (shade.py and path.py use it too.)"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise TypeError("%s must be a GPU tensor" % name)
    if x.dtype != dtype:
        raise TypeError("%s must be %s, not %s" % (name, str(dtype).replace("torch.", ""), x.dtype))
    if device is not None and x.device != device:
        raise ValueError("%s is on %s, not on %s" % (name, x.device, device))
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, not %s" % (name, tuple(shape), tuple(x.shape)))
    if last is not None and (x.dim() < 1 or x.shape[-1] != last):
        raise ValueError("%s must have shape [..., %d], not %s" % (name, last, tuple(x.shape)))
    if not x.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if max_numel is not None and x.numel() > max_numel:
        raise ValueError("at most 2^31 - 1 floats per tensor and call")
    return x


def _count(x, width, what):
    """The number of rows of `width` numbers in x: what the C ABI takes as an int."""
    n = x.numel() // width
    if n > 2**31 - 1:
        raise ValueError("at most 2^31 - 1 %s per call" % what)
    return n


def _check_rays(rays, t_max):
    """The number of rays, after the checks every query makes of its rays and t_max."""
    _tensor("rays", rays, torch.float32, last=6)
    if t_max is not None:
        _tensor("t_max", t_max, torch.float32, rays.shape[:-1], device=rays.device)
    return _count(rays, 6, "rays")


def _row_shape(tri, lead):
    """tri.shape, which must be `lead` -- one entry per ray, point or box -- or `lead` and one trailing dimension more: a row each."""
    shape = tuple(tri.shape)
    if shape != lead and shape[:-1] != lead:
        raise ValueError("tri must have shape %s or %s, not %s" % (lead, lead + ("K",), shape))
    return shape


class _OnStream:
    """The stream one device call of `scene` runs on, and the one path from Python into the library (shade.py and path.py use it
    too).  `like` is a tensor of the call, or its torch.device; `stream` is None (the device's current stream), a torch.cuda.Stream
    or a raw hipStream_t handle.  `h` is the raw handle and `stream` a torch stream object in every case.  The rule for memory, the
    same for the three kinds of stream: a tensor the wrapper allocates and does not return is allocated inside `on()`, so its block
    belongs to the call's stream; a tensor it returns, or was given, is allocated on the current stream and recorded by `done`."""
    __slots__ = ("scene", "h", "stream", "side", "kept")

    def __init__(self, scene, like, stream):
        dev = like if isinstance(like, torch.device) else like.device
        cur = torch.cuda.current_stream(dev)
        if stream is None:
            own, h = cur, cur.cuda_stream
        elif isinstance(stream, torch.cuda.Stream):
            own, h = stream, stream.cuda_stream
        else:
            h = int(stream)
            own = torch.cuda.ExternalStream(h, device=dev)
        self.scene, self.h, self.stream, self.side, self.kept = scene, h, own, own != cur, []

    def on(self):
        """The context in which torch allocates, gathers and reads on the call's stream."""
        return torch.cuda.stream(self.stream)

    def call(self, fn, *args):
        """fn(scene handle, *args, stream handle), a TraceError unless it returns 0.  A tensor goes in as its data_ptr() (every
        pointer parameter of _abi.py is a c_void_p, which takes an int or None) and is remembered for `done`; all else as it is."""
        a = []
        for x in args:
            if isinstance(x, torch.Tensor):
                self.kept.append(x)
                x = x.data_ptr()
            a.append(x)
        rc = fn(self.scene._h, *a, self.h)
        if rc != 0:
            raise trace.TraceError("%s (rc=%d)" % (self.scene._tl.lib.ezrt_last_error().decode(), rc))

    def done(self, *extra):
        """The closing step: the caching allocator must not hand out the blocks of the tensors the calls were given, nor of
        `extra`, before the call's stream is done with them."""
        if self.side:
            for x in self.kept + [x for x in extra if x is not None]:
                x.record_stream(self.stream)
        self.kept = []

    def run(self, fn, *args):
        """A wrapper's only library call: `call`, then `done`."""
        self.call(fn, *args)
        self.done()

    def scratch(self, dev, work_bytes, summary=True):
        """(work, summary) of a mesh call: the library's scratch of `work_bytes` (from its own *_work_bytes) as int64 words and the
        eight int64 of its summary, zeroed -- both on the call's stream, so the scratch goes back to torch's allocator when that
        stream is done with it."""
        with self.on():
            work = torch.empty((work_bytes // 8,), dtype=torch.int64, device=dev)
            return work, torch.zeros((8,), dtype=torch.int64, device=dev) if summary else None


def _per_entry(x, lead, shape, q):
    """x [lead + (w,)] as one operand per entry of tri [shape]: x itself, or where a row has entries of its own a copy that repeats
    x's row for each of them, made on the query's own stream."""
    if shape == lead:
        return x
    with q.on():
        return x.unsqueeze(-2).expand(lead + (shape[-1], x.shape[-1])).contiguous()


def _pairs(scene, fn, operands, tri, outs, stream):
    """The call of an `_at` function, fn(operands..., tri, n, outputs...): tri [lead] or [lead + (K,)] checked against the first
    operand, every operand [lead + (w,)] expanded to one row per entry of tri, and the outputs `outs` -- (trailing shape, dtype)
    each -- allocated with tri's shape in front."""
    dev, lead = operands[0].device, tuple(operands[0].shape[:-1])
    _tensor("tri", tri, torch.int32, device=dev)
    shape = _row_shape(tri, lead)
    n = _count(tri, 1, "elements")
    out = [torch.empty(shape + tail, dtype=dtype, device=dev) for tail, dtype in outs]
    if n > 0:
        q = _OnStream(scene, dev, stream)
        q.call(fn, *[_per_entry(x, lead, shape, q) for x in operands], tri, n, *out)
        q.done(*operands)
    return out


# (dist, point_query, point_scene, crosses) of tri_distance_at and segment_distance_at
_DISTANCE_OUTS = (((), torch.float32), ((3,), torch.float32), ((3,), torch.float32), ((), torch.uint8))


def closest(scene, rays, t_max=None, stream=None):
    """(tri int32, t float32), each of shape rays.shape[:-1]: the reference's closest hit where it lies below t_max, else (-1, 114514)."""
    lib, n = _check(scene, rays, t_max)
    lead = tuple(rays.shape[:-1])
    tri = torch.empty(lead, dtype=torch.int32, device=rays.device)
    t = torch.empty(lead, dtype=torch.float32, device=rays.device)
    if n > 0:
        _OnStream(scene, rays, stream).run(lib.ezrt_query_closest_device, rays, t_max, n, tri, t)
    return tri, t


def occluded(scene, rays, t_max=None, stream=None):
    """bool of shape rays.shape[:-1]: whether the ray hits a triangle at a distance below t_max (any distance without t_max)."""
    lib, n = _check(scene, rays, t_max)
    out = torch.empty(tuple(rays.shape[:-1]), dtype=torch.uint8, device=rays.device)
    if n > 0:
        _OnStream(scene, rays, stream).run(lib.ezrt_query_occluded_device, rays, t_max, n, out)
    return out.view(torch.bool)


_SURFACE_INTEGRATORS = (_abi.INTEGRATOR_P3_DIFFUSE, _abi.INTEGRATOR_P4_DISNEY, _abi.INTEGRATOR_P5_SOBOL, _abi.INTEGRATOR_P5_MIS,
                        _abi.INTEGRATOR_P5_MIS_ANISO)


def surface(scene, rays, t_max=None, integrator=_abi.INTEGRATOR_P5_SOBOL, stream=None):
    """Surface(tri, t, point, normal, inside): `closest` plus the reference's hitTriangle fields of each hit -- point = o + d * t
    (float32 [..., 3]), normal = the smooth shading normal, facing the ray's side (float32 [..., 3]), inside = the ray meets the
    triangle's back (bool).  `integrator` picks the form of the smooth normal as a render call does: 3 and 4 the chapter-3/4 form, 50,
    51 and 52 chapter 5's.  A miss gives zeros in point, normal and inside.  The winner's material is tri36[tri, 18:36]."""
    lib, n = _check(scene, rays, t_max)
    _abi._declare(lib, _abi.SURFACE_ABI)
    if integrator not in _SURFACE_INTEGRATORS:
        raise ValueError("integrator must be one of %s, not %r" % (_SURFACE_INTEGRATORS, integrator))
    lead = tuple(rays.shape[:-1])
    tri = torch.empty(lead, dtype=torch.int32, device=rays.device)
    t = torch.empty(lead, dtype=torch.float32, device=rays.device)
    point = torch.empty(lead + (3,), dtype=torch.float32, device=rays.device)
    normal = torch.empty(lead + (3,), dtype=torch.float32, device=rays.device)
    inside = torch.empty(lead, dtype=torch.uint8, device=rays.device)
    if n > 0:
        _OnStream(scene, rays, stream).run(lib.ezrt_query_surface_device, rays, t_max, n, int(integrator), tri, t, point, normal, inside)
    return Surface(tri, t, point, normal, inside.view(torch.bool))


def all_hits(scene, rays, max_hits, t_max=None, stream=None):
    """(tri int32 [..., max_hits], t float32 [..., max_hits], count int32 [...]): every triangle the ray crosses below t_max, sorted
    by distance (equal distances in the reference's visit order: slot 0 is `closest`'s answer on the bits).  `count` is the full
    number of crossings and may exceed max_hits (1 .. 64); the slots beyond it hold (-1, 114514)."""
    if not isinstance(max_hits, int) or isinstance(max_hits, bool) or not 1 <= max_hits <= _abi.ALL_HITS_MAX:
        raise ValueError("max_hits must be an int in [1, %d], not %r" % (_abi.ALL_HITS_MAX, max_hits))
    n = _check_rays(rays, t_max)
    lib = _scene_lib(scene, _abi.MULTIHIT_ABI)
    lead = tuple(rays.shape[:-1])
    if n * max_hits > 2**31 - 1:
        raise ValueError("at most 2^31 - 1 output slots per call")
    tri = torch.empty(lead + (max_hits,), dtype=torch.int32, device=rays.device)
    t = torch.empty(lead + (max_hits,), dtype=torch.float32, device=rays.device)
    count = torch.empty(lead, dtype=torch.int32, device=rays.device)
    if n > 0:
        _OnStream(scene, rays, stream).run(lib.ezrt_query_all_hits_device, rays, t_max, n, max_hits, tri, t, count)
    return tri, t, count


def surface_at(scene, rays, tri, t, integrator=_abi.INTEGRATOR_P5_SOBOL, stream=None):
    """(point float32 tri.shape + (3,), normal float32 tri.shape + (3,), inside bool tri.shape): for triangle tri[...] at distance
    t[...] along its ray, what `surface` gives for its winner.  `tri` (int32) and `t` (float32) have the shape rays.shape[:-1], or one
    trailing dimension more -- the output of `all_hits` -- and every entry of a row then belongs to the row's ray.  An id that is no
    triangle of the scene (a miss, -1) gives zeros."""
    _check_rays(rays, None)
    lib = _scene_lib(scene, _abi.MULTIHIT_ABI)
    if integrator not in _SURFACE_INTEGRATORS:
        raise ValueError("integrator must be one of %s, not %r" % (_SURFACE_INTEGRATORS, integrator))
    lead = tuple(rays.shape[:-1])
    _tensor("tri", tri, torch.int32, device=rays.device)
    _tensor("t", t, torch.float32, device=rays.device)
    shape = _row_shape(tri, lead)
    if tuple(t.shape) != shape:
        raise ValueError("t must have shape %s, not %s" % (shape, tuple(t.shape)))
    n = _count(tri, 1, "hits")
    point = torch.empty(shape + (3,), dtype=torch.float32, device=rays.device)
    normal = torch.empty(shape + (3,), dtype=torch.float32, device=rays.device)
    inside = torch.empty(shape, dtype=torch.uint8, device=rays.device)
    if n > 0:
        q = _OnStream(scene, rays, stream)
        q.call(lib.ezrt_surface_at_device, _per_entry(rays, lead, shape, q), tri, t, n, int(integrator), point, normal, inside)
        q.done(rays)
    return point, normal, inside.view(torch.bool)


def _check_points(points, d_max):
    """The number of points, after the checks every point query makes of its points and d_max."""
    _tensor("points", points, torch.float32, last=3)
    if d_max is not None:
        _tensor("d_max", d_max, torch.float32, points.shape[:-1], device=points.device)
    return _count(points, 3, "points")


def closest_point(scene, points, d_max=None, stream=None):
    """ClosestPoint(tri int32 [...], point float32 [..., 3], dist float32 [...], bary float32 [..., 2]): for every point of `points`
    (a contiguous float32 GPU tensor [..., 3]) the nearest triangle of the scene, the nearest point on it, the distance and the
    barycentrics (v, w) of that point -- attributes interpolate with (1 - v - w, v, w).  `d_max` (optional, float32, of shape
    points.shape[:-1]) admits only triangles within that distance.  A miss is (-1, zeros, +inf, zeros).  Equal distances: the lowest
    triangle index.  The definition, on the bits: include/ezrt_closest_point.h."""
    n = _check_points(points, d_max)
    lead = tuple(points.shape[:-1])
    lib = _scene_lib(scene, _abi.CLOSEST_POINT_ABI)
    tri = torch.empty(lead, dtype=torch.int32, device=points.device)
    point = torch.empty(lead + (3,), dtype=torch.float32, device=points.device)
    dist = torch.empty(lead, dtype=torch.float32, device=points.device)
    bary = torch.empty(lead + (2,), dtype=torch.float32, device=points.device)
    if n > 0:
        _OnStream(scene, points, stream).run(lib.ezrt_query_closest_point_device, points, d_max, n, tri, point, dist, bary)
    return ClosestPoint(tri, point, dist, bary)


def nearest(scene, points, k, d_max=None, count=False, stream=None):
    """Nearest(tri int32 [..., k], dist float32 [..., k], count int32 [...] or None): for every point of `points` (a contiguous
    float32 GPU tensor [..., 3]) the k nearest triangles of the scene, nearest first, and their distances; equal distances are ordered
    by ascending triangle index, so slot 0 is `closest_point`'s (tri, dist) on the bits and a larger k only appends.  `d_max`
    (optional, float32, of shape points.shape[:-1]) admits only triangles within that distance.  Slots beyond the candidates hold
    (-1, +inf).  `count=True` also returns the full number of triangles within d_max, which may exceed k (1 .. 64) -- at a price: the
    search can then not shrink below d_max, and without a d_max it visits every triangle for every point.  The definition, on the
    bits: include/ezrt_nearest.h; `closest_point_at` gives the points and barycentrics of the rows."""
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= _abi.NEAREST_MAX:
        raise ValueError("k must be an int in [1, %d], not %r" % (_abi.NEAREST_MAX, k))
    n = _check_points(points, d_max)
    lib = _scene_lib(scene, _abi.NEAREST_ABI)
    lead = tuple(points.shape[:-1])
    if n * k > 2**31 - 1:
        raise ValueError("at most 2^31 - 1 output slots per call")
    tri = torch.empty(lead + (k,), dtype=torch.int32, device=points.device)
    dist = torch.empty(lead + (k,), dtype=torch.float32, device=points.device)
    within = torch.empty(lead, dtype=torch.int32, device=points.device) if count else None
    if n > 0:
        _OnStream(scene, points, stream).run(lib.ezrt_query_nearest_device, points, d_max, n, k, tri, dist, within)
    return Nearest(tri, dist, within)


def closest_point_at(scene, points, tri, stream=None):
    """ClosestPoint(tri, point float32 tri.shape + (3,), dist float32 tri.shape, bary float32 tri.shape + (2,)): for triangle
    tri[...] and its point, what `closest_point` gives for its winner -- the nearest point on that triangle, its distance and
    barycentrics.  `tri` (int32) has the shape points.shape[:-1], or one trailing dimension more -- the output of `nearest` -- and
    every entry of a row then belongs to the row's point.  An id that is no triangle of the scene (an unused slot, -1) or a
    non-finite distance gives (zeros, +inf, zeros).  `tri` is returned as given."""
    _check_points(points, None)
    lib = _scene_lib(scene, _abi.NEAREST_ABI)
    f32 = torch.float32
    return ClosestPoint(tri, *_pairs(scene, lib.ezrt_closest_point_at_device, (points,), tri, (((3,), f32), ((), f32), ((2,), f32)), stream))


def _check_axis(axis):
    if not isinstance(axis, int) or isinstance(axis, bool) or not 0 <= axis <= 5:
        raise ValueError("axis must be an int in [0, 5] (+x, -x, +y, -y, +z, -z), not %r" % (axis,))


def inside(scene, points, axis=0, crossings=False, stream=None):
    """bool [...]: whether each point of `points` (a contiguous float32 GPU tensor [..., 3]) is inside the mesh -- the parity of the
    number of triangles crossed by the ray that leaves the point along `axis` (0..5: +x, -x, +y, -y, +z, -z), by a rule that is
    consistent on shared edges and vertices and independent of the tree, of the order of the triangles and of their windings.
    `crossings=True` returns (inside, crossings int32 [...]).  A point with a non-finite coordinate crosses nothing.  On an open mesh
    the answer is still that parity and may differ between axes: vote over several -- or use `winding_number(...) > 0.5` (`abs(...)`
    for a mesh that faces inwards), the robust test on open meshes.  The definition, on the bits: include/ezrt_inside.h."""
    _check_axis(axis)
    n = _check_points(points, None)
    lib = _scene_lib(scene, _abi.INSIDE_ABI)
    lead = tuple(points.shape[:-1])
    out = torch.empty(lead, dtype=torch.uint8, device=points.device)
    count = torch.empty(lead, dtype=torch.int32, device=points.device) if crossings else None
    if n > 0:
        _OnStream(scene, points, stream).run(lib.ezrt_query_inside_device, points, n, axis, out, count)
    return (out.view(torch.bool), count) if crossings else out.view(torch.bool)


def signed_distance(scene, points, d_max=None, axis=0, stream=None):
    """SignedDistance(tri int32 [...], point float32 [..., 3], dist float32 [...], bary float32 [..., 2], inside bool [...]):
    `closest_point`'s tri, point and bary on the bits, its dist with the sign bit set where the point is inside the mesh (`inside`'s
    answer for `axis`), in one launch.  A miss (no triangle within `d_max`) is +inf outside and -inf inside.  The definition, on the
    bits: include/ezrt_inside.h."""
    _check_axis(axis)
    n = _check_points(points, d_max)
    lib = _scene_lib(scene, _abi.INSIDE_ABI)
    lead = tuple(points.shape[:-1])
    tri = torch.empty(lead, dtype=torch.int32, device=points.device)
    point = torch.empty(lead + (3,), dtype=torch.float32, device=points.device)
    dist = torch.empty(lead, dtype=torch.float32, device=points.device)
    bary = torch.empty(lead + (2,), dtype=torch.float32, device=points.device)
    ins = torch.empty(lead, dtype=torch.uint8, device=points.device)
    if n > 0:
        _OnStream(scene, points, stream).run(lib.ezrt_query_signed_distance_device, points, d_max, n, axis, tri, point, dist, bary, ins)
    return SignedDistance(tri, point, dist, bary, ins.view(torch.bool))


def _check_boxes(lo, hi):
    """The number of boxes, after the checks every box query makes of its corners."""
    _tensor("lo", lo, torch.float32, last=3)
    _tensor("hi", hi, torch.float32, last=3)
    if hi.device != lo.device:
        raise ValueError("hi is on %s, not on %s" % (hi.device, lo.device))
    if tuple(hi.shape) != tuple(lo.shape):
        raise ValueError("hi must have shape %s, not %s" % (tuple(lo.shape), tuple(hi.shape)))
    return _count(lo, 3, "boxes")


def box_overlap(scene, lo, hi, max_k=8, count=False, stream=None):
    """BoxOverlap(tri int32 [..., max_k], n_overlap int32 [...] or None): for every axis-aligned box [lo, hi] (contiguous float32 GPU
    tensors of one shape [..., 3]) the triangles of the scene that touch it -- the exact separating-axis test of a closed triangle
    against a closed box, so touching counts and a degenerate triangle overlaps as the segment or point it is.  `tri` holds the
    lowest triangle indices in ascending order, then -1: a larger max_k (0 .. 64) only appends, and the answer depends on neither the
    tree nor the order of the visits.  `count=True` also returns the full number of overlapping triangles, which may exceed max_k;
    with max_k == 0 the call only counts (`tri` is empty and `count` must be True).  A box with a non-finite number or lo > hi on
    some axis overlaps nothing, as does a triangle with a non-finite vertex.  The definition, on the bits:
    include/ezrt_box_overlap.h; `box_overlap_at` tests pairs.  `box_overlap_list` returns every such triangle, not the
    lowest max_k."""
    _check_max_k(max_k, _abi.BOX_OVERLAP_MAX, count)
    n = _check_boxes(lo, hi)
    lib = _scene_lib(scene, _abi.BOX_OVERLAP_ABI)
    return BoxOverlap(*_overlap_rows(scene, lib.ezrt_query_box_overlap_device, (lo, hi), n, lo.shape[:-1], lo.device, max_k, count, stream))


def box_overlap_at(scene, lo, hi, tri, stream=None):
    """bool tri.shape: whether triangle tri[...] touches its box, by `box_overlap`'s test.  `tri` (int32) has the shape lo.shape[:-1],
    or one trailing dimension more -- the output of `box_overlap` -- and every entry of a row then belongs to the row's box.  An id
    that is no triangle of the scene (an unused slot, -1) gives False."""
    _check_boxes(lo, hi)
    lib = _scene_lib(scene, _abi.BOX_OVERLAP_ABI)
    return _pairs(scene, lib.ezrt_box_overlap_at_device, (lo, hi), tri, (((), torch.uint8),), stream)[0].view(torch.bool)


def _check_tris(tris):
    """The number of query triangles, after the checks every triangle query makes of them."""
    _tensor("tris", tris, torch.float32, last=9)
    return _count(tris, 9, "triangles")


def tri_overlap(scene, tris, max_k=8, count=False, stream=None):
    """TriOverlap(tri int32 [..., max_k], n_overlap int32 [...] or None): for every triangle of `tris` (a contiguous float32 GPU
    tensor [..., 9]: p1 p2 p3) the triangles of the scene that it crosses or touches -- the exact separating-axis test of two closed
    triangles, so touching counts (a vertex on a face, an edge or a vertex, edges that cross, coplanar triangles that share an edge or
    a point), coplanar pairs are answered by the same rule, and swapping the two triangles gives the same answer.  `tri` holds the
    lowest triangle indices in ascending order, then -1: a larger max_k (0 .. 64) only appends, and the answer depends on neither the
    tree nor the order of the visits.  `count=True` also returns the full number of overlapping triangles, which may exceed max_k;
    with max_k == 0 the call only counts (`tri` is empty and `count` must be True).  A triangle with a non-finite number or with
    collinear or repeated vertices overlaps nothing, on either side -- unlike `box_overlap`, where a degenerate triangle overlaps as
    the segment or point it is.  The definition, on the bits: include/ezrt_tri_overlap.h; `tri_overlap_at` tests pairs.  `tri_overlap_list` returns every such triangle, not the
    lowest max_k."""
    _check_max_k(max_k, _abi.TRI_OVERLAP_MAX, count)
    n = _check_tris(tris)
    lib = _scene_lib(scene, _abi.TRI_OVERLAP_ABI)
    return TriOverlap(*_overlap_rows(scene, lib.ezrt_query_tri_overlap_device, (tris,), n, tris.shape[:-1], tris.device, max_k, count, stream))


def tri_overlap_at(scene, tris, tri, stream=None):
    """bool tri.shape: whether triangle tri[...] of the scene crosses or touches its query triangle, by `tri_overlap`'s test.  `tri`
    (int32) has the shape tris.shape[:-1], or one trailing dimension more -- the output of `tri_overlap` -- and every entry of a row
    then belongs to the row's query triangle.  An id that is no triangle of the scene (an unused slot, -1) gives False."""
    _check_tris(tris)
    lib = _scene_lib(scene, _abi.TRI_OVERLAP_ABI)
    return _pairs(scene, lib.ezrt_tri_overlap_at_device, (tris,), tri, (((), torch.uint8),), stream)[0].view(torch.bool)


def self_overlap(scene, ids=None, max_k=8, count=False, stream=None):
    """SelfOverlap(tri int32 [..., max_k], n_overlap int32 [...] or None): for every triangle id of `ids` (a contiguous int32 GPU
    tensor of any shape; None: every triangle of the scene, in order, on the current device -- the scene's when it was created there)
    the OTHER triangles of the scene that meet it anywhere except in what the two share by value: nothing for neighbours that
    share a vertex or an edge and are otherwise apart, the crossing for two that pierce each other from a shared vertex or fold onto
    each other over a shared edge, a duplicated face, and `tri_overlap`'s test for two that share nothing.  A mesh that does not
    cross itself has empty rows: what `inside` and `signed_distance` assume, to be checked between two refits.  `tri` holds the
    lowest triangle indices in ascending order, then -1: a larger max_k (0 .. 64) only appends, a pair appears in both triangles'
    rows, and the answer depends on neither the tree nor the order or winding of any triangle.  `count=True` also returns the full
    number of crossing triangles, which may exceed max_k; with max_k == 0 the call only counts (`tri` is empty and `count` must be
    True).  An id that is no triangle of the scene, or a triangle that is not live, has an empty row.  The definition, on the bits:
    include/ezrt_self_overlap.h; `self_overlap_at` tests pairs.  `self_overlap_list` returns every such triangle, not the
    lowest max_k."""
    _check_max_k(max_k, _abi.SELF_OVERLAP_MAX, count)
    if ids is not None:
        _tensor("ids", ids, torch.int32)
    lib = _scene_lib(scene, _abi.SELF_OVERLAP_ABI)
    if ids is None:
        lead, device = (scene.stats()["n_tri"],), torch.device("cuda", torch.cuda.current_device())
        n = lead[0]
    else:
        lead, device = ids.shape, ids.device
        n = _count(ids, 1, "triangle ids")
    return SelfOverlap(*_overlap_rows(scene, lib.ezrt_query_self_overlap_device, (ids,), n, lead, device, max_k, count, stream))


def self_overlap_at(scene, a, b, stream=None):
    """bool a.shape: whether triangles a[...] and b[...] of the scene cross, by `self_overlap`'s test.  `a` and `b` are contiguous
    int32 GPU tensors of one shape.  Equal ids, an id that is no triangle of the scene (an unused slot, -1) and a triangle that is
    not live give False."""
    _tensor("a", a, torch.int32)
    lib = _scene_lib(scene, _abi.SELF_OVERLAP_ABI)
    _tensor("b", b, torch.int32, shape=a.shape, device=a.device)
    n = _count(a, 1, "pairs")
    out = torch.empty(tuple(a.shape), dtype=torch.uint8, device=a.device)
    if n > 0:
        _OnStream(scene, a, stream).run(lib.ezrt_self_overlap_at_device, a, b, n, out)
    return out.view(torch.bool)


def tri_distance(scene, tris, d_max=None, stream=None):
    """TriDistance(tri int32 [...], dist float32 [...], point_query float32 [..., 3], point_scene float32 [..., 3], crosses bool
    [...]): for every triangle of `tris` (a contiguous float32 GPU tensor [..., 9]: p1 p2 p3) the nearest triangle of the scene, the
    distance between the two, and the points where they come closest -- `point_query` on the query triangle, `point_scene` on the
    scene's.  The distance is taken over vertex against face, both ways, and edge against edge; where the two triangles cross or
    touch by `tri_overlap`'s test it is 0 and `crosses` is set, and the two points are then the nearest features, not a common
    point.  `d_max` (optional, float32, of shape tris.shape[:-1]) admits only triangles within that distance: a clearance check.  A
    miss is (-1, +inf, zeros, zeros, False).  Equal distances: a triangle that crosses first, then the lowest triangle index, so
    `crosses` is True exactly where `tri_overlap` finds something, and `tri` is then its row's first entry.  A triangle with a non-finite number or with
    collinear or repeated vertices misses as a query and is never found in the scene.  The definition, on the bits:
    include/ezrt_tri_distance.h; `tri_distance_at` evaluates pairs."""
    n = _check_tris(tris)
    if d_max is not None:
        _tensor("d_max", d_max, torch.float32, tris.shape[:-1], device=tris.device)
    lead = tuple(tris.shape[:-1])
    lib = _scene_lib(scene, _abi.TRI_DISTANCE_ABI)
    tri = torch.empty(lead, dtype=torch.int32, device=tris.device)
    dist = torch.empty(lead, dtype=torch.float32, device=tris.device)
    point_query = torch.empty(lead + (3,), dtype=torch.float32, device=tris.device)
    point_scene = torch.empty(lead + (3,), dtype=torch.float32, device=tris.device)
    crosses = torch.empty(lead, dtype=torch.uint8, device=tris.device)
    if n > 0:
        _OnStream(scene, tris, stream).run(lib.ezrt_query_tri_distance_device, tris, d_max, n, tri, dist, point_query, point_scene, crosses)
    return TriDistance(tri, dist, point_query, point_scene, crosses.view(torch.bool))


def tri_distance_at(scene, tris, tri, stream=None):
    """TriDistance(tri, dist float32 tri.shape, point_query float32 tri.shape + (3,), point_scene float32 tri.shape + (3,), crosses
    bool tri.shape): for triangle tri[...] of the scene and its query triangle, what `tri_distance` gives for its winner.  `tri`
    (int32) has the shape tris.shape[:-1], or one trailing dimension more -- rows of `tri_overlap` or `nearest` -- and every entry of
    a row then belongs to the row's query triangle.  An id that is no triangle of the scene (an unused slot, -1) or a triangle that
    is not live on either side gives (+inf, zeros, zeros, False).  `tri` is returned as given."""
    _check_tris(tris)
    lib = _scene_lib(scene, _abi.TRI_DISTANCE_ABI)
    dist, point_query, point_scene, crosses = _pairs(scene, lib.ezrt_tri_distance_at_device, (tris,), tri, _DISTANCE_OUTS, stream)
    return TriDistance(tri, dist, point_query, point_scene, crosses.view(torch.bool))


def _check_spheres(rays, radius, t_max):
    n = _check_rays(rays, t_max)
    _tensor("radius", radius, torch.float32, rays.shape[:-1], device=rays.device)
    return n


def sphere_cast(scene, rays, radius, t_max=None, stream=None):
    """SphereCast(tri int32 [...], t float32 [...], point float32 [..., 3], touching bool [...]): for every ray of `rays` (a
    contiguous float32 GPU tensor [..., 6]: origin o, direction d -- d need not have unit length) the first triangle that a sphere of
    radius `radius` (float32, of shape rays.shape[:-1], world units) touches while its centre moves along o + d*t, the time t of that
    contact IN UNITS OF d, and the contact point on the triangle: the contact normal is (o + d*t - point) / radius.  Where the sphere
    already touches the mesh at t = 0, `touching` is set, t is 0 and (tri, point) are those of `closest_point(scene, o, radius)`.
    `t_max` (optional, float32, of shape rays.shape[:-1]) admits only contacts at t <= t_max.  A miss is (-1, +inf, zeros, False).
    Equal t: the lowest triangle index.  A query with a non-finite number, a negative radius or a direction of length 0 misses.  The
    definition, on the bits: include/ezrt_sphere_cast.h; `sphere_cast_at` evaluates pairs."""
    n = _check_spheres(rays, radius, t_max)
    lead = tuple(rays.shape[:-1])
    lib = _scene_lib(scene, _abi.SPHERE_CAST_ABI)
    tri = torch.empty(lead, dtype=torch.int32, device=rays.device)
    t = torch.empty(lead, dtype=torch.float32, device=rays.device)
    point = torch.empty(lead + (3,), dtype=torch.float32, device=rays.device)
    touching = torch.empty(lead, dtype=torch.uint8, device=rays.device)
    if n > 0:
        _OnStream(scene, rays, stream).run(lib.ezrt_query_sphere_cast_device, rays, radius, t_max, n, tri, t, point, touching)
    return SphereCast(tri, t, point, touching.view(torch.bool))


def sphere_cast_at(scene, rays, radius, tri, stream=None):
    """SphereCast(tri, t float32 tri.shape, point float32 tri.shape + (3,), touching bool tri.shape): for triangle tri[...] of the
    scene and its ray and radius, what `sphere_cast` gives for its winner (no t_max).  `tri` (int32) has the shape rays.shape[:-1],
    or one trailing dimension more -- rows of `nearest` -- and every entry of a row then belongs to the row's ray.  An id that is no
    triangle of the scene (an unused slot, -1), a query that is not live or a pair without a contact gives (+inf, zeros, False).
    `tri` is returned as given."""
    _check_spheres(rays, radius, None)
    lib = _scene_lib(scene, _abi.SPHERE_CAST_ABI)
    t, point, touching = _pairs(scene, lib.ezrt_sphere_cast_at_device, (rays, radius.unsqueeze(-1)), tri,
                                (((), torch.float32), ((3,), torch.float32), ((), torch.uint8)), stream)
    return SphereCast(tri, t, point, touching.view(torch.bool))


def _check_segs(segs):
    """The number of segments, after the checks every segment query makes of them."""
    _tensor("segs", segs, torch.float32, last=6)
    return _count(segs, 6, "segments")


def segment_distance(scene, segs, d_max=None, stream=None):
    """SegmentDistance(tri int32 [...], dist float32 [...], point_query float32 [..., 3], point_scene float32 [..., 3], crosses bool
    [...]): for every segment of `segs` (a contiguous float32 GPU tensor [..., 6]: THE TWO END POINTS a, b -- not an origin and a
    direction) the nearest triangle of the scene, the distance between the two, and the points where they come closest --
    `point_query` on the segment, `point_scene` on the triangle.  The distance is taken over the two end points against the face and
    the segment against the three edges; where the segment crosses or touches the triangle it is 0 and `crosses` is set, and the two
    points are then the nearest features, not a common point.  `d_max` (optional, float32, of shape segs.shape[:-1]) admits only
    triangles within that distance: the clearance check of a capsule of that radius.  A miss is (-1, +inf, zeros, zeros, False).
    Equal distances: a triangle that is crossed first, then the lowest triangle index.  a == b is a point.  A segment with a
    non-finite number misses; a triangle with a non-finite number or with collinear or repeated vertices is never found.  The
    definition, on the bits: include/ezrt_segment.h; `segment_distance_at` evaluates pairs."""
    n = _check_segs(segs)
    if d_max is not None:
        _tensor("d_max", d_max, torch.float32, segs.shape[:-1], device=segs.device)
    lead = tuple(segs.shape[:-1])
    lib = _scene_lib(scene, _abi.SEGMENT_ABI)
    tri = torch.empty(lead, dtype=torch.int32, device=segs.device)
    dist = torch.empty(lead, dtype=torch.float32, device=segs.device)
    point_query = torch.empty(lead + (3,), dtype=torch.float32, device=segs.device)
    point_scene = torch.empty(lead + (3,), dtype=torch.float32, device=segs.device)
    crosses = torch.empty(lead, dtype=torch.uint8, device=segs.device)
    if n > 0:
        _OnStream(scene, segs, stream).run(lib.ezrt_query_segment_distance_device, segs, d_max, n, tri, dist, point_query, point_scene, crosses)
    return SegmentDistance(tri, dist, point_query, point_scene, crosses.view(torch.bool))


def segment_distance_at(scene, segs, tri, stream=None):
    """SegmentDistance(tri, dist float32 tri.shape, point_query float32 tri.shape + (3,), point_scene float32 tri.shape + (3,),
    crosses bool tri.shape): for triangle tri[...] of the scene and its segment (`segs` [..., 6]: the two END POINTS), what
    `segment_distance` gives for its winner.  `tri` (int32) has the shape segs.shape[:-1], or one trailing dimension more -- rows of
    `capsule_overlap` or `nearest` -- and every entry of a row then belongs to the row's segment.  An id that is no triangle of the
    scene (an unused slot, -1), a segment with a non-finite number or a triangle that is not live gives (+inf, zeros, zeros, False).
    `tri` is returned as given."""
    _check_segs(segs)
    lib = _scene_lib(scene, _abi.SEGMENT_ABI)
    dist, point_query, point_scene, crosses = _pairs(scene, lib.ezrt_segment_distance_at_device, (segs,), tri, _DISTANCE_OUTS, stream)
    return SegmentDistance(tri, dist, point_query, point_scene, crosses.view(torch.bool))


def capsule_overlap(scene, segs, radius, max_k=8, count=False, stream=None):
    """CapsuleOverlap(tri int32 [..., max_k], n_overlap int32 [...] or None): for every capsule -- the segment of `segs` (a contiguous
    float32 GPU tensor [..., 6]: THE TWO END POINTS a, b, not an origin and a direction) and its `radius` (float32, of shape
    segs.shape[:-1], world units) -- the triangles of the scene within `radius` of the segment by `segment_distance`'s rule:
    dist2 <= radius*radius in float32.  `tri` holds the lowest triangle indices in ascending order, then -1: a larger max_k (0 .. 64)
    only appends, and the answer depends on neither the tree nor the order of the visits.  `count=True` also returns the full number
    of such triangles, which may exceed max_k; with max_k == 0 the call only counts (`tri` is empty and `count` must be True).
    radius == 0 lists the triangles the segment crosses or touches, and any whose nearest point rounds onto it.  A capsule with a
    non-finite number or a negative radius touches nothing.  `segment_distance(scene, segs, radius)` finds a triangle exactly where
    the count here is > 0.  The definition, on the bits: include/ezrt_segment.h.  `capsule_overlap_list` returns every such triangle, not the
    lowest max_k."""
    _check_max_k(max_k, _abi.CAPSULE_OVERLAP_MAX, count)
    n = _check_segs(segs)
    _tensor("radius", radius, torch.float32, segs.shape[:-1], device=segs.device)
    lib = _scene_lib(scene, _abi.SEGMENT_ABI)
    return CapsuleOverlap(*_overlap_rows(scene, lib.ezrt_query_capsule_overlap_device, (segs, radius), n, segs.shape[:-1], segs.device,
                                         max_k, count, stream))


def _check_obbs(centre, axes):
    """The number of oriented boxes, after the checks every such query makes of its centres and axes."""
    _tensor("centre", centre, torch.float32, last=3)
    _tensor("axes", axes, torch.float32)
    if axes.device != centre.device:
        raise ValueError("axes is on %s, not on %s" % (axes.device, centre.device))
    if tuple(axes.shape) != tuple(centre.shape) + (3,):
        raise ValueError("axes must have shape %s, not %s" % (tuple(centre.shape) + (3,), tuple(axes.shape)))
    if not axes.is_contiguous():
        raise ValueError("axes must be contiguous")
    return _count(centre, 3, "boxes")


def obb_overlap(scene, centre, axes, max_k=8, count=False, stream=None):
    """ObbOverlap(tri int32 [..., max_k], n_overlap int32 [...] or None): for every oriented box -- `centre` [..., 3] and `axes`
    [..., 3, 3] with the half-axis vectors u0 u1 u2 as rows, contiguous float32 GPU tensors; the box is c + s0 u0 + s1 u1 + s2 u2 with
    |s_j| <= 1, and the vectors need not be unit or orthogonal (a sheared box is allowed) -- the triangles of the scene that touch it:
    the exact separating-axis test of a closed triangle against a closed parallelepiped, so touching counts and a degenerate triangle
    overlaps as the segment or point it is.  `tri` holds the lowest triangle indices in ascending order, then -1: a larger max_k
    (0 .. 64) only appends, and the answer depends on neither the tree nor the order of the visits.  `count=True` also returns the
    full number of overlapping triangles, which may exceed max_k; with max_k == 0 the call only counts (`tri` is empty and `count`
    must be True).  A box with a non-finite number or without volume (a zero axis, parallel or coplanar axes: give a thin box
    instead) overlaps nothing, as does a triangle with a non-finite vertex.  The definition, on the bits:
    include/ezrt_obb_overlap.h; `obb_overlap_at` tests pairs.  `obb_overlap_list` returns every such triangle, not the
    lowest max_k."""
    _check_max_k(max_k, _abi.OBB_OVERLAP_MAX, count)
    n = _check_obbs(centre, axes)
    lib = _scene_lib(scene, _abi.OBB_OVERLAP_ABI)
    return ObbOverlap(*_overlap_rows(scene, lib.ezrt_query_obb_overlap_device, (centre, axes), n, centre.shape[:-1], centre.device, max_k, count,
                                     stream))


def obb_overlap_at(scene, centre, axes, tri, stream=None):
    """bool tri.shape: whether triangle tri[...] touches its oriented box, by `obb_overlap`'s test.  `tri` (int32) has the shape
    centre.shape[:-1], or one trailing dimension more -- the output of `obb_overlap` -- and every entry of a row then belongs to the
    row's box.  An id that is no triangle of the scene (an unused slot, -1) gives False."""
    _check_obbs(centre, axes)
    lib = _scene_lib(scene, _abi.OBB_OVERLAP_ABI)
    flat = axes.reshape(tuple(centre.shape[:-1]) + (9,))
    return _pairs(scene, lib.ezrt_obb_overlap_at_device, (centre, flat), tri, (((), torch.uint8),), stream)[0].view(torch.bool)


def _check_chunks(chunks):
    if chunks is None:
        return 0
    if not isinstance(chunks, int) or isinstance(chunks, bool) or chunks < 1:
        raise ValueError("chunks must be None or an int >= 1, not %r" % (chunks,))
    return min(chunks, 2**31 - 1)


def winding_number(scene, points, fixed=False, chunks=None, stream=None):
    """float32 [...]: the generalised winding number of the mesh at each point of `points` (a contiguous float32 GPU tensor [..., 3])
    -- the solid angles of all triangles summed and divided by 4 pi: 1 inside and 0 outside a closed mesh that faces outwards (-1
    inside one that faces inwards), and a smooth value across a hole, a doubled sheet or a self-crossing, where `inside`'s parity
    differs between axes: `winding_number(...) > 0.5` (`abs(...)` for inward-facing meshes) is the robust inside test on open
    meshes.  `fixed=True` returns (winding, fixed int64 [...]): the sum in units of 2^-36 rad of half solid angle, an INTEGER sum and
    so independent of the order of the triangles, the tree and the split of the work, on the bits; `fixed` of mesh parts (or of one
    mesh split over devices) may be added, and a flipped triangle negates its term exactly.  A point in the plane of a triangle gets
    nothing from it; a point with a non-finite coordinate has 0.  Every triangle is summed for every point (no tree is read):
    `chunks=None` lets the library split the triangle range over workgroups where the points alone do not fill the device,
    `chunks=k` forces k slices -- the answer is the same.  The definition, on the bits: include/ezrt_winding.h."""
    c = _check_chunks(chunks)
    n = _check_points(points, None)
    lib = _scene_lib(scene, _abi.WINDING_ABI)
    lead = tuple(points.shape[:-1])
    acc = torch.empty(lead, dtype=torch.int64, device=points.device) if fixed else None
    out = torch.empty(lead, dtype=torch.float32, device=points.device)
    if n > 0:
        q = _OnStream(scene, points, stream)
        if not fixed:                                                # the call's accumulator, a temporary where it is not returned
            with q.on():
                acc = torch.empty(lead, dtype=torch.int64, device=points.device)
        q.run(lib.ezrt_query_winding_device, points, n, c, acc, out)
    return (out, acc) if fixed else out


def winding_number_at(scene, points, tri, stream=None):
    """(winding float32 tri.shape, fixed int64 tri.shape): the term of triangle tri[...] alone in `winding_number` of its point.  `tri`
    (int32) has the shape points.shape[:-1], or one trailing dimension more, and every entry of a row then belongs to the row's
    point.  An id that is no triangle of the scene (an unused slot, -1) gives 0.  The sum of `fixed` over all triangles of the scene
    is `winding_number`'s."""
    _check_points(points, None)
    lib = _scene_lib(scene, _abi.WINDING_ABI)
    acc, out = _pairs(scene, lib.ezrt_winding_at_device, (points,), tri, (((), torch.int64), ((), torch.float32)), stream)
    return out, acc


def _check_slices(slices):
    if slices is None:
        return 0
    if not isinstance(slices, int) or isinstance(slices, bool) or slices < 1:
        raise ValueError("slices must be None or an int >= 1, not %r" % (slices,))
    return min(slices, 2**31 - 1)


def _check_planes(planes):
    _tensor("planes", planes, torch.float32, last=4)
    return _count(planes, 4, "planes")


def _plane_counts(q, lib, planes, n, c, n_cross=None):
    """(part int32 [n, S], offsets int64 [n + 1] or None), enqueued on the query's stream: the counts go into the caller's n_cross
    (int32 [n]), or without one into a temporary, and the offsets are then made of them.  part is a temporary of the caller's."""
    S = int(lib.ezrt_plane_slices(n, q.scene.stats()["n_tri"], c))
    dev = planes.device
    offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev) if n_cross is None else None
    with q.on():
        part = torch.empty((n, S), dtype=torch.int32, device=dev)
        if n_cross is None:
            n_cross = torch.empty((n,), dtype=torch.int32, device=dev)
    q.call(lib.ezrt_query_plane_count_device, planes, n, c, part, n_cross, offsets)
    return part, offsets


def plane_count(scene, planes, slices=None, stream=None):
    """int32 planes.shape[:-1]: the number of triangles each plane of `planes` (a contiguous float32 GPU tensor [..., 4]: a, b, c, d of
    a x + b y + c z = d, the normal need not be unit) CROSSES: the triangles with a vertex on the plane or on the side its normal
    points to, and a vertex strictly on the other side.  A plane with a non-finite entry or a zero normal crosses nothing.  Every
    plane is tested against every triangle (no tree is read); `slices=None` lets the library split the triangle range over
    workgroups where the planes alone do not fill the device, `slices=k` forces k slices -- the answer is the same.  The
    definition, on the bits: include/ezrt_plane.h."""
    c = _check_slices(slices)
    n = _check_planes(planes)
    lib = _scene_lib(scene, _abi.PLANE_ABI)
    n_cross = torch.empty(tuple(planes.shape[:-1]), dtype=torch.int32, device=planes.device)
    if n > 0:
        q = _OnStream(scene, planes, stream)
        _plane_counts(q, lib, planes, n, c, n_cross)
        q.done()
    return n_cross


def plane_section(scene, planes, capacity=None, slices=None, stream=None):
    """(offsets int64 [n + 1], tri int32 [rows], seg float32 [rows, 2, 3]): the cross-sections of the mesh with the n planes of `planes`
    ([..., 4], flattened row-major), complete, in CSR form: rows offsets[i] .. offsets[i + 1] hold the triangles plane i crosses in
    ascending id, and for each the segment q0 -> q1 in which the plane cuts it, oriented so that the material of an outward-wound
    mesh lies on its left seen from the side the plane's normal points to.  Two triangles that share an edge by value get the same
    end point on the bits, so the segments chain into loops with a dictionary on the end points' bytes.  `capacity=None`
    synchronises the stream once to read the total, offsets[n], and returns exactly that many rows.  A given `capacity` never
    synchronises and returns `capacity` rows: rows past offsets[n] keep tri == -1, and rows that did not fit are simply missing --
    compare offsets[n] with the capacity.  `slices` as for plane_count.  The definition, on the bits: include/ezrt_plane.h."""
    c = _check_slices(slices)
    n = _check_planes(planes)
    _check_capacity("capacity", capacity)
    lib = _scene_lib(scene, _abi.PLANE_ABI)
    dev = planes.device
    q = _OnStream(scene, planes, stream)
    if n == 0:
        rows = 0 if capacity is None else capacity
        with q.on():
            return (torch.zeros((1,), dtype=torch.int64, device=dev), torch.full((rows,), -1, dtype=torch.int32, device=dev),
                    torch.zeros((rows, 2, 3), dtype=torch.float32, device=dev))
    part, offsets = _plane_counts(q, lib, planes, n, c)
    with q.on():
        rows = int(offsets[n].item()) if capacity is None else capacity    # None: the one synchronisation, of the query's stream
        tri = torch.full((rows,), -1, dtype=torch.int32, device=dev)
        seg = torch.zeros((rows, 2, 3), dtype=torch.float32, device=dev)
    q.run(lib.ezrt_query_plane_section_device, planes, n, c, part, offsets, rows, tri if rows else None, seg if rows else None)
    return offsets, tri, seg


def plane_section_at(scene, planes, tri, stream=None):
    """(crosses bool tri.shape, side int8 tri.shape + (3,), seg float32 tri.shape + (2, 3)): the plane rule for pairs already held --
    plane i against triangle tri[i].  `tri` (int32) has the shape planes.shape[:-1], or one trailing dimension more, and every entry
    of a row then belongs to the row's plane.  `side` is the sign of p1, p2 and p3 against the plane (-1 / 0 / +1; 0 is ON the plane,
    which the rule counts to the normal's side): with it a caller applies a touching rule of their own.  An id that is no triangle
    of the scene (an unused slot, -1), a plane that is not live and a triangle with a non-finite coordinate give zeros; a pair that
    is not crossed has a zero seg.  `crosses` summed over all triangles of the scene is plane_count's."""
    _check_planes(planes)
    lib = _scene_lib(scene, _abi.PLANE_ABI)
    crosses, side, seg = _pairs(scene, lib.ezrt_plane_section_at_device, (planes,), tri,
                                (((), torch.uint8), ((3,), torch.int8), ((2, 3), torch.float32)), stream)
    return crosses.view(torch.bool), side, seg


def _check_tile_rows(tile_rows):
    if tile_rows is None:
        return 0
    if not isinstance(tile_rows, int) or isinstance(tile_rows, bool) or tile_rows < 1:
        raise ValueError("tile_rows must be None or an int >= 1, not %r" % (tile_rows,))
    return min(tile_rows, 2**31 - 1)


def _check_capacity(name, x):
    if x is not None and (not isinstance(x, int) or isinstance(x, bool) or x < 0):
        raise ValueError("%s must be None or an int >= 0, not %r" % (name, x))


def plane_loops_of(scene, offsets, seg, capacity=None, loop_capacity=None, want_next=False, tile_rows=None, stream=None):
    """PlaneLoopsOf(next int64 [capacity] or None, order int64 [capacity], plane_loops int64 [n + 1], loop_offsets int64
    [loop_capacity + 1], closed uint8 [loop_capacity]): the rows of a section already held -- `offsets` (int64 [n + 1]) and `seg`
    (float32 [rows, 2, 3]) as plane_section returns them -- chained into polylines by comparing the bits of their end points:
    loop l of plane i, plane_loops[i] <= l < plane_loops[i + 1], is the rows order[loop_offsets[l] .. loop_offsets[l + 1]) in walking
    order, closed[l] says whether it returns to its first point, and next (want_next=True) is every row's successor or -1.  A row
    of zero length is in no loop.  `capacity` (default: all rows of seg) is the number of rows that count: a plane whose rows reach
    past it has no loops.  Entries of order past loop_offsets[L], and of next outside chained planes, are -1.  With both `capacity`
    and `loop_capacity` given the call never synchronises; loops that do not fit are missing from loop_offsets and closed (entries
    past the loops hold -1 and 0) -- compare plane_loops[n] with loop_capacity.  `loop_capacity=None` makes room for as many loops
    as there are rows, synchronises the stream once to read plane_loops[n] and returns exactly L + 1 and L entries.  `tile_rows`
    (None: the library's choice) is the longest plane that is chained in LDS; it changes the time only.  MEMORY: besides the outputs
    (8 or 16 B per row of the capacity, 9 B per loop of the loop capacity -- with `loop_capacity=None` per ROW) the call allocates the
    library's scratch, ezrt_plane_loops_work_bytes(capacity) = 64 B per row of the capacity: 1.5 GB for a section of 24 M rows,
    beside the 0.6 GB of its `seg`; it is freed to torch's allocator when the stream is done with it.  The definition:
    include/ezrt_plane_loops.h."""
    return _plane_loops_of(scene, offsets, seg, capacity, loop_capacity, want_next, tile_rows, stream)[0]


def _plane_loops_of(scene, offsets, seg, capacity, loop_capacity, want_next, tile_rows, stream):
    """(plane_loops_of's answer, the number of chained rows where loop_capacity is None -- read in the same synchronisation -- else None)"""
    c = _check_tile_rows(tile_rows)
    _check_capacity("capacity", capacity)
    _check_capacity("loop_capacity", loop_capacity)
    _tensor("offsets", offsets, torch.int64)
    if offsets.dim() != 1 or offsets.shape[0] < 1:
        raise ValueError("offsets must have shape [n + 1], not %s" % (tuple(offsets.shape),))
    _tensor("seg", seg, torch.float32, device=offsets.device)
    if seg.dim() != 3 or tuple(seg.shape[1:]) != (2, 3):
        raise ValueError("seg must have shape [rows, 2, 3], not %s" % (tuple(seg.shape),))
    rows = seg.shape[0] if capacity is None else capacity
    if rows > seg.shape[0]:
        raise ValueError("capacity %d exceeds the %d rows of seg" % (rows, seg.shape[0]))
    n = _count(offsets, 1, "planes") - 1
    lib = _scene_lib(scene, _abi.PLANE_LOOPS_ABI)
    dev = offsets.device
    q = _OnStream(scene, offsets, stream)
    lcap = rows if loop_capacity is None else loop_capacity
    work_bytes = int(lib.ezrt_plane_loops_work_bytes(rows))
    work = q.scratch(dev, work_bytes + 8, summary=False)[0]
    with q.on():
        nxt = torch.full((rows,), -1, dtype=torch.int64, device=dev) if want_next else None
        order = torch.full((rows,), -1, dtype=torch.int64, device=dev)
        plane_loops = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        loop_offsets = torch.full((lcap + 1,), -1, dtype=torch.int64, device=dev)
        closed = torch.zeros((lcap,), dtype=torch.uint8, device=dev)
        if n == 0:
            loop_offsets[0] = 0
    if n > 0:
        q.call(lib.ezrt_plane_loops_device, offsets, n, seg if rows else None, rows, c, nxt if rows else None, order if rows else None,
               plane_loops, lcap, loop_offsets, closed if lcap else None, work, work_bytes)
    q.done(offsets, seg, nxt, order, plane_loops, loop_offsets, closed)
    R = None
    if loop_capacity is None:
        with q.on():                                                 # the one synchronisation, of the query's stream: L, and the chained
            L, R = torch.stack([plane_loops[n], (order >= 0).sum()]).tolist()   # rows (the entries of order that were written)
        loop_offsets, closed = loop_offsets[:L + 1], closed[:L]
    return PlaneLoopsOf(nxt, order, plane_loops, loop_offsets, closed), R


def plane_loops(scene, planes, slices=None, tile_rows=None, stream=None):
    """PlaneLoops(plane_loops int64 [n + 1], loop_offsets int64 [L + 1], closed uint8 [L], row int64 [R], tri int32 [R], seg float32
    [R, 2, 3]): the cross-sections of the mesh with the n planes of `planes` ([..., 4], flattened row-major) as POLYLINES.  Loop l of
    plane i, plane_loops[i] <= l < plane_loops[i + 1], is entries loop_offsets[l] .. loop_offsets[l + 1] of `tri` and `seg`: the
    crossed triangles and their segments in walking order, each segment's q1 the next one's q0 on the bits; its points are
    seg[loop_offsets[l]:loop_offsets[l + 1], 0], a closed loop (closed[l] == 1) returns to the first and an open one ends in the
    last segment's q1.  `row` is the row of plane_section's answer that each entry came from.  Segments of zero length are left out.
    On a closed, consistently wound mesh every loop is closed, outer loops run counter-clockwise seen from the side the plane's
    normal points to and holes clockwise.  Synchronises the stream twice, for the number of rows and for the number of loops.
    `slices` as for plane_count, `tile_rows` as for plane_loops_of.  MEMORY: the section (28 B per row) and plane_loops_of's arrays
    and scratch (about 90 B per row while the call runs, see there) are allocated here: count the rows with plane_count first where
    memory is tight.  The definition: include/ezrt_plane.h and include/ezrt_plane_loops.h."""
    _check_tile_rows(tile_rows)
    offsets, tri, seg = plane_section(scene, planes, slices=slices, stream=stream)
    lp, R = _plane_loops_of(scene, offsets, seg, None, None, False, tile_rows, stream)
    q = _OnStream(scene, planes, stream)
    with q.on():
        row = lp.order[:R]
        out = PlaneLoops(lp.plane_loops, lp.loop_offsets, lp.closed, row, tri[row], seg[row])
    q.done(tri, seg, lp.order, *out)
    return out


def loop_measures(loops, planes):
    """(length, area), float64 [L]: of every loop of `loops` (a PlaneLoops of these `planes`) the sum of its segments' lengths
    |q1 - q0| and the signed area 1/2 sum n^ . (q0 x q1) about the plane's unit normal -- the area enclosed by a closed loop,
    positive for a loop that runs counter-clockwise seen from the normal's side (an outer boundary) and negative for a hole, so that
    a plane's areas add up to its cross-section; of an open loop the area is that of the fan from the origin and means little.  Plain
    float64 torch expressions on the current stream: NOT pinned on the bits (the order of a sum is the library's)."""
    _check_planes(planes)
    seg = loops.seg.to(torch.float64)
    dev = seg.device
    L = loops.closed.shape[0]
    sizes = loops.loop_offsets[1:] - loops.loop_offsets[:-1]
    loop_of = torch.repeat_interleave(torch.arange(L, device=dev), sizes, output_size=seg.shape[0])
    per_plane = loops.plane_loops[1:] - loops.plane_loops[:-1]
    plane_of = torch.repeat_interleave(torch.arange(per_plane.shape[0], device=dev), per_plane, output_size=L)
    nrm = planes.reshape(-1, 4)[:, :3].to(torch.float64)
    nrm = (nrm / nrm.square().sum(1, keepdim=True).sqrt())[plane_of][loop_of]
    q0, q1 = seg[:, 0], seg[:, 1]
    length = torch.zeros(L, dtype=torch.float64, device=dev).index_add_(0, loop_of, (q1 - q0).square().sum(1).sqrt())
    area = torch.zeros(L, dtype=torch.float64, device=dev).index_add_(0, loop_of, 0.5 * (torch.linalg.cross(q0, q1) * nrm).sum(1))
    return length, area


def mesh_topology(scene, components=True, mult=False, stream=None):
    """MeshTopology(twin int32 [n_tri, 3], edge_class uint8 [n_tri, 3], neighbours int32 [n_tri, 3], mult int32 [n_tri, 3] or None,
    root int32 [n_tri], component int32 [n_tri], comp_root int32 [C], comp_size int32 [C], comp_flags uint8 [C], summary int64 [8],
    closed bool, oriented bool): the topology of the scene's triangles as they are stored, vertices compared by value on the bits
    (-0 is +0).  twin[t, e] is the half-edge 3 t' + e' paired with edge e of triangle t (from its vertex e to vertex (e + 1) % 3) or
    -1, neighbours[t, e] = t' or -1, edge_class[t, e] is 0 for a triangle that does not take part (a non-finite coordinate, two
    equal vertices), 1 BOUNDARY, 2 MANIFOLD, 3 FLIPPED (the two neighbours are wound inconsistently), 4 NONMANIFOLD (three or more
    triangles on the edge), and mult (mult=True) the number of triangles on the edge.  root[t] is the lowest id of the triangles
    connected with t across edges and component[t] its number 0 .. C - 1 in ascending order of the roots (-1 for a triangle that
    does not take part); comp_root, comp_size and comp_flags (bit 0 / 1 / 2: the component has a BOUNDARY / FLIPPED / NONMANIFOLD
    edge) describe the components.  summary is [triangles taking part, edges, BOUNDARY, MANIFOLD, FLIPPED, NONMANIFOLD edges, C,
    largest multiplicity].  `closed` (no BOUNDARY and no NONMANIFOLD edge) is what inside and signed_distance assume, `closed and
    oriented` (no FLIPPED edge either) what plane_loops needs for closed loops and winding_number for a sign.  With
    components=False the union-find is not run: root .. comp_flags are None and summary[6] is 0.  The tensors are on the current
    device (the scene's, when it was created there).  Synchronises the stream once, to read the summary.  After a refit the topology
    can change: call again.  MEMORY: the library's scratch, ezrt_topology_work_bytes(n_tri), about 100 B per triangle, is allocated
    here and freed to torch's allocator when the stream is done with it.  The definition: include/ezrt_topology.h."""
    if not isinstance(components, bool) or not isinstance(mult, bool):
        raise ValueError("components and mult must be bools")
    lib = _scene_lib(scene, _abi.TOPOLOGY_ABI)
    n = scene.stats()["n_tri"]
    dev = torch.device("cuda", torch.cuda.current_device())
    q = _OnStream(scene, dev, stream)
    work_bytes = int(lib.ezrt_topology_work_bytes(n))
    work, summary = q.scratch(dev, work_bytes)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    with q.on():
        twin, cls = i32(n, 3), torch.empty((n, 3), dtype=torch.uint8, device=dev)
        mu = i32(n, 3) if mult else None
        root, comp, croot, csize = (i32(n), i32(n), i32(n), i32(n)) if components else (None,) * 4
        cflags = torch.empty((n,), dtype=torch.uint8, device=dev) if components else None
    if n > 0:
        q.call(lib.ezrt_mesh_topology_device, twin, cls, mu, root, comp, croot, csize, cflags, summary, work, work_bytes)
    with q.on():
        nb = torch.where(twin >= 0, torch.div(twin, 3, rounding_mode="floor"), twin)
        sm = summary.tolist()                                        # the one synchronisation, of the query's stream
        if components:
            croot, csize, cflags = croot[:sm[6]], csize[:sm[6]], cflags[:sm[6]]
    q.done(twin, cls, mu, root, comp, croot, csize, cflags, summary, nb)
    return MeshTopology(twin, cls, nb, mu, root, comp, croot, csize, cflags, summary, sm[2] == 0 and sm[5] == 0, sm[4] == 0 and sm[5] == 0)


def mesh_topology_at(scene, tri_a, edge_a, tri_b, stream=None):
    """(shared int8 tri_a.shape, opposite int8 tri_a.shape): mesh_topology's rule for pairs already held.  For edge edge_a[...] (0, 1
    or 2) of triangle tri_a[...], shared is the edge of triangle tri_b[...] that joins the same two vertices by value, or -1, and
    opposite is 1 when the two run in opposite directions (consistent windings), 0 when they run the same way, -1 without a shared
    edge.  The three are contiguous int32 GPU tensors of one shape.  An id that is no triangle of the scene, an edge outside 0 .. 2
    and a triangle that does not take part give (-1, -1)."""
    _tensor("tri_a", tri_a, torch.int32)
    _tensor("edge_a", edge_a, torch.int32, shape=tri_a.shape, device=tri_a.device)
    _tensor("tri_b", tri_b, torch.int32, shape=tri_a.shape, device=tri_a.device)
    lib = _scene_lib(scene, _abi.TOPOLOGY_ABI)
    n = _count(tri_a, 1, "pairs")
    shared = torch.empty(tuple(tri_a.shape), dtype=torch.int8, device=tri_a.device)
    opposite = torch.empty(tuple(tri_a.shape), dtype=torch.int8, device=tri_a.device)
    if n > 0:
        _OnStream(scene, tri_a, stream).run(lib.ezrt_mesh_topology_at_device, tri_a, edge_a, tri_b, n, shared, opposite)
    return shared, opposite


def mesh_weld(scene, flags=True, stream=None):
    """MeshWeld(vertex int32 [n_tri, 3], vert_corner int32 [V], star_offsets int32 [V + 1], star int32 [L], fans int32 [V] or None,
    vert_flags uint8 [V] or None, summary int64 [8], n_vert int, manifold_vertices bool): the scene's triangles as an indexed mesh,
    vertices compared by value on the bits (-0 is +0), as mesh_topology compares them.  vertex[t, k] is the number 0 .. V - 1 of stored
    vertex k of triangle t, or -1 for a triangle that does not take part (a non-finite coordinate, two equal vertices); vertices are
    numbered by their lowest corner 3 t + k, which is vert_corner[v].  star[star_offsets[v] : star_offsets[v + 1]] is the corners
    that are vertex v, ascending.  fans[v] is the number of cones of triangles that meet at v (1 on an ordinary vertex) and
    vert_flags[v] has bit 0 set on the border, bit 1 at an edge of three or more triangles, bit 2 where fans[v] > 1.  summary is
    [corners taking part, V, largest valence, vertices with bit 0, bit 1, bit 2, 0, 0]; n_vert is V and manifold_vertices says that no
    vertex has bit 2: with mesh_topology's `closed` the mesh is a closed 2-manifold.  With flags=False fans and vert_flags are None,
    the three counts are 0 and manifold_vertices is None.  The trimmed tensors are views of arrays of the full size, which is what
    vertex_normals takes.  The tensors are on the current device (the scene's, when it was created there).  Synchronises the
    stream once, to read the summary.  The weld is taken by value: it holds for every refit that moves vertices and keeps which
    corners coincide.  MEMORY: the library's scratch, ezrt_weld_work_bytes(n_tri), up to 168 B per triangle, is allocated here and
    freed to torch's allocator when the stream is done with it.  The definition: include/ezrt_vertices.h."""
    if not isinstance(flags, bool):
        raise ValueError("flags must be a bool")
    lib = _scene_lib(scene, _abi.WELD_ABI)
    n = scene.stats()["n_tri"]
    dev = torch.device("cuda", torch.cuda.current_device())
    q = _OnStream(scene, dev, stream)
    work_bytes = int(lib.ezrt_weld_work_bytes(n))
    work, summary = q.scratch(dev, work_bytes)
    i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
    with q.on():
        vertex, corner, offsets, star = i32(3 * n).view(n, 3), i32(3 * n), i32(3 * n + 1), i32(3 * n)
        fans = i32(3 * n) if flags else None
        vflags = torch.empty((3 * n,), dtype=torch.uint8, device=dev) if flags else None
        if n == 0:
            offsets.zero_()
    if n > 0:
        q.call(lib.ezrt_mesh_weld_device, vertex, corner, offsets, star, fans, vflags, summary, work, work_bytes)
    q.done(vertex, corner, offsets, star, fans, vflags, summary)
    with q.on():
        sm = summary.tolist()                                        # the one synchronisation, of the query's stream
    L, V = sm[0], sm[1]
    return MeshWeld(vertex, corner[:V], offsets[:V + 1], star[:L], fans[:V] if flags else None, vflags[:V] if flags else None, summary, V,
                    sm[5] == 0 if flags else None)


def mesh_weld_at(scene, corner_a, corner_b, stream=None):
    """same int8 corner_a.shape: mesh_weld's rule for pairs already held.  1 when corners corner_a[...] and corner_b[...] (3 t + k:
    stored vertex k of triangle t) are one vertex by value, 0 when they are two, -1 when either is no corner of the scene or belongs
    to a triangle that does not take part.  The two are contiguous int32 GPU tensors of one shape."""
    _tensor("corner_a", corner_a, torch.int32)
    _tensor("corner_b", corner_b, torch.int32, shape=corner_a.shape, device=corner_a.device)
    lib = _scene_lib(scene, _abi.WELD_ABI)
    n = _count(corner_a, 1, "pairs")
    same = torch.empty(tuple(corner_a.shape), dtype=torch.int8, device=corner_a.device)
    if n > 0:
        _OnStream(scene, corner_a, stream).run(lib.ezrt_mesh_weld_at_device, corner_a, corner_b, n, same)
    return same


def _weld_array(name, x, size, dev, q, dtype=torch.int32):
    """x, an int32 array of a weld (or its uint8 flags), as the `size` entries the C call may read: x itself where that much memory
    lies behind it (the trimmed views of mesh_weld), else a zero-padded copy made on the query's stream"""
    _tensor(name, x, dtype, device=dev)
    if x.numel() >= size or (x.untyped_storage().nbytes() - x.storage_offset() * x.element_size()) >= size * x.element_size():
        return x
    with q.on():
        full = torch.zeros((size,), dtype=dtype, device=dev)
        full[:x.numel()] = x.reshape(-1)
    return full


def vertex_normals(scene, tri36, weld, stream=None):
    """tri36, with floats 9-17 of every row (n1 n2 n3) overwritten by the smooth normals of its OWN positions (floats 0-8) over the
    stars of `weld` (a MeshWeld of this scene, or any object with vertex, star_offsets and star): the reference's readObj(...,
    smoothNormal=True) -- face normals summed in fp32 from +0 in ascending corner order, normalised -- on the bits wherever the
    mesh's vertices are distinct by value; a corner of a triangle that does not take part gets its face normal.  tri36 is the
    caller's contiguous float32 [n_tri, 36] GPU tensor, the one about to go into refit.refit; nothing else of it is written.  Weld once,
    then per step: deform, vertex_normals, refit, render.  Does not synchronise.  The definition: include/ezrt_vertices.h."""
    lib = _scene_lib(scene, _abi.WELD_ABI)
    n = scene.stats()["n_tri"]
    _tensor("tri36", tri36, torch.float32, shape=(n, 36))
    dev = tri36.device
    q = _OnStream(scene, tri36, stream)
    vertex = _weld_array("weld.vertex", weld.vertex, 3 * n, dev, q)
    offsets = _weld_array("weld.star_offsets", weld.star_offsets, 3 * n + 1, dev, q)
    star = _weld_array("weld.star", weld.star, 3 * n, dev, q)
    if vertex.numel() != 3 * n:
        raise ValueError("weld.vertex must have 3 * n_tri = %d entries, not %d" % (3 * n, vertex.numel()))
    if n == 0:
        return tri36
    work_bytes = int(lib.ezrt_vertex_normals_work_bytes(n))
    work = q.scratch(dev, work_bytes, summary=False)[0]
    q.run(lib.ezrt_vertex_normals_device, tri36, n, vertex, offsets, star, work, work_bytes)
    return tri36


def indexed_mesh(weld, tri36):
    """(positions float32 [V, 3], faces int32 [n_tri, 3]): the indexed mesh of a weld, by plain torch indexing on the current stream.
    positions[v] is read from tri36 (float32 [n_tri, 36], or [n_tri, 9]: the rows the weld was made of, or moved ones) at corner
    vert_corner[v]; faces is weld.vertex, -1 in the rows of triangles that do not take part."""
    if not isinstance(tri36, torch.Tensor) or tri36.dim() != 2 or tri36.shape[1] not in (9, 36) or tri36.shape[0] != weld.vertex.shape[0]:
        raise ValueError("tri36 must be a tensor of shape [n_tri, 36] or [n_tri, 9] with the weld's n_tri")
    corner = weld.vert_corner.to(torch.int64)
    positions = tri36[:, :9].reshape(-1, 3)[corner]
    return positions, weld.vertex


def euler_characteristic(weld, topo):
    """V - E + F of the triangles that take part: weld.summary[1] - topo.summary[1] + topo.summary[0] (2 for a sphere, 0 for a
    torus).  Reads the two summaries (a synchronisation of the current stream)."""
    w, t = weld.summary.tolist(), topo.summary.tolist()
    if w[0] != 3 * t[0]:
        raise ValueError("the weld and the topology are not of the same triangles (%d live corners, %d live triangles)" % (w[0], t[0]))
    return w[1] - t[1] + t[0]


def mesh_orient(scene, topo=None, outward=True, stream=None):
    """MeshOrient(flip uint8 [n_tri], patch_root int32 [n_tri], patch int32 [n_tri], proot int32 [P], psize int32 [P], pflags uint8 [P],
    vol6 int64 [P], summary int64 [8], n_patch int, orientable bool, scale int): a consistent winding of the scene's triangles as
    they are stored.  `topo` is a MeshTopology of this scene (or any object with twin and edge_class); with topo=None
    mesh_topology(scene, components=False) is run on the same stream first.  Triangles joined across MANIFOLD and FLIPPED edges form
    a patch; patch_root[t] is the lowest id of t's patch and patch[t] its number 0 .. P - 1 in ascending order of the roots (-1 for a
    triangle that does not take part); flip[t] is 1 where the triangle has to be reversed for its patch to be wound like the patch's
    root -- or, with outward=True on a closed orientable patch, so that the patch faces outward.  pflags[p] has _abi.PATCH_OPEN,
    PATCH_NONORIENTABLE (a Moebius band: flip is 0 on all of it), PATCH_REWOUND (some flip is 1) and PATCH_INWARD (closed, orientable
    and of negative volume as stored); vol6[p] * 2 ** scale / 6 is the patch's signed volume (patch_volume).  summary is [triangles
    taking part, P, orientable patches, closed patches, flips, INWARD patches, scale, 0]; `orientable` says that every patch is: the
    mesh can be made consistently wound, by query.rewind and a refit.  The tensors are on the device of topo's.  Synchronises the
    stream once, to read the summary.  The topology is taken by value: after a refit that changes windings make both again.  MEMORY:
    the library's scratch, ezrt_orient_work_bytes(n_tri), 32 B per triangle, is allocated here and freed to torch's allocator when the
    stream is done with it.  The definition: include/ezrt_orient.h."""
    if not isinstance(outward, bool):
        raise ValueError("outward must be a bool")
    lib = _scene_lib(scene, _abi.ORIENT_ABI)
    n = scene.stats()["n_tri"]
    if topo is None:
        topo = mesh_topology(scene, components=False, stream=stream)
    twin = _tensor("topo.twin", topo.twin, torch.int32)
    cls = _tensor("topo.edge_class", topo.edge_class, torch.uint8, device=twin.device)
    if twin.numel() != 3 * n or cls.numel() != 3 * n:
        raise ValueError("topo.twin and topo.edge_class must have 3 * n_tri = %d entries, not %d and %d" % (3 * n, twin.numel(), cls.numel()))
    dev = twin.device
    q = _OnStream(scene, twin, stream)
    work_bytes = int(lib.ezrt_orient_work_bytes(n))
    work, summary = q.scratch(dev, work_bytes)
    i32 = lambda: torch.empty((n,), dtype=torch.int32, device=dev)
    u8 = lambda: torch.empty((n,), dtype=torch.uint8, device=dev)
    with q.on():
        flip, root, patch, proot, psize, pflags = u8(), i32(), i32(), i32(), i32(), u8()
        vol6 = torch.empty((n,), dtype=torch.int64, device=dev)
    if n > 0:
        q.call(lib.ezrt_mesh_orient_device, twin, cls, 1 if outward else 0, flip, root, patch, proot, psize, pflags, vol6, summary, work,
               work_bytes)
    q.done(twin, cls, flip, root, patch, proot, psize, pflags, vol6, summary)
    with q.on():
        sm = summary.tolist()                                        # the one synchronisation, of the query's stream
    k = sm[1]
    return MeshOrient(flip, root, patch, proot[:k], psize[:k], pflags[:k], vol6[:k], summary, k, sm[2] == sm[1], sm[6])


def rewind(scene, tri36, orient, stream=None):
    """tri36, with the rows that `orient` (a MeshOrient of this scene, or any object with flip) marks reversed in place: p2 <-> p3
    (floats 3-5 and 6-8) and n2 <-> n3 (floats 12-14 and 15-17); a normal travels with its vertex.  tri36 is the caller's contiguous
    float32 [n_tri, 36] GPU tensor, the one about to go into refit.refit; nothing else of it is written, and a second call restores it.
    For smooth normals of the new winding call vertex_normals afterwards.  Does not synchronise.  The definition:
    include/ezrt_orient.h."""
    lib = _scene_lib(scene, _abi.ORIENT_ABI)
    n = scene.stats()["n_tri"]
    _tensor("tri36", tri36, torch.float32, shape=(n, 36))
    flip = _tensor("orient.flip", orient.flip, torch.uint8, shape=(n,), device=tri36.device)
    if n > 0:
        _OnStream(scene, tri36, stream).run(lib.ezrt_rewind_device, tri36, n, flip)
    return tri36


def patch_volume(orient):
    """float64 [P]: the signed volume of every patch of a MeshOrient in scene units, vol6 * 2.0 ** scale / 6, on vol6's device and
    torch's current stream.  Exact wherever the header says so (small integer coordinates); the volume of an open patch depends on
    the origin."""
    if not isinstance(orient.vol6, torch.Tensor) or orient.vol6.dtype != torch.int64 or not isinstance(orient.scale, int):
        raise TypeError("orient must be a MeshOrient: vol6 an int64 tensor, scale an int")
    v = orient.vol6.to(torch.float64) * 2.0 ** orient.scale                    # exact: a power of two
    return v / torch.full_like(v, 6.0)                                         # (a tensor divisor: torch multiplies by the reciprocal of a scalar one)


def mesh_boundary(scene, topo=None, area=True, stream=None):
    """MeshBoundary(next int32 [3 n_tri], loop int32 [3 n_tri], pos int32 [3 n_tri], order int32 [B], loop_offsets int32 [L + 1],
    lflags uint8 [L], area2 int64 [L, 3] or None, summary int64 [8], n_boundary int, n_loops int, closed bool, scale int): the
    boundary of the scene's triangles as they are stored, as ordered loops of half-edges.  `topo` is a MeshTopology of this scene (or
    any object with twin and edge_class); with topo=None mesh_topology(scene, components=False) is run on the same stream first.
    Half-edge h = 3 t + e runs from vertex e of triangle t to vertex (e + 1) % 3; next[h] is the boundary half-edge that follows a
    boundary half-edge h (-1: none, or h is no boundary), found by rotating about the end vertex across MANIFOLD edges; loop[h] and
    pos[h] are its loop and its position in it (-1 for other half-edges); order[loop_offsets[l] : loop_offsets[l + 1]] are the
    half-edges of loop l in order, loops numbered by ascending head (of a cycle its lowest half-edge); lflags[l] has _abi.LOOP_CLOSED
    where the loop is a cycle -- a chain that ends at a FLIPPED or NONMANIFOLD edge is an open path: orient and rewind first.  With
    area=True, area2[l] * 2 ** scale / 2 is the vector area of loop l (loop_area).  summary is [B, L, closed loops, the longest loop,
    boundary half-edges without a successor, scale, 0, 0]; `closed` says that every loop is a cycle.  The tensors are on the device of
    topo's.  Synchronises the stream once, to read the summary.  The topology is taken by value: after a refit make both again.
    MEMORY: the library's scratch, ezrt_boundary_work_bytes(n_tri), 132 B per triangle, is allocated here and freed to torch's
    allocator when the stream is done with it.  The definition: include/ezrt_boundary.h."""
    if not isinstance(area, bool):
        raise ValueError("area must be a bool")
    lib = _scene_lib(scene, _abi.BOUNDARY_ABI)
    n = scene.stats()["n_tri"]
    if topo is None:
        topo = mesh_topology(scene, components=False, stream=stream)
    twin = _tensor("topo.twin", topo.twin, torch.int32)
    cls = _tensor("topo.edge_class", topo.edge_class, torch.uint8, device=twin.device)
    if twin.numel() != 3 * n or cls.numel() != 3 * n:
        raise ValueError("topo.twin and topo.edge_class must have 3 * n_tri = %d entries, not %d and %d" % (3 * n, twin.numel(), cls.numel()))
    dev = twin.device
    q = _OnStream(scene, twin, stream)
    work_bytes = int(lib.ezrt_boundary_work_bytes(n))
    work, summary = q.scratch(dev, work_bytes)
    H = 3 * n
    i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
    with q.on():
        nxt, loop, pos, order, offsets = i32(H), i32(H), i32(H), i32(H), i32(H + 1)
        lflags = torch.empty((H,), dtype=torch.uint8, device=dev)
        area2 = torch.empty((H, 3), dtype=torch.int64, device=dev) if area else None
        offsets[:1] = 0                                                        # (a scene without triangles: L = 0, B = 0)
    if n > 0:
        q.call(lib.ezrt_mesh_boundary_device, twin, cls, nxt, loop, pos, order, offsets, lflags, area2, summary, work, work_bytes)
    q.done(twin, cls, nxt, loop, pos, order, offsets, lflags, area2, summary)
    with q.on():
        sm = summary.tolist()                                        # the one synchronisation, of the query's stream
    B, L = sm[0], sm[1]
    return MeshBoundary(nxt, loop, pos, order[:B], offsets[:L + 1], lflags[:L], area2[:L] if area else None, summary, B, L, sm[2] == sm[1],
                        sm[5])


def _boundary(boundary):
    if not isinstance(boundary, MeshBoundary) or not all(isinstance(x, torch.Tensor) for x in boundary[:6] + (boundary.summary,)):
        raise TypeError("boundary must be a MeshBoundary of query.mesh_boundary")
    return boundary


def boundary_points(boundary, tri36):
    """float32 [B, 3]: the start points of the boundary half-edges in `order`, loop after loop -- points[loop_offsets[l] :
    loop_offsets[l + 1]] is the polygon of loop l.  tri36 is the rows the scene was made of, a float32 [n_tri, 36] GPU tensor on the
    boundary's device.  A gather on torch's current stream."""
    b = _boundary(boundary)
    n = b.next.numel() // 3
    _tensor("tri36", tri36, torch.float32, shape=(n, 36), device=b.order.device)
    return tri36[:, :9].reshape(-1, 3)[b.order.to(torch.int64)]


def loop_area(boundary):
    """float64 [L, 3]: the vector area of every loop of a MeshBoundary made with area=True, area2 * 2.0 ** scale / 2, on area2's
    device and torch's current stream.  Of a closed loop it is the vector area of any surface that spans it, exact wherever the header
    says so (small integer coordinates); of an open path it depends on the origin."""
    if not isinstance(boundary, MeshBoundary) or not isinstance(boundary.area2, torch.Tensor) or boundary.area2.dtype != torch.int64 or \
            not isinstance(boundary.scale, int):
        raise TypeError("boundary must be a MeshBoundary made with area=True: area2 an int64 tensor, scale an int")
    return boundary.area2.to(torch.float64) * 2.0 ** (boundary.scale - 1)     # exact: a power of two


def cap_rows(scene, tri36, boundary, stream=None):
    """float32 [n_cap, 36]: the triangles that close the closed loops of `boundary` (a MeshBoundary of this scene), a fan from each
    loop's head, k - 2 triangles for a loop of k edges, in row order; torch.cat([tri36, cap]) is the closed mesh, for a new scene.
    Positions and materials are read from tri36, the caller's contiguous float32 [n_tri, 36] GPU rows: each new triangle has the face
    normal at its three corners and the material of the triangle it closes against.  A fan closes a hole topologically; a non-planar
    or non-convex hole gets a folded cap.  Synchronises (the compaction of the valid rows).  The definition: include/ezrt_boundary.h."""
    lib = _scene_lib(scene, _abi.BOUNDARY_ABI)
    n = scene.stats()["n_tri"]
    _tensor("tri36", tri36, torch.float32, shape=(n, 36))
    b = _boundary(boundary)
    dev = tri36.device
    H = 3 * n
    for name, x, dt, k in (("next", b.next, torch.int32, H), ("loop", b.loop, torch.int32, H), ("pos", b.pos, torch.int32, H),
                           ("order", b.order, torch.int32, b.n_boundary), ("loop_offsets", b.loop_offsets, torch.int32, b.n_loops + 1),
                           ("lflags", b.lflags, torch.uint8, b.n_loops), ("summary", b.summary, torch.int64, 8)):
        _tensor("boundary." + name, x, dt, shape=(k,), device=dev)
    if not 0 <= b.n_loops <= b.n_boundary <= H:
        raise ValueError("boundary is not of this scene: %d loops, %d boundary half-edges, %d half-edges" % (b.n_loops, b.n_boundary, H))
    B = b.n_boundary
    q = _OnStream(scene, tri36, stream)
    with q.on():
        # the library takes arrays of the full size; order, loop_offsets and lflags were cut to what was written
        room = lambda x: x.untyped_storage().nbytes() // x.element_size() - x.storage_offset()
        pad = lambda x, k: x if x.numel() and room(x) >= k else torch.cat([x, torch.zeros((k - x.numel(),), dtype=x.dtype, device=dev)])
        order, offsets, lflags = pad(b.order, H), pad(b.loop_offsets, H + 1), pad(b.lflags, H)
        cap = torch.empty((H, 36), dtype=torch.float32, device=dev)
        valid = torch.zeros((H,), dtype=torch.uint8, device=dev)
    if n > 0:
        q.call(lib.ezrt_cap_rows_device, tri36, n, order, b.loop, b.pos, offsets, lflags, b.summary, cap, valid)
    with q.on():
        out = cap[:B][valid[:B] != 0]
    q.done(tri36, order, b.loop, b.pos, offsets, lflags, b.summary, out)
    return out


def clip_rows(scene, tri36, plane, src=True, stream=None):
    """ClipRows(rows float32 [T, 36], src int32 [T] or None, cut_edge int8 [T] or None, summary int64 [8], n_rows int): the part of
    the caller's triangle rows `tri36` (a contiguous float32 [n, 36] GPU tensor: p1 p2 p3, n1 n2 n3, material -- the rows a scene is
    made of) on the side a x + b y + c z >= d of `plane`, a float32 [4] tensor (a, b, c, d) on tri36's device or a sequence of four
    numbers.  A row with every vertex on that side (a vertex ON the plane counts) is kept on the bits, a row on the other side is
    dropped, and a row the plane crosses is replaced by one or two triangles with the winding of the row, whose new vertices are the
    points of plane_section on the bits, with the row's normals interpolated along the edge (not renormalised) and its material.
    rows are in ascending source row; with src=True, src[r] is the source row of output row r and cut_edge[r] the edge (0, 1, 2:
    from vertex e to vertex (e + 1) % 3) of output row r that the cut made, -1 where there is none (cut_segments gathers them: they
    are plane_section's segments of the rows that were cut; on a closed, consistently wound mesh the boundary of a scene of `rows` is
    the section).  summary is [T, rows kept whole,
    rows cut, finite rows dropped, rows with a non-finite coordinate (dropped), cut edges, plane live, 0]; n_rows is n.  A plane with a
    non-finite entry or a zero normal keeps nothing.  `scene` supplies the library and the device only: the rows need not be the
    scene's, and the rows of one call are the input of the next -- six calls trim a mesh to a box.  To go on, make a scene of
    `rows` and run mesh_topology, mesh_boundary and cap_rows on it: torch.cat([rows, cap]) is the closed half.  Synchronises the
    stream once, to read T; rows, src and cut_edge are allocated to exactly T rows.  MEMORY besides the result: 8 B per input row of
    offsets and the library's scratch, ezrt_clip_work_bytes(n), freed to torch's allocator when the stream is done with them.  The
    definition: include/ezrt_clip.h."""
    if not isinstance(src, bool):
        raise ValueError("src must be a bool")
    lib = _scene_lib(scene, _abi.CLIP_ABI)
    _tensor("tri36", tri36, torch.float32, last=36)
    if tri36.dim() != 2:
        raise ValueError("tri36 must have shape [n, 36], not %s" % (tuple(tri36.shape),))
    n = tri36.shape[0]
    if n > (2**31 - 1) // 2:
        raise ValueError("at most (2^31 - 1) / 2 rows per call")
    dev = tri36.device
    q = _OnStream(scene, tri36, stream)
    if isinstance(plane, torch.Tensor):
        _tensor("plane", plane, torch.float32, shape=(4,), device=dev)
    else:
        p = [float(x) for x in plane]
        if len(p) != 4:
            raise ValueError("plane must have four entries (a, b, c, d), not %d" % len(p))
        with q.on():
            plane = torch.tensor(p, dtype=torch.float64).to(torch.float32).to(dev)
    work_bytes = int(lib.ezrt_clip_work_bytes(n))
    work, summary = q.scratch(dev, work_bytes)
    with q.on():
        offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    if n > 0:
        q.call(lib.ezrt_clip_count_device, tri36, n, plane, offsets, summary, work, work_bytes)
    with q.on():
        T = int(offsets[n].item())                                   # the one synchronisation, of the query's stream
        rows = torch.empty((T, 36), dtype=torch.float32, device=dev)
        srcs = torch.empty((T,), dtype=torch.int32, device=dev) if src else None
        cut = torch.empty((T,), dtype=torch.int8, device=dev) if src else None
    if n > 0 and T > 0:
        q.call(lib.ezrt_clip_rows_device, tri36, n, plane, offsets, T, rows, srcs, cut)
    q.done(tri36, plane, summary, rows, srcs, cut)
    return ClipRows(rows, srcs, cut, summary, n)


def cut_segments(clip):
    """float32 [n_cut, 2, 3]: the cut edges of a ClipRows made with src=True, start to end, in row order -- of every output row r
    with cut_edge[r] = e >= 0 its vertices e and (e + 1) % 3.  Each is plane_section's segment q0 -> q1 of its source row for the same
    plane, on the bits and in direction; a source row that emits cut pieces has exactly one.  A gather on torch's current stream."""
    if not isinstance(clip, ClipRows) or not isinstance(clip.rows, torch.Tensor) or not isinstance(clip.cut_edge, torch.Tensor):
        raise TypeError("clip must be a ClipRows of query.clip_rows made with src=True")
    _tensor("clip.rows", clip.rows, torch.float32, last=36)
    _tensor("clip.cut_edge", clip.cut_edge, torch.int8, shape=(clip.rows.shape[0],), device=clip.rows.device)
    r = torch.nonzero(clip.cut_edge >= 0).reshape(-1)
    e = clip.cut_edge[r].to(torch.int64)
    v = clip.rows[:, :9].reshape(-1, 3, 3)
    return torch.stack([v[r, e], v[r, (e + 1) % 3]], dim=1)


def subdivide_rows(scene, tri36, mode="midpoint", topo=None, weld=None, stream=None):
    """SubdivRows(rows float32 [4 n, 36], summary int64 [8], n_rows int): every row t of the caller's triangle rows `tri36` (a
    contiguous float32 [n, 36] GPU tensor: p1 p2 p3, n1 n2 n3, material -- the rows a scene is made of) split in four, rows 4 t .. 4 t + 3
    of `rows`: the three corner pieces (P0 E0 E2), (E0 P1 E1), (E2 E1 P2) and the middle one (E0 E1 E2), each with the winding and the
    material of its row.  mode="midpoint" keeps every corner and puts the edge points at (a + b) * 0.5f -- scenes.subdivide on the
    bits -- with the corner normals kept and averaged along the edges.  mode="loop" is Loop's scheme with Warren's weights: smooth
    vertices and interior edges are averaged over their neighbours, border vertices and edges along the border, and vertices on a
    non-manifold edge or pinched stay where they are; every output row gets its face normal (for smooth ones: a scene of `rows`,
    mesh_weld, vertex_normals).  It requires `topo`, a MeshTopology, and `weld`, a MeshWeld made with flags=True, of a scene of these
    rows (or any objects with twin, edge_class and vertex, star_offsets, star, vert_flags); both are taken by value: the rows may have
    been moved since, as long as the same corners coincide.  summary is [4 n, corners smoothed, corners on a border, corners kept,
    interior half-edges, midpoint half-edges, mode, 0]; n_rows is n.  `scene` supplies the library and the device only: the rows need
    not be the scene's, and the rows of one call are the input of the next (Loop mode: with a topology and a weld of a scene of
    them).  Does not synchronise: the size of the answer is known.  MEMORY besides the result: the library's scratch,
    ezrt_subdivide_work_bytes(n, mode) -- 8 B, in Loop mode 48 B per input row -- freed to torch's allocator when the stream is
    done with it.  The definition: include/ezrt_subdivide.h."""
    if mode not in ("midpoint", "loop"):
        raise ValueError('mode must be "midpoint" or "loop"')
    loop = mode == "loop"
    lib = _scene_lib(scene, _abi.SUBDIVIDE_ABI)
    _tensor("tri36", tri36, torch.float32, last=36)
    if tri36.dim() != 2:
        raise ValueError("tri36 must have shape [n, 36], not %s" % (tuple(tri36.shape),))
    n = tri36.shape[0]
    if n > (2**31 - 1) // 12:
        raise ValueError("at most (2^31 - 1) / 12 rows per call")
    dev = tri36.device
    q = _OnStream(scene, tri36, stream)
    arrays = (None,) * 6
    if loop:
        if topo is None or weld is None or getattr(weld, "vert_flags", None) is None:
            raise ValueError('mode="loop" needs topo, a MeshTopology, and weld, a MeshWeld made with flags=True')
        twin = _tensor("topo.twin", topo.twin, torch.int32, device=dev)
        cls = _tensor("topo.edge_class", topo.edge_class, torch.uint8, device=dev)
        if twin.numel() != 3 * n or cls.numel() != 3 * n:
            raise ValueError("topo.twin and topo.edge_class must have 3 * n = %d entries, not %d and %d" % (3 * n, twin.numel(), cls.numel()))
        vertex = _weld_array("weld.vertex", weld.vertex, 3 * n, dev, q)
        if vertex.numel() != 3 * n:
            raise ValueError("weld.vertex must have 3 * n = %d entries, not %d" % (3 * n, vertex.numel()))
        offsets = _weld_array("weld.star_offsets", weld.star_offsets, 3 * n + 1, dev, q)
        star = _weld_array("weld.star", weld.star, 3 * n, dev, q)
        vflags = _weld_array("weld.vert_flags", weld.vert_flags, 3 * n, dev, q, torch.uint8)
        arrays = (twin, cls, vertex, offsets, star, vflags)
    elif topo is not None or weld is not None:
        raise ValueError('mode="midpoint" takes no topo and no weld')
    code = _abi.SUBDIVIDE_LOOP if loop else _abi.SUBDIVIDE_MIDPOINT
    work_bytes = int(lib.ezrt_subdivide_work_bytes(n, code))
    work, summary = q.scratch(dev, work_bytes)
    with q.on():
        rows = torch.empty((4 * n, 36), dtype=torch.float32, device=dev)
        if n == 0:
            summary[6] = code
    if n > 0:
        q.call(lib.ezrt_subdivide_rows_device, tri36, n, code, *arrays, rows, summary, work, work_bytes)
    q.done(tri36, rows, summary, *arrays)
    return SubdivRows(rows, summary, n)


def decimate_rows(scene, tri36, cell_size, origin=(0, 0, 0), dedup=True, src=True, stream=None):
    """DecimatedRows(rows float32 [T, 36], src int32 [T] or None, cell int32 [n, 3], cell_point float32 [n_cells, 3], summary int64 [8],
    n_rows int): the caller's triangle rows `tri36` (a contiguous float32 [n, 36] GPU tensor: p1 p2 p3, n1 n2 n3, material -- the rows a
    scene is made of) with their vertices CLUSTERED on the uniform grid of cubes of edge `cell_size` that has a corner at `origin`
    (a number and three numbers; both are rounded to float32).  All vertices in one cell become one point -- the mean of their
    positions in the cell's fixed-point coordinates, exact and independent of any order, and per axis the common value itself where
    they all agree, so a vertex alone in its cell does not move and an axis-aligned flat face stays flat.  A row whose three vertices
    fall into three different cells is kept, with the winding and the material of its row and its face normal at all three corners;
    every other row has collapsed and is dropped; with dedup=True, of the rows that come out with the same three cells only the lowest
    is kept (the two faces of a thin plate).  rows are in ascending source row; with src=True, src[r] is the source row of output row
    r.  cell[t] are the cells of row t's three vertices (-1: the row has a non-finite coordinate or lies more than 2^20 cells from
    the origin, and takes no part) and cell_point their points: together the decimated mesh in INDEXED form.  summary is [T,
    collapsed rows, duplicates, rows that take no part, n_cells, cells not moved at all, flags, grid live]; n_rows is n.  A cell_size
    that is not a finite number above zero, or a non-finite origin, keeps nothing.  Clustering does not preserve manifoldness: the
    output of a closed mesh may have non-manifold and boundary edges (mesh_topology says).  `scene` supplies the library and the
    device only: the rows need not be the scene's, and the rows of one call are the input of the next.  Synchronises the stream once,
    to read T; rows and src are allocated to exactly T rows and cell_point is cut to n_cells.  MEMORY besides the result: 8 B per
    input row of offsets, 12 B per corner for the lowest corners and the points of up to 3 n cells, and the library's scratch,
    ezrt_decimate_work_bytes(n) -- between 430 and 830 B per input row, the table is sized for one cell per corner -- freed to
    torch's allocator when the stream is done with them.  The definition: include/ezrt_decimate.h."""
    if not isinstance(src, bool) or not isinstance(dedup, bool):
        raise ValueError("src and dedup must be bools")
    lib = _scene_lib(scene, _abi.DECIMATE_ABI)
    _tensor("tri36", tri36, torch.float32, last=36)
    if tri36.dim() != 2:
        raise ValueError("tri36 must have shape [n, 36], not %s" % (tuple(tri36.shape),))
    n = tri36.shape[0]
    if n > (2**31 - 1) // 3:
        raise ValueError("at most (2^31 - 1) / 3 rows per call")
    o = [float(x) for x in origin]
    if len(o) != 3:
        raise ValueError("origin must have three entries, not %d" % len(o))
    dev = tri36.device
    q = _OnStream(scene, tri36, stream)
    flags = _abi.DECIMATE_DEDUP if dedup else 0
    work_bytes = int(lib.ezrt_decimate_work_bytes(n))
    work, summary = q.scratch(dev, work_bytes)
    with q.on():
        grid = torch.tensor(o + [float(cell_size)], dtype=torch.float64).to(torch.float32).to(dev)
        cell = torch.full((n, 3), -1, dtype=torch.int32, device=dev)
        corner = torch.empty((3 * n,), dtype=torch.int32, device=dev)
        point = torch.empty((3 * n, 3), dtype=torch.float32, device=dev)
        offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        if n == 0:
            summary[6] = flags
            summary[7] = int(bool(torch.isfinite(grid).all()) and float(grid[3]) > 0)
    if n > 0:
        q.call(lib.ezrt_decimate_count_device, tri36, n, grid, flags, cell, corner, point, offsets, summary, work, work_bytes)
    with q.on():
        T, n_cells = (int(x) for x in torch.stack([offsets[n], summary[4]]).tolist())   # the one synchronisation, of the query's stream
        rows = torch.empty((T, 36), dtype=torch.float32, device=dev)
        srcs = torch.empty((T,), dtype=torch.int32, device=dev) if src else None
    if n > 0 and T > 0:
        q.call(lib.ezrt_decimate_rows_device, tri36, n, cell, point, offsets, T, rows, srcs)
    q.done(tri36, cell, point, summary, rows, srcs)
    return DecimatedRows(rows, srcs, cell, point[:n_cells], summary, n)


def _grid_numbers(origin, spacing):
    """(origin, spacing) as three floats each; spacing may be one number"""
    o = [float(x) for x in origin]
    if len(o) != 3:
        raise ValueError("origin must have three entries, not %d" % len(o))
    try:
        h = [float(x) for x in spacing]
    except TypeError:
        h = [float(spacing)] * 3
    if len(h) != 3:
        raise ValueError("spacing must be a number or have three entries, not %d" % len(h))
    return o, h


def _grid_shape(shape):
    d = tuple(int(x) for x in shape)
    if len(d) != 3 or min(d) < 1:
        raise ValueError("shape must be (nz, ny, nx) with every dimension >= 1, not %s" % (tuple(shape),))
    if d[0] * d[1] * d[2] > 2**31 - 1:
        raise ValueError("at most 2^31 - 1 grid vertices per call")
    return d


def grid_points(shape, origin=(0, 0, 0), spacing=1.0, device=None):
    """float32 [nz ny nx, 3]: the positions of the vertices of the regular grid of `shape` = (nz, ny, nx), x fastest -- row
    (k ny + j) nx + i is (ox + i hx, oy + j hy, oz + k hz), every coordinate computed in float64 from the float32 values of `origin`
    (three numbers) and `spacing` (a number or three) with one multiply and one add, then rounded to float32: exactly the positions
    isosurface_rows gives the vertices of a grid with the same origin and spacing (G2 of include/ezrt_isosurface.h).  A field sampled
    at these points and reshaped to `shape` is what isosurface_rows takes; the offset surface of a scene at distance r is
        pts = query.grid_points(shape, origin, spacing, device)
        sd = query.signed_distance(scene, pts)
        off = query.isosurface_rows(scene, sd.dist.reshape(shape), r, origin, spacing)
    On torch's current stream of `device`."""
    nz, ny, nx = _grid_shape(shape)
    o, h = _grid_numbers(origin, spacing)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    g = torch.tensor(o + h, dtype=torch.float64).to(torch.float32).to(torch.float64).to(dev)
    axis = lambda n, a: (torch.arange(n, dtype=torch.float64, device=dev) * g[3 + a] + g[a]).to(torch.float32)
    x, y, z = axis(nx, 0), axis(ny, 1), axis(nz, 2)
    out = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=dev)
    out[..., 0], out[..., 1], out[..., 2] = x[None, None, :], y[None, :, None], z[:, None, None]
    return out.reshape(-1, 3)


def isosurface_rows(scene, values, iso, origin=(0, 0, 0), spacing=1.0, material=None, cell=True, stream=None):
    """IsoRows(rows float32 [T, 36], cell int32 [T] or None, summary int64 [8], shape (nz, ny, nx)): the surface on which the field
    `values` (a contiguous float32 [nz, ny, nx] GPU tensor, x fastest, sampled at grid_points(shape, origin, spacing)) crosses the
    level `iso`, as triangle rows -- the rows a scene is made of: p1 p2 p3, the face normal at all three corners, and `material`
    (None: 18 zeros, or 18 numbers) in floats 18-35.  A vertex with a value below `iso` is inside, as with signed_distance, and the
    normals face the outside.  The method is marching tetrahedra on the Kuhn split of every cell: away from the border of the grid
    and from non-finite values the rows are a closed, consistently wound 2-manifold by value (mesh_topology of a scene of them says
    closed and oriented); where the surface meets the border it is open -- pad the field with one layer of values >= iso to close it.
    rows are in ascending cell, and with cell=True cell[r] is the cell (k (ny - 1) + j) (nx - 1) + i of row r.  summary is [T, cells
    that emit, finite cells that emit nothing, cells with a non-finite value (a hole), blocks of 256 cells that emit, n_cells, grid
    live, 0].  A non-finite iso, origin or spacing, or a spacing that is not above zero, emits nothing.  A grid with a dimension of 1
    has no cells: the library launches nothing and writes no summary then, so this wrapper fills in `grid live` itself, by G1's rule
    restated on the float32 values (the one place outside the library that states it).  Smooth normals: a scene of
    the rows, mesh_weld, vertex_normals.  With values = signed_distance(scene, grid_points(shape, origin, spacing, dev)).dist
    .reshape(shape) and iso = r this is the offset surface of the scene at distance r; with winding_number at iso 0.5 (negated: inside
    is below) a watertight remesh; with torch.minimum / maximum of two fields the union / intersection of two parts.  `scene`
    supplies the library and the device only.  Synchronises the stream once, to read T; rows and cell are allocated to exactly T
    rows.  MEMORY besides the result: 8 B per 256 cells of offsets and the library's scratch, ezrt_iso_work_bytes(nx, ny, nz) -- 8 B
    per 2048 * 256 cells -- freed to torch's allocator when the stream is done with them.  The definition:
    include/ezrt_isosurface.h."""
    if not isinstance(cell, bool):
        raise ValueError("cell must be a bool")
    lib = _scene_lib(scene, {**_abi.ISO_ABI, **_abi.ISO_SIZES})
    _tensor("values", values, torch.float32)
    if values.dim() != 3:
        raise ValueError("values must have shape [nz, ny, nx], not %s" % (tuple(values.shape),))
    nz, ny, nx = _grid_shape(values.shape)
    o, hh = _grid_numbers(origin, spacing)
    mat = [0.0] * 18 if material is None else [float(x) for x in material]
    if len(mat) != 18:
        raise ValueError("material must have 18 entries, not %d" % len(mat))
    dev = values.device
    q = _OnStream(scene, values, stream)
    n_cells = (nx - 1) * (ny - 1) * (nz - 1)
    n_blocks = (n_cells + _abi.ISO_BLOCK - 1) // _abi.ISO_BLOCK
    work_bytes = int(lib.ezrt_iso_work_bytes(nx, ny, nz))
    grid_host = torch.tensor(o + hh + [float(iso), 0.0], dtype=torch.float64).to(torch.float32)
    work, summary = q.scratch(dev, work_bytes)
    with q.on():
        grid = grid_host.to(dev)
        mat18 = torch.tensor(mat, dtype=torch.float64).to(torch.float32).to(dev)
        offsets = torch.zeros((n_blocks + 1,), dtype=torch.int64, device=dev)
        if n_cells == 0:                                             # the C call writes nothing then: G1's LIVE, restated (see the docstring)
            summary[6] = int(bool(torch.isfinite(grid_host[:7]).all()) and bool((grid_host[3:6] > 0).all()))
    if n_cells > 0:
        q.call(lib.ezrt_iso_count_device, values, nx, ny, nz, grid, offsets, summary, work, work_bytes)
    with q.on():
        T = int(offsets[n_blocks].item())                            # the one synchronisation, of the query's stream
        rows = torch.empty((T, 36), dtype=torch.float32, device=dev)
        cells = torch.empty((T,), dtype=torch.int32, device=dev) if cell else None
    if n_cells > 0 and T > 0:
        q.call(lib.ezrt_iso_rows_device, values, nx, ny, nz, grid, mat18, offsets, T, rows, cells)
    q.done(values, summary, rows, cells)
    return IsoRows(rows, cells, summary, (nz, ny, nx))


def _check_max_k(max_k, most, count):
    if not isinstance(max_k, int) or isinstance(max_k, bool) or not 0 <= max_k <= most:
        raise ValueError("max_k must be an int in [0, %d], not %r" % (most, max_k))
    if max_k == 0 and not count:
        raise ValueError("max_k == 0 asks for the count alone: pass count=True")


def _overlap_rows(scene, fn, inputs, n, lead, dev, max_k, count, stream):
    """(tri int32 lead + (max_k,), n_overlap int32 lead or None) of a max_k call fn(inputs..., n, max_k, tri, n_overlap) for n queries,
    after _check_max_k and the function's own checks of its `inputs`."""
    lead = tuple(lead)
    if n * max_k > 2**31 - 1:
        raise ValueError("at most 2^31 - 1 output slots per call")
    tri = torch.empty(lead + (max_k,), dtype=torch.int32, device=dev)
    total = torch.empty(lead, dtype=torch.int32, device=dev) if count else None
    if n > 0:
        _OnStream(scene, dev, stream).run(fn, *inputs, n, max_k, tri if max_k else None, total)
    return tri, total


def _overlap_list(scene, kind, inputs, n, dev, capacity, check, stream):
    """The three steps of include/ezrt_overlap_list.h on the query's stream for the `kind` ("box", "obb", ...) of query whose
    `inputs` the caller has checked: the sibling's max_k == 0 call, then the offsets, then the fill."""
    _check_capacity("capacity", capacity)
    lib = _scene_lib(scene, _abi.OVERLAP_LIST_ABI)
    q = _OnStream(scene, dev, stream)
    n_found = torch.empty((n,), dtype=torch.int32, device=dev) if check else None
    if n == 0:
        rows = 0 if capacity is None else capacity
        with q.on():
            return OverlapList(torch.zeros((1,), dtype=torch.int64, device=dev), torch.full((rows,), -1, dtype=torch.int32, device=dev), n_found)
    offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    with q.on():
        n_overlap = torch.empty((n,), dtype=torch.int32, device=dev)
    q.call(getattr(lib, "ezrt_query_%s_overlap_device" % kind), *inputs, n, 0, None, n_overlap)
    q.call(lib.ezrt_overlap_offsets_device, n_overlap, n, offsets)
    with q.on():
        rows = int(offsets[n].item()) if capacity is None else capacity    # None: the one synchronisation, of the query's stream
        tri = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    q.run(getattr(lib, "ezrt_query_%s_overlap_list_device" % kind), *inputs, n, offsets, rows, tri if rows else None, n_found)
    return OverlapList(offsets, tri, n_found)


def box_overlap_list(scene, lo, hi, capacity=None, check=False, stream=None):
    """OverlapList(offsets int64 [n + 1], tri int32 [rows], n_found int32 [n] or None): for the n boxes of `lo`, `hi` (as for
    `box_overlap`, flattened row-major) EVERY triangle of the scene that touches the box, complete, in CSR form: tri[offsets[i] ..
    offsets[i + 1]) holds the triangles of box i in ascending id.  The test is `box_overlap`'s: a row's length is its n_overlap, its
    first 64 entries are its max_k = 64 row, and a box that is not live has an empty row.  `capacity=None` synchronises the stream
    once to read the total, offsets[n], and returns exactly that many entries.  A given `capacity` never synchronises and returns
    `capacity` entries: a row is written whole or not at all, rows that end past the capacity are missing (compare offsets[n] with
    the capacity), and every entry that belongs to no written row keeps tri == -1.  `check=True` also returns the number of
    triangles the fill pass itself met per box; it equals the row's length unless the scene was refitted between the passes.  The
    contract: include/ezrt_overlap_list.h."""
    n = _check_boxes(lo, hi)
    _scene_lib(scene, _abi.BOX_OVERLAP_ABI)
    return _overlap_list(scene, "box", (lo, hi), n, lo.device, capacity, check, stream)


def obb_overlap_list(scene, centre, axes, capacity=None, check=False, stream=None):
    """OverlapList(offsets, tri, n_found or None): `box_overlap_list` for the oriented boxes of `obb_overlap` -- every triangle that
    touches each box, in ascending id, CSR.  The contract: include/ezrt_overlap_list.h."""
    n = _check_obbs(centre, axes)
    _scene_lib(scene, _abi.OBB_OVERLAP_ABI)
    return _overlap_list(scene, "obb", (centre, axes), n, centre.device, capacity, check, stream)


def tri_overlap_list(scene, tris, capacity=None, check=False, stream=None):
    """OverlapList(offsets, tri, n_found or None): `box_overlap_list` for the query triangles of `tri_overlap` -- every triangle of
    the scene that each one crosses or touches, in ascending id, CSR.  The contract: include/ezrt_overlap_list.h."""
    n = _check_tris(tris)
    _scene_lib(scene, _abi.TRI_OVERLAP_ABI)
    return _overlap_list(scene, "tri", (tris,), n, tris.device, capacity, check, stream)


def self_overlap_list(scene, ids=None, capacity=None, check=False, stream=None):
    """OverlapList(offsets, tri, n_found or None): `box_overlap_list` for the triangle ids of `self_overlap` (None: every triangle of
    the scene, in order, on the current device) -- every OTHER triangle that crosses each one, in ascending id, CSR: every place
    where the mesh crosses itself.  The lists are symmetric: b is in a's row exactly when a is in b's, so with ids=None a pair
    appears twice; keep the entries above the row's own id for each pair once.  The contract: include/ezrt_overlap_list.h."""
    if ids is not None:
        _tensor("ids", ids, torch.int32)
    _scene_lib(scene, _abi.SELF_OVERLAP_ABI)
    if ids is None:
        n, device = scene.stats()["n_tri"], torch.device("cuda", torch.cuda.current_device())
    else:
        n, device = _count(ids, 1, "triangle ids"), ids.device
    return _overlap_list(scene, "self", (ids,), n, device, capacity, check, stream)


def capsule_overlap_list(scene, segs, radius, capacity=None, check=False, stream=None):
    """OverlapList(offsets, tri, n_found or None): `box_overlap_list` for the capsules of `capsule_overlap` -- every triangle within
    `radius` of each segment, in ascending id, CSR.  The contract: include/ezrt_overlap_list.h."""
    n = _check_segs(segs)
    _tensor("radius", radius, torch.float32, segs.shape[:-1], device=segs.device)
    _scene_lib(scene, _abi.SEGMENT_ABI)
    return _overlap_list(scene, "capsule", (segs, radius), n, segs.device, capacity, check, stream)


# the mesh smoothing has a module of its own (ezrt_amd/smooth.py) and is reached from here like every other mesh call
from .smooth import SmoothRows, smooth_rows  # noqa: E402,F401
