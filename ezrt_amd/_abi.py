"""ctypes declarations for the C ABIs (include/ezrt.h, include/ezrt_scene_c.h, and the HIP library's own headers).

`declare_trace_abi(lib)` attaches argtypes/restypes for every symbol of
include/ezrt.h to an already-opened CDLL.  The product only ever opens
ezrt_amd/lib/libezrt_hip.so (see `load_hip`); tests open the CPU oracle
themselves and reuse `declare_trace_abi` so both sides share one binding.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)
c_uint64_p = C.POINTER(C.c_uint64)
c_int64_p = C.POINTER(C.c_int64)

EZRT_CTR_COUNT = 8
CTR_NAMES = ("rays", "node_pops", "inner_pops", "tri_tests", "mat_fetch", "samples", "env_map", "env_cache")

INTEGRATOR_P3_DIFFUSE = 3
INTEGRATOR_P4_DISNEY = 4
INTEGRATOR_P5_SOBOL = 50
INTEGRATOR_P5_MIS = 51
INTEGRATOR_P5_MIS_ANISO = 52  # P5's loop with the anisotropic lobe evaluated + importance-sampled
FILTER_NEAREST = 0
FILTER_BILINEAR = 1


class EzrtRenderParams(C.Structure):
    """Mirror of `EzrtRenderParams` (include/ezrt.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
        ("frame0", C.c_uint32), ("spp", C.c_uint32),
        ("max_bounce", C.c_int32), ("integrator", C.c_int32),
        ("eye", C.c_float * 3),
        ("camera_rotate", C.c_float * 16),
        ("env_clamp", C.c_float),
        ("tile_w", C.c_int32), ("tile_h", C.c_int32),
        ("shard_index", C.c_int32), ("shard_count", C.c_int32),
    ]


# every symbol include/ezrt.h declares: name -> (restype, argtypes)
TRACE_ABI = {
    "ezrt_scene_create": (C.c_int, [c_float_p, C.c_int, c_float_p, C.c_int, C.POINTER(C.c_void_p)]),
    "ezrt_scene_destroy": (None, [C.c_void_p]),
    "ezrt_scene_set_env": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int]),
    "ezrt_scene_set_sampler": (C.c_int, [C.c_void_p, C.c_int]),
    "ezrt_render": (C.c_int, [C.c_void_p, C.POINTER(EzrtRenderParams), c_float_p]),
    "ezrt_render_device": (C.c_int, [C.c_void_p, C.POINTER(EzrtRenderParams), C.c_void_p, C.c_void_p]),
    "ezrt_frame_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "ezrt_frame_destroy": (C.c_int, [C.c_void_p]),
    "ezrt_frame_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p]),
    "ezrt_frame_write": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p]),
    "ezrt_render_paths": (C.c_int, [C.c_void_p, C.POINTER(EzrtRenderParams), c_int32_p, c_float_p, c_float_p]),
    "ezrt_frame_nonfinite": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_int64_p]),
    "ezrt_query_hits": (C.c_int, [C.c_void_p, c_float_p, C.c_int, c_int32_p, c_float_p]),
    "ezrt_tonemap": (C.c_int, [c_float_p, C.c_int, c_uint8_p]),
    "ezrt_sobol": (C.c_int, [C.c_uint32, C.c_int, C.c_int, c_float_p]),
    "ezrt_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "ezrt_set_instrumentation": (C.c_int, [C.c_void_p, C.c_int]),
    "ezrt_counters": (C.c_int, [C.c_void_p, c_uint64_p]),
    "ezrt_counters_reset": (C.c_int, [C.c_void_p]),
    "ezrt_last_render_ms": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.POINTER(C.c_int)]),
    "ezrt_scene_stats": (C.c_int, [C.c_void_p, c_int64_p]),
    "ezrt_scene_prune_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "ezrt_debug_math": (C.c_int, [C.c_int, c_float_p, c_float_p, C.c_int, c_float_p]),
    "ezrt_debug_fn": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, c_float_p]),
    "ezrt_last_error": (C.c_char_p, []),
    "ezrt_trim": (C.c_int, []),
    "ezrt_backend": (C.c_char_p, []),
}

HOST_ABI = {
    "ezrt_host_scene_new": (C.c_void_p, []),
    "ezrt_host_scene_free": (None, [C.c_void_p]),
    "ezrt_host_material_defaults": (C.c_int, [C.c_int, c_float_p]),
    "ezrt_host_get_transform_matrix": (C.c_int, [c_float_p, c_float_p, c_float_p, c_float_p]),
    "ezrt_host_read_obj": (C.c_int, [C.c_void_p, C.c_char_p, c_float_p, c_float_p, C.c_int]),
    "ezrt_host_read_obj_text": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64, c_float_p, c_float_p, C.c_int]),
    "ezrt_host_add_triangles": (C.c_int, [C.c_void_p, c_float_p, C.c_int]),
    "ezrt_host_build_bvh": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ezrt_host_set_tie_order": (C.c_int, [C.c_int]),
    "ezrt_host_build_stats": (C.c_int, [C.c_void_p, c_int64_p]),
    "ezrt_host_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ezrt_host_encode": (C.c_int, [C.c_void_p, c_float_p, c_float_p]),
    "ezrt_host_hdr_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(c_float_p)]),
    "ezrt_host_hdr_load_memory": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(c_float_p)]),
    "ezrt_host_hdr_cache": (C.c_int, [c_float_p, C.c_int, C.c_int, c_float_p]),
    "ezrt_host_free": (None, [C.c_void_p]),
    "ezrt_host_camera": (C.c_int, [C.c_float, C.c_float, C.c_float, c_float_p, c_float_p]),
    "ezrt_host_p2_query": (C.c_int, [c_float_p, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int, C.c_int, c_float_p,
                                     C.POINTER(C.c_int), c_float_p]),
    "ezrt_host_refit_nodes": (C.c_int, [c_float_p, C.c_int, c_float_p, C.c_int, c_float_p]),
    "ezrt_host_last_error": (C.c_char_p, []),
}


# GPU scene-build entry points of libezrt_hip.so only (include/ezrt_build.h)
BUILD_ABI = {
    "ezrt_build_lbvh": (C.c_int, [c_float_p, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, C.POINTER(C.c_int),
                                  c_float_p]),
    "ezrt_build_sah": (C.c_int, [c_float_p, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, C.POINTER(C.c_int),
                                 c_float_p]),
    "ezrt_build_median": (C.c_int, [c_float_p, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, C.POINTER(C.c_int),
                                    c_float_p]),
    "ezrt_build_device_count": (C.c_int, []),
}


# stream-ordered ray queries on device memory, libezrt_hip.so only (include/ezrt_query.h); pointers are device addresses
QUERY_ABI = {
    "ezrt_query_closest_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ezrt_query_occluded_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}


# stream-ordered surface queries on device memory, libezrt_hip.so only (include/ezrt_surface.h); pointers are device addresses
SURFACE_ABI = {
    "ezrt_query_surface_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


# stream-ordered shading queries on device memory, libezrt_hip.so only (include/ezrt_shade.h); pointers are device addresses
SHADE_ABI = {
    # s, tri_id, n, mat18, stream
    "ezrt_query_material_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # s, integrator, tri_id, V, N, L, n, f_r, pdf, stream
    "ezrt_shade_eval_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    # s, integrator, tri_id, xi, V, N, n, L, stream
    "ezrt_shade_sample_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p]),
    # s, L, n, env_clamp, colour, pdf, stream
    "ezrt_env_eval_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, xi, n, L, stream
    "ezrt_env_sample_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}


# stream-ordered path queries on device memory, libezrt_hip.so only (include/ezrt_path.h); pointers are device addresses
PATH_ABI = {
    # s, p, sample_xyf, n, rays_od6, stream
    "ezrt_camera_rays_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # s, integrator, max_bounce, env_clamp, rays_od6, sample_xyf, n, radiance, stream
    "ezrt_query_radiance_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p]),
}


# stream-ordered all-hits queries on device memory, libezrt_hip.so only (include/ezrt_multihit.h); pointers are device addresses
MULTIHIT_ABI = {
    # s, rays_od6, t_max, n_rays, max_hits, tri_id, t_hit, n_hits, stream
    "ezrt_query_all_hits_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    # s, rays_od6, tri_id, t_hit, n, integrator, hit_point, normal, inside, stream
    "ezrt_surface_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
}
ALL_HITS_MAX = 64  # EZRT_ALL_HITS_MAX


# stream-ordered closest-point queries on device memory, libezrt_hip.so only (include/ezrt_closest_point.h); pointers are device addresses
CLOSEST_POINT_ABI = {
    # s, points3, d_max, n, tri_id, point, dist, bary, stream
    "ezrt_query_closest_point_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
}


# stream-ordered nearest-K queries on device memory, libezrt_hip.so only (include/ezrt_nearest.h); pointers are device addresses
NEAREST_ABI = {
    # s, points3, d_max, n, max_k, tri_id, dist, n_within, stream
    "ezrt_query_nearest_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    # s, points3, tri_id, n, point, dist, bary, stream
    "ezrt_closest_point_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
}
NEAREST_MAX = 64  # EZRT_NEAREST_MAX


# stream-ordered inside and signed-distance queries on device memory, libezrt_hip.so only (include/ezrt_inside.h); pointers are
# device addresses
INSIDE_ABI = {
    # s, points3, n, axis, inside, crossings, stream
    "ezrt_query_inside_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, points3, d_max, n, axis, tri_id, point, sdist, bary, inside, stream
    "ezrt_query_signed_distance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


# stream-ordered box-overlap queries on device memory, libezrt_hip.so only (include/ezrt_box_overlap.h); pointers are device addresses
BOX_OVERLAP_ABI = {
    # s, box_lo3, box_hi3, n, max_k, tri_id, n_overlap, stream
    "ezrt_query_box_overlap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, box_lo3, box_hi3, tri_id, n, overlaps, stream
    "ezrt_box_overlap_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}
BOX_OVERLAP_MAX = 64  # EZRT_BOX_OVERLAP_MAX


# stream-ordered triangle-overlap queries on device memory, libezrt_hip.so only (include/ezrt_tri_overlap.h); pointers are device
# addresses
TRI_OVERLAP_ABI = {
    # s, tris9, n, max_k, tri_id, n_overlap, stream
    "ezrt_query_tri_overlap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, tris9, tri_id, n, overlaps, stream
    "ezrt_tri_overlap_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}
TRI_OVERLAP_MAX = 64  # EZRT_TRI_OVERLAP_MAX


# stream-ordered self-overlap queries on device memory, libezrt_hip.so only (include/ezrt_self_overlap.h); pointers are device
# addresses
SELF_OVERLAP_ABI = {
    # s, ids, n, max_k, tri_id, n_overlap, stream
    "ezrt_query_self_overlap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, tri_a, tri_b, n, crosses, stream
    "ezrt_self_overlap_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}
SELF_OVERLAP_MAX = 64  # EZRT_SELF_OVERLAP_MAX


# stream-ordered triangle-distance queries on device memory, libezrt_hip.so only (include/ezrt_tri_distance.h); pointers are device
# addresses
TRI_DISTANCE_ABI = {
    # s, tris9, d_max, n, tri_id, dist, point_query, point_scene, crosses, stream
    "ezrt_query_tri_distance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, tris9, tri_id, n, dist, point_query, point_scene, crosses, stream
    "ezrt_tri_distance_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
}


# stream-ordered sphere-cast queries on device memory, libezrt_hip.so only (include/ezrt_sphere_cast.h); pointers are device addresses
SPHERE_CAST_ABI = {
    # s, rays6, radius, t_max, n, tri_id, t, point, touching, stream
    "ezrt_query_sphere_cast_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, rays6, radius, tri_id, n, t, point, touching, stream
    "ezrt_sphere_cast_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
}


# stream-ordered segment queries on device memory, libezrt_hip.so only (include/ezrt_segment.h); pointers are device addresses.
# segs6 holds the two END POINTS of every segment, not an origin and a direction.
SEGMENT_ABI = {
    # s, segs6, d_max, n, tri_id, dist, point_query, point_scene, crosses, stream
    "ezrt_query_segment_distance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, segs6, tri_id, n, dist, point_query, point_scene, crosses, stream
    "ezrt_segment_distance_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    # s, segs6, radius, n, max_k, tri_id, n_overlap, stream
    "ezrt_query_capsule_overlap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]),
}
CAPSULE_OVERLAP_MAX = 64  # EZRT_CAPSULE_OVERLAP_MAX


# stream-ordered oriented-box queries on device memory, libezrt_hip.so only (include/ezrt_obb_overlap.h); pointers are device addresses
OBB_OVERLAP_ABI = {
    # s, centre3, axes9, n, max_k, tri_id, n_overlap, stream
    "ezrt_query_obb_overlap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, centre3, axes9, tri_id, n, overlaps, stream
    "ezrt_obb_overlap_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}
OBB_OVERLAP_MAX = 64  # EZRT_OBB_OVERLAP_MAX


# stream-ordered winding-number queries on device memory, libezrt_hip.so only (include/ezrt_winding.h); pointers are device addresses
WINDING_ABI = {
    # s, points3, n, chunks, fixed, winding, stream
    "ezrt_query_winding_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, points3, tri_id, n, fixed, winding, stream
    "ezrt_winding_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # n, n_tri: the slices of a call with chunks == 0
    "ezrt_winding_chunks": (C.c_int, [C.c_int, C.c_int]),
}


# stream-ordered plane queries on device memory, libezrt_hip.so only (include/ezrt_plane.h); pointers are device addresses
PLANE_ABI = {
    # n, n_tri, slices: the effective number of slices
    "ezrt_plane_slices": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    # s, planes4, n, slices, part, n_cross, offsets, stream
    "ezrt_query_plane_count_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # s, planes4, n, slices, part, offsets, capacity, tri_id, seg, stream
    "ezrt_query_plane_section_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    # s, planes4, tri_id, n, crosses, side, seg, stream
    "ezrt_plane_section_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
PLANE_TILE = 64  # planes per workgroup (ezrt_point_queries.h: PL_TILE)


# stream-ordered plane loops on device memory, libezrt_hip.so only (include/ezrt_plane_loops.h); pointers are device addresses
PLANE_LOOPS_ABI = {
    # capacity: the bytes of `work` (no device work)
    "ezrt_plane_loops_work_bytes": (C.c_size_t, [C.c_int64]),
    # tile_rows_max: the limit as compiled (a host pointer; no device work)
    "ezrt_plane_loops_limits": (None, [C.c_void_p]),
    # s, offsets, n, seg, capacity, tile_rows, next, order, plane_loops, loop_capacity, loop_offsets, closed, work, work_bytes, stream
    "ezrt_plane_loops_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}


def plane_loops_limits():
    """tile_rows_max of the loaded HIP library: the longest plane that is chained in the LDS of one workgroup
    (include/ezrt_plane_loops.h).  No device work."""
    lib = _declare(load_hip(), PLANE_LOOPS_ABI)
    a = C.c_int(-1)
    lib.ezrt_plane_loops_limits(C.byref(a))
    return a.value


# stream-ordered mesh topology on device memory, libezrt_hip.so only (include/ezrt_topology.h); pointers are device addresses
TOPOLOGY_ABI = {
    # n_tri: the bytes of `work` (no device work)
    "ezrt_topology_work_bytes": (C.c_size_t, [C.c_int]),
    # s, twin, edge_class, mult, root, component, comp_root, comp_size, comp_flags, summary, work, work_bytes, stream
    "ezrt_mesh_topology_device": (C.c_int, [C.c_void_p] * 11 + [C.c_size_t, C.c_void_p]),
    # s, tri_a, edge_a, tri_b, n, shared, opposite, stream
    "ezrt_mesh_topology_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}
EDGE_BOUNDARY, EDGE_MANIFOLD, EDGE_FLIPPED, EDGE_NONMANIFOLD = 1, 2, 3, 4


# stream-ordered vertex weld and smooth normals on device memory, libezrt_hip.so only (include/ezrt_vertices.h); pointers are device
# addresses
WELD_ABI = {
    # n_tri: the bytes of `work` (no device work)
    "ezrt_weld_work_bytes": (C.c_size_t, [C.c_int]),
    # s, vertex, vert_corner, star_offsets, star, fans, vert_flags, summary, work, work_bytes, stream
    "ezrt_mesh_weld_device": (C.c_int, [C.c_void_p] * 9 + [C.c_size_t, C.c_void_p]),
    # s, corner_a, corner_b, n, same, stream
    "ezrt_mesh_weld_at_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ezrt_vertex_normals_work_bytes": (C.c_size_t, [C.c_int]),
    # s, tri36, n_tri, vertex, star_offsets, star, work, work_bytes, stream
    "ezrt_vertex_normals_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p]),
}
VERTEX_BORDER, VERTEX_NONMANIFOLD_EDGE, VERTEX_PINCHED = 1, 2, 4


# stream-ordered mesh orientation on device memory, libezrt_hip.so only (include/ezrt_orient.h); pointers are device addresses
ORIENT_ABI = {
    # n_tri: the bytes of `work` (no device work)
    "ezrt_orient_work_bytes": (C.c_size_t, [C.c_int]),
    # s, twin, edge_class, outward, flip, patch_root, patch, proot, psize, pflags, vol6, summary, work, work_bytes, stream
    "ezrt_mesh_orient_device": (C.c_int, [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, C.c_void_p]),
    # s, tri36, n_tri, flip, stream
    "ezrt_rewind_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}
PATCH_OPEN, PATCH_NONORIENTABLE, PATCH_REWOUND, PATCH_INWARD = 1, 2, 4, 8


# stream-ordered boundary loops and caps on device memory, libezrt_hip.so only (include/ezrt_boundary.h); pointers are device addresses
BOUNDARY_ABI = {
    # n_tri: the bytes of `work` (no device work)
    "ezrt_boundary_work_bytes": (C.c_size_t, [C.c_int]),
    # s, twin, edge_class, next, loop, pos, order, loop_offsets, lflags, area2 (or None), summary, work, work_bytes, stream
    "ezrt_mesh_boundary_device": (C.c_int, [C.c_void_p] * 12 + [C.c_size_t, C.c_void_p]),
    # s, tri36, n_tri, order, loop, pos, loop_offsets, lflags, summary, cap, cap_valid, stream
    "ezrt_cap_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9),
}
LOOP_CLOSED = 1


# stream-ordered plane clipping on device memory, libezrt_hip.so only (include/ezrt_clip.h); pointers are device addresses
CLIP_ABI = {
    # n_rows: the bytes of `work` (no device work)
    "ezrt_clip_work_bytes": (C.c_size_t, [C.c_int]),
    # s, tri36, n_rows, plane4, offsets, summary, work, work_bytes, stream
    "ezrt_clip_count_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    # s, tri36, n_rows, plane4, offsets, capacity, out, src (or None), cut_edge (or None), stream
    "ezrt_clip_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4),
}


# stream-ordered subdivision on device memory, libezrt_hip.so only (include/ezrt_subdivide.h); pointers are device addresses
SUBDIVIDE_ABI = {
    # n_rows, mode: the bytes of `work` (no device work)
    "ezrt_subdivide_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    # s, tri36, n_rows, mode, twin, edge_class, vertex, star_offsets, star, vert_flags (the six: None in midpoint mode), out, summary,
    # work, work_bytes, stream
    "ezrt_subdivide_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, C.c_void_p]),
}
SUBDIVIDE_MIDPOINT, SUBDIVIDE_LOOP = 0, 1


# stream-ordered decimation on device memory, libezrt_hip.so only (include/ezrt_decimate.h); pointers are device addresses
DECIMATE_ABI = {
    # n_rows: the bytes of `work` (no device work)
    "ezrt_decimate_work_bytes": (C.c_size_t, [C.c_int]),
    # s, tri36, n_rows, grid4, flags, cell, cell_corner, cell_point, offsets, summary, work, work_bytes, stream
    "ezrt_decimate_count_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]),
    # s, tri36, n_rows, cell, cell_point, offsets, capacity, out, src (or None), stream
    "ezrt_decimate_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 3),
}
DECIMATE_DEDUP = 1


# stream-ordered isosurface extraction on device memory, libezrt_hip.so only (include/ezrt_isosurface.h); pointers are device addresses
ISO_ABI = {
    # s, values, nx, ny, nz, grid8, offsets, summary, work, work_bytes, stream
    "ezrt_iso_count_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    # s, values, nx, ny, nz, grid8, material18, offsets, capacity, out, cell (or None), stream
    "ezrt_iso_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3),
}
# the header's third entry point, in a table of its own: the *_work_bytes of the *_ABI tables are functions of a row count, which
# tests/test_mesh_work_bytes.py holds to their formulas over one list of counts; this one takes the grid's three dimensions
# (tests/test_iso_abi.py holds it to its formula)
ISO_SIZES = {
    # nx, ny, nz: the bytes of `work` (no device work)
    "ezrt_iso_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
}
ISO_BLOCK = 256  # EZRT_ISO_BLOCK: cells per entry of offsets


# stream-ordered mesh smoothing on device memory, libezrt_hip.so only (include/ezrt_smooth.h); pointers are device addresses
SMOOTH_ABI = {
    # s, tri36, n_rows, edge_class, vertex, star_offsets, star, vert_flags, steps, lambda, mu, flags, tile_rows, out, summary, work,
    # work_bytes, stream
    "ezrt_smooth_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_float, C.c_float, C.c_int, C.c_int]
                                + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
}
# the header's other entry points, in a table of their own as ISO_SIZES: tests/test_mesh_work_bytes.py holds the *_work_bytes of the
# *_ABI tables to its own list of formulas (tests/test_smooth_abi.py holds this one to its formula)
SMOOTH_SIZES = {
    # n_rows: the bytes of `work` (no device work)
    "ezrt_smooth_work_bytes": (C.c_size_t, [C.c_int]),
    # tile_rows_max: the limit as compiled (a host pointer; no device work)
    "ezrt_smooth_limits": (None, [C.c_void_p]),
}
SMOOTH_PIN_BORDER = 1
SMOOTH_STEPS_MAX = 1024


def smooth_limits():
    """tile_rows_max of the loaded HIP library: the rows whose smoothing steps run in LDS, in one launch (include/ezrt_smooth.h).  No
    device work."""
    lib = _declare(load_hip(), SMOOTH_SIZES)
    a = C.c_int(-1)
    lib.ezrt_smooth_limits(C.byref(a))
    return a.value


# stream-ordered overlap lists on device memory, libezrt_hip.so only (include/ezrt_overlap_list.h); pointers are device addresses
_LIST = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]  # offsets, capacity, tri_id, n_found, stream
OVERLAP_LIST_ABI = {
    # insert_max, tile_max: the limits as compiled (host pointers; no device work)
    "ezrt_overlap_list_limits": (None, [C.c_void_p, C.c_void_p]),
    # s, n_overlap, n, offsets, stream
    "ezrt_overlap_offsets_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # s, box_lo3, box_hi3, n, offsets, capacity, tri_id, n_found, stream
    "ezrt_query_box_overlap_list_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + _LIST),
    # s, centre3, axes9, n, offsets, capacity, tri_id, n_found, stream
    "ezrt_query_obb_overlap_list_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + _LIST),
    # s, tris9, n, offsets, capacity, tri_id, n_found, stream
    "ezrt_query_tri_overlap_list_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + _LIST),
    # s, ids, n, offsets, capacity, tri_id, n_found, stream
    "ezrt_query_self_overlap_list_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + _LIST),
    # s, segs6, radius, n, offsets, capacity, tri_id, n_found, stream
    "ezrt_query_capsule_overlap_list_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + _LIST),
}


def overlap_list_limits():
    """(insert_max, tile_max) of the loaded HIP library: rows up to insert_max ids are kept sorted while they are filled, rows up to
    tile_max ids are sorted in LDS, longer ones in global memory (include/ezrt_overlap_list.h).  No device work."""
    lib = _declare(load_hip(), OVERLAP_LIST_ABI)
    a, b = C.c_int(-1), C.c_int(-1)
    lib.ezrt_overlap_list_limits(C.byref(a), C.byref(b))
    return a.value, b.value


# device-side refit of a scene's geometry, libezrt_hip.so only (include/ezrt_refit.h); tri36 is a device address
REFIT_ABI = {
    "ezrt_scene_refit_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
}


# include/ezrt_mgpu.h: one process, N devices (both libraries: the oracle's "devices" are host memory)
MGPU_ABI = {
    "ezrt_mgpu_create": (C.c_int, [c_float_p, C.c_int, c_float_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int,
                                   C.POINTER(C.c_void_p)]),
    "ezrt_mgpu_destroy": (None, [C.c_void_p]),
    "ezrt_mgpu_set_env": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int]),
    "ezrt_mgpu_set_sampler": (C.c_int, [C.c_void_p, C.c_int]),
    "ezrt_mgpu_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "ezrt_mgpu_render": (C.c_int, [C.c_void_p, C.POINTER(EzrtRenderParams)]),
    "ezrt_mgpu_gather": (C.c_int, [C.c_void_p, c_float_p]),
    "ezrt_mgpu_frame_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "ezrt_mgpu_counters": (C.c_int, [C.c_void_p, c_uint64_p]),
    "ezrt_mgpu_last_ms": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_int64_p]),
    "ezrt_tiles_packed_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ezrt_tiles_pack_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "ezrt_tiles_unpack_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p]),
}
TRANSPORT_RCCL, TRANSPORT_PEER, TRANSPORT_HOST = 0, 1, 2


# Test hooks of include/ezrt.h that a library may have been built without (an oracle built from older sources): binding such a
# library does not fail, calling the hook on it does (AttributeError).  The product library is bound strictly (load_hip).
TEST_HOOKS = ("ezrt_debug_fn",)


def _declare(lib, table, optional=()):
    for name, (res, args) in table.items():
        if name in optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    return lib


def declare_trace_abi(lib, strict=False):
    return _declare(_declare(lib, TRACE_ABI, () if strict else TEST_HOOKS), MGPU_ABI)


def declare_host_abi(lib):
    return _declare(lib, HOST_ABI)


_hip = None
_host = None


def load_hip():
    """Open the HIP product library.  There is no CPU fallback: if the extension
    is missing this raises."""
    global _hip
    if _hip is None:
        path = os.environ.get("EZRT_HIP_LIB") or os.path.join(LIB_DIR, "libezrt_hip.so")  # override: A/B builds
        if not os.path.exists(path):
            raise RuntimeError(
                "ezrt_amd: %s is missing -- build it with `make hip` (or __graft_entry__.build()); "
                "there is no CPU fallback for the trace" % path)
        lib = declare_trace_abi(C.CDLL(path), strict=True)
        for table in (BUILD_ABI, QUERY_ABI, SURFACE_ABI, SHADE_ABI, PATH_ABI, MULTIHIT_ABI, CLOSEST_POINT_ABI, NEAREST_ABI,
                      INSIDE_ABI, BOX_OVERLAP_ABI, TRI_OVERLAP_ABI, SELF_OVERLAP_ABI, TRI_DISTANCE_ABI, SPHERE_CAST_ABI, SEGMENT_ABI,
                      OBB_OVERLAP_ABI, WINDING_ABI, PLANE_ABI, PLANE_LOOPS_ABI, TOPOLOGY_ABI, WELD_ABI, ORIENT_ABI, BOUNDARY_ABI,
                      CLIP_ABI, SUBDIVIDE_ABI, DECIMATE_ABI, ISO_ABI, ISO_SIZES, SMOOTH_ABI, SMOOTH_SIZES, OVERLAP_LIST_ABI,
                      REFIT_ABI):
            _declare(lib, table)
        _hip = lib
    return _hip


def load_host():
    global _host
    if _host is None:
        path = os.path.join(LIB_DIR, "libezrt_scene.so")
        if not os.path.exists(path):
            raise RuntimeError("ezrt_amd: %s is missing -- build it with `make host`" % path)
        _host = declare_host_abi(C.CDLL(path))
    return _host
