/* ezrt_refit.h -- device-side refit: move a scene's triangles without re-creating it (libezrt_hip.so only).
 *
 * A refit keeps every piece of a scene's topology -- the caller's tree, the triangle ranges of its leaves, the library's own tree over
 * those leaves and its 4-wide records -- and recomputes everything that depends on the vertices: the geometry and shading records,
 * every box, the distance-pruning bounds and flags.  Animation, picking after an object moved, shadow rays between frames.
 *
 *   tri36   DEVICE memory of the scene's device: n_tri x 36 floats in the layout and the triangle order given to ezrt_scene_create.
 *           Only floats 0-17 are read (p1 p2 p3 n1 n2 n3); the materials (floats 18-35) are not, and the scene keeps its own.
 *
 * Afterwards every entry point (ezrt_render, ezrt_render_device, ezrt_render_paths, ezrt_query_hits, ezrt_query.h, the counters)
 * answers exactly as a scene created by ezrt_scene_create(tri', n_tri, nodes', n_nodes) would, where tri' is the new triangle array
 * (with the scene's materials) and nodes' = ezrt_host_refit_nodes(tri', nodes) (ezrt_scene_c.h): the caller's arrays with every box
 * recomputed by the builder's own fold over the node's triangle range.  The results do not depend on the quality of the kept tree,
 * only the speed does: a tree built for other positions can cost more per ray.
 *
 *   - Kept as at create: the route (4-wide records or the binary kernel), whether the 4-wide records are the library's own tree over
 *     the leaves, the traversal stack bound, the tables that order exact ties.  These depend on the topology only.
 *   - Recomputed by create's rules: whether the scene prunes at all (every leaf box must hold its triangles, which a NaN vertex or a
 *     coordinate beyond the builder's start value of +-1145141919 can break) and every pruning scalar (ezrt_scene_prune_info).
 *
 * Ordering: the call is synchronous.  It makes `stream` (a hipStream_t of the scene's device; NULL = the default stream) wait for
 * every render call and device query already issued on the scene, whatever streams they were issued on, enqueues its kernels on
 * `stream`, and returns when the scene is updated.  Render calls and queries issued after it returns see the new geometry.  A render
 * call or query issued from another host thread while a refit runs is the caller's bug.  Steady state neither allocates nor frees
 * device memory (the scratch is sized at the first refit and kept with the scene) and never synchronises the whole device.
 *
 * Returns 0 or a negative EZRT_ERR_* code (ezrt.h; message in ezrt_last_error()); a rejected call changes nothing:
 *   EZRT_ERR_INVALID      NULL scene or tri36, n_tri other than the scene's triangle count, tri36 not device memory of the scene's
 *                         device (host memory included: it is never dereferenced)
 *   EZRT_ERR_UNSUPPORTED  the scene's node arrays are not a tree (a node with two parents) */
#ifndef EZRT_REFIT_H
#define EZRT_REFIT_H

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_scene_refit_device(EzrtScene* s, const float* tri36, int n_tri, void* stream);

#ifdef __cplusplus
}
#endif
#endif
