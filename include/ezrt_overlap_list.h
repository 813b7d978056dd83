/* ezrt_overlap_list.h -- stream-ordered overlap LISTS on device memory (libezrt_hip.so only): all triangles a query touches, in CSR form.
 *
 * The five list queries -- ezrt_box_overlap.h, ezrt_obb_overlap.h, ezrt_tri_overlap.h, ezrt_self_overlap.h and the capsules of
 * ezrt_segment.h -- return the lowest max_k ids, max_k at most 64, and the full count.  The box that holds a whole part, a tool swept
 * through a dense region and "every place where this mesh crosses itself" have rows far longer than 64: those calls say HOW MANY
 * triangles such a query touches and cannot hand them over.  The calls here do, by the count / offsets / fill pattern of ezrt_plane.h:
 *
 *   1. count    the existing call with max_k == 0 writes n_overlap[i], the length of row i;
 *   2. offsets  ezrt_overlap_offsets_device writes the exclusive prefix sum in int64: offsets[i] = n_overlap[0] + .. + n_overlap[i - 1],
 *               and offsets[n] the total -- the number of ids the caller must have room for;
 *   3. fill     ezrt_query_*_overlap_list_device writes row i into tri_id[offsets[i] .. offsets[i + 1]).
 *
 * THE RULE.  No new geometry is defined: a triangle k is in row i exactly when the query's existing per-pair rule holds for (i, k) --
 * H1 .. H3 of ezrt_box_overlap.h, H0 .. H3 of ezrt_obb_overlap.h, the rule of ezrt_tri_overlap.h, of ezrt_self_overlap.h (for every
 * triangle but the query's own), and dist2 <= radius * radius of ezrt_segment.h -- evaluated by the same functions as in the max_k
 * calls.  Every answer is a set of integers.
 * L1  Row i holds EVERY such triangle, in ASCENDING id; the rows follow one another in the order of the queries.
 * L2  Agreement with the max_k calls: the length of row i is their n_overlap[i], and its first min(64, length) entries are their
 *     max_k = 64 row, bit for bit.  A query that is not live (a box with lo > hi, a NaN, an id outside the scene, ...) has an empty row.
 * L3  Independence: the rows depend on neither the tree, nor the route (the pruned walk or the sweep over all triangles), nor the
 *     order of the triangles beyond the ids themselves, nor the batch a query is part of.
 * L4  ezrt_query_self_overlap_list_device is SYMMETRIC: b is in a's row exactly when a is in b's (self_crosses is symmetric in its
 *     two triangles).  With ids == NULL every crossing pair therefore appears twice, once in either row.  No de-duplicated pair form
 *     is offered: keep the entries with tri_id > the row's own id.
 *
 * n_found (optional) receives, per query, the number of triangles that the FILL pass itself met.  n_found[i] == offsets[i + 1] -
 * offsets[i] for all i certifies the list.  Where the two differ -- the scene was refitted between count and fill, or the offsets are
 * not those of a count of these queries on this scene -- the contents of row i are unspecified, and still nothing outside row i is
 * touched.
 *
 * MEMORY SAFETY FOR ANY offsets ARRAY.  The fill call reads offsets and believes nothing:
 * - a row with offsets[i] < 0 or offsets[i + 1] < offsets[i] is treated as empty;
 * - a row is written WHOLE OR NOT AT ALL: a row with offsets[i + 1] > capacity is skipped entirely.  With offsets from step 2 the
 *   caller sees the overflow in offsets[n] > capacity and may call again with a larger array (the count need not be repeated);
 * - entries of tri_id that belong to no written row are not touched, and no entry at or past `capacity` is ever addressed;
 * - n_found is the truth in every one of these cases.
 *
 * How it is computed.  One query per lane, the traversal, the gate and the per-pair rule of the max_k sibling (the kernels share one
 * body), on the route that call would take.  A row of at most insert_max ids is kept sorted while it is filled, by the sibling's
 * insertion; a longer row is appended in the order of the visits and sorted in place afterwards by a second kernel, in LDS when it
 * has at most tile_max ids and in global memory, without a second buffer, when it has more.  On the sweep route the visits ascend
 * and no row needs the second kernel, which is then not launched.  ezrt_overlap_list_limits reports the two limits as compiled
 * (0 <= insert_max <= 64 < tile_max, tile_max a power of two whose ids fit in 64 KiB); they change the time of a call and nothing
 * of its answer.  Either pointer may be NULL.
 *
 * Memory, streams, ordering and errors are those of the sibling calls: every pointer is device memory of the scene's device, large
 * enough for its elements (anything else is rejected before any launch, never dereferenced); work is enqueued on `stream` and the
 * call returns without synchronising; no scratch allocation is used; the calls may run beside ezrt_render_device and the other
 * queries on other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them, and a
 * call issued after the refit returned sees the new geometry (count and fill must see the same).
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, NULL input array (ids may be NULL: query i is triangle i,
 * and n must not exceed the scene's triangles), NULL n_overlap or offsets; NULL tri_id with capacity > 0; n < 0; capacity < 0, or
 * more than an array can hold (PTRDIFF_MAX / 4 ids); a pointer that is not device memory of the scene's device.  n == 0 returns 0
 * and launches nothing (offsets[0] is then not written either). */
#ifndef EZRT_OVERLAP_LIST_H
#define EZRT_OVERLAP_LIST_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the limits as compiled (no device work; never fails) */
void ezrt_overlap_list_limits(int* insert_max, int* tile_max);
/* step 2: the exclusive prefix sum of n_overlap, the total in offsets[n] */
int ezrt_overlap_offsets_device(EzrtScene* s, const int32_t* n_overlap /* n */, int n, int64_t* offsets /* n + 1 */, void* stream);
/* step 3, one per query kind; the inputs are those of the max_k call */
int ezrt_query_box_overlap_list_device(EzrtScene* s, const float* box_lo3 /* n x 3 */, const float* box_hi3 /* n x 3 */, int n,
                                       const int64_t* offsets /* n + 1 */, int64_t capacity, int32_t* tri_id /* capacity */,
                                       int32_t* n_found /* n, or NULL */, void* stream);
int ezrt_query_obb_overlap_list_device(EzrtScene* s, const float* centre3 /* n x 3 */, const float* axes9 /* n x 9 */, int n,
                                       const int64_t* offsets /* n + 1 */, int64_t capacity, int32_t* tri_id /* capacity */,
                                       int32_t* n_found /* n, or NULL */, void* stream);
int ezrt_query_tri_overlap_list_device(EzrtScene* s, const float* tris9 /* n x 9 */, int n, const int64_t* offsets /* n + 1 */, int64_t capacity,
                                       int32_t* tri_id /* capacity */, int32_t* n_found /* n, or NULL */, void* stream);
int ezrt_query_self_overlap_list_device(EzrtScene* s, const int32_t* ids /* n, or NULL */, int n, const int64_t* offsets /* n + 1 */,
                                        int64_t capacity, int32_t* tri_id /* capacity */, int32_t* n_found /* n, or NULL */, void* stream);
int ezrt_query_capsule_overlap_list_device(EzrtScene* s, const float* segs6 /* n x 6 */, const float* radius /* n */, int n,
                                           const int64_t* offsets /* n + 1 */, int64_t capacity, int32_t* tri_id /* capacity */,
                                           int32_t* n_found /* n, or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
