/* ezrt_smooth.h -- stream-ordered MESH SMOOTHING on device memory (libezrt_hip.so only): Laplacian and Taubin fairing of the caller's
 * triangle rows, many steps in one call.
 *
 * The mesh calls of this library make a mesh (ezrt_isosurface.h) and clip, refine and coarsen it (ezrt_clip.h, ezrt_subdivide.h,
 * ezrt_decimate.h); none of them improves the shape of the triangles it is given, and the two newest need that most: marching
 * tetrahedra emits slivers, vertex clustering leaves a jagged surface.  The call here relaxes: every vertex moves towards the mean of
 * its neighbours, `steps` times, with the weights lambda and mu in turn.  The star of a vertex is the weld's (ezrt_vertices.h), its
 * border the topology's (ezrt_topology.h); the walk of a star is the one of Loop subdivision (ezrt_subdivide.h, S4 .. S7).  The rows
 * go in and come out at the same size, so a chain "signed distance -> isosurface -> smooth -> decimate -> normals -> refit" stays on
 * the device with no host round trip.
 *
 * THE DEFINITION.  All arithmetic is fp32, one rounding per written operation, no contraction; division is IEEE.  Corners,
 * half-edges, "Key" and the row layout are those of ezrt_subdivide.h: corner c = 3 t + k is stored vertex k of row t; half-edge
 * 3 t + e runs from stored vertex e to stored vertex (e + 1) % 3; pa(c) is the next stored vertex of c's row and pb(c) the one after.
 *
 * U1  Output shape.  n_rows rows in, n_rows rows out; row t keeps its winding.  Floats 18-35 are the source row's on the bits.
 *     Floats 9-17 are N1 of ezrt_vertices.h for the OUTPUT row, in all three corners (as S8 of ezrt_subdivide.h); a degenerate output
 *     row gets NaN.  Non-finite input gets no special treatment: NaNs propagate.
 * U2  Usable, active.  A corner is USABLE exactly as in S4 of ezrt_subdivide.h: v = vertex[c] is in 0 .. 3 n_rows - 1, lo =
 *     star_offsets[v] and hi = star_offsets[v + 1] satisfy 0 <= lo < hi <= 3 n_rows, and every entry of star[lo .. hi) is in
 *     0 .. 3 n_rows - 1.  Vertex v is ACTIVE when some usable corner names it and f = star[star_offsets[v]] has vertex[f] == v (on a
 *     weld's own arrays f is vert_corner[v]).  A corner is ACTIVE when it is usable and its vertex is active.  Only stars of vertices
 *     that a corner names are ever walked: entries of star_offsets beyond V are never looked at.
 * U3  State.  x_0(v) is the stored position of corner f.  pos_j(c) is x_j(vertex[c]) for an ACTIVE corner; for every other corner
 *     pos_j(c) is the corner's own stored position, at every j.
 * U4  The rule of a vertex.  It is fixed for all steps and comes from the arrays alone.  SMOOTH when vert_flags[v] == 0.  BORDER when
 *     vert_flags[v] == 1, EZRT_SMOOTH_PIN_BORDER is not set, and S6's walk counts r == 2 terms: over the star in ascending order it
 *     takes pa(c') when edge_class of the half-edge that LEAVES c' is 1, then pb(c') when edge_class of the half-edge that ENTERS c'
 *     is 1.  KEPT otherwise: a non-manifold edge, a pinched vertex, a pinned border, r != 2.
 * U5  Weight.  Steps are j = 0 .. steps - 1; w_j = lambda for even j and mu for odd j.  mu == lambda is the plain umbrella operator;
 *     lambda = 0.5f, mu = -0.53f is Taubin's lambda|mu fairing.
 * U6  SMOOTH step.  k = hi - lo.  S is the sum, starting from +0, over the star in ascending order, of (pos_j(pa(c')) +
 *     pos_j(pb(c'))), the inner sum formed first.  m = S / (float)(2 * k) per component.
 *       x_{j+1} = x_j + w_j * (m - x_j)
 *     (one subtraction, one product, one sum).  (On a manifold fan every neighbour is in S twice.)
 * U7  BORDER step.  B = (+0 + first term) + second term in the walk's order, read through pos_j.  m = B * 0.5f.  The update is U6's.
 * U8  KEPT, and the output.  A KEPT vertex has x_{j+1} = x_j.  A corner whose vertex is ACTIVE and SMOOTH or BORDER gets
 *     x_steps(v).  Every other corner keeps its own stored bits, a -0 included.
 * U9  Summary (int64[8]).  [0] n_rows; [1] corners under SMOOTH; [2] corners under BORDER; [3] every other corner; [4] ACTIVE
 *     vertices; [5] steps; [6] flags; [7] 0.  [1] + [2] + [3] = 3 n_rows.
 *
 * What follows from U1 .. U9.
 * - Nothing depends on how the work was split, on the route, on tile_rows, on the arrival order of threads or on what `work` held.
 * - Reversing every winding (p1 with p2, and the topology and weld of the reversed rows) gives the same points: the sums pa + pb
 *   and B's two terms commute.
 * - A permutation of the triangle ids changes the order of U6's sum, so it may change last bits: the limit of N2 of ezrt_vertices.h.
 * - All corners of a moved vertex get the same bits, so the weld and the topology, taken by value, still describe the output.
 *   STATED LIMIT: that holds as long as no two vertices round onto one value; then the output's own weld sees one vertex.
 * - steps = a + b is steps = a and then steps = b on the output, with the same arrays, when a is even.
 * - The plain umbrella operator shrinks a closed mesh and Taubin's pair largely does not: an observation, not a rule.
 *
 * THE CALLS.
 * ezrt_smooth_work_bytes(n_rows) does no device work: the bytes of `work` a call needs -- a pure function, monotone in n_rows, a
 * multiple of 8, 8 for n_rows <= 0, and otherwise, with H = 3 n_rows, b = ceil(H / 256) and c = ceil(b / 2048),
 *   45 H + 8 (b + 1) + 8 (c + 1), rounded up to a multiple of 8
 * : per corner two positions of 12 B (the two buffers), two terms of 4 B, a record of 12 B for a vertex that moves and a byte of
 * state; one int64 per 256 corners for the compaction and the scan's tiles.  About 135 B per row, never above
 * ezrt_weld_work_bytes(n_rows): a caller who has just welded these rows can hand the same buffer on.
 * ezrt_smooth_limits reports tile_rows_max as compiled: the rows the LDS route holds.
 * ezrt_smooth_rows_device reads tri36 and writes out (U1 .. U8) and summary (U9).  The five arrays are given at the full sizes that
 * ezrt_mesh_topology_device and ezrt_mesh_weld_device write (the weld with its flags group) and are taken BY VALUE, as
 * ezrt_subdivide_rows_device takes them: nothing is trusted, nothing is read or written out of bounds.  `s` supplies the device and
 * the error slot only: n_rows need not be the scene's n_tri.  out == tri36 exactly is allowed, so a deformation loop can smooth in
 * place; any other overlap is rejected.  work is scratch of at least ezrt_smooth_work_bytes(n_rows) bytes, 8-byte aligned, whose
 * contents before and after the call mean nothing; two calls in flight at once need two.  tile_rows picks the route of the steps:
 * 0 is the library's choice, anything else is clamped to [1, tile_rows_max]; it changes the time of a call and nothing of its answer.
 *
 * How it is computed.  A memset of the summary.  PLAN, once per call, two launches and the tiled prefix sum between them: one lane
 * per corner decides U2 and U4 -- the lane that is the first entry of its vertex's star walks the star once -- copies its position into both
 * buffers and counts the moving vertices of its workgroup; the counts are scanned; then one lane per index resolves every term of
 * U6 and U7 to a SLOT (the first corner f for an ACTIVE vertex, the corner itself otherwise: these cannot collide), so that a step
 * reads a contiguous term list per vertex, 2 x 4 B per star corner, and does not chase star -> row -> vertex again; the same lanes
 * compact the moving vertices into records, so that a step launches only lanes that work.  STEP, global route: one launch per step;
 * one lane per moving vertex sums its terms in order from buffer j & 1 and writes buffer (j + 1) & 1.  (The number of records M is
 * known on the device only and the call does not synchronise: a step is launched with min(ceil(3 n_rows / 256), 2048) workgroups
 * that stride over the records, and those beyond M read M and exit.)  STEP, LDS route (the
 * precedent is tile_rows of ezrt_point_queries.h's plane loops): when n_rows <= tile_rows ONE workgroup keeps both buffers in LDS
 * and runs all steps in one launch with a workgroup barrier between steps -- 100 steps on a collision proxy of a few hundred rows
 * are one launch instead of 100.  FILL: at most 2048 workgroups stride over tiles of 64 consecutive rows; a workgroup stages a tile in
 * LDS with the lanes laid over its float4s, replaces the positions from the final buffer, computes N1 and stores 16 B per lane at
 * consecutive addresses; rows that are not 16-byte aligned take a per-lane route to the same bits; with out == tri36 a tile (a row)
 * is read whole before it is written.  No floating-point atomics; the summary is reduced over the wave and the workgroup and added
 * with one int64 atomic per workgroup and term; no grid-wide barrier, no workgroup waits for another; the only loops not bounded by a
 * constant are the walk of a star, at most 3 n_rows steps, the steps, and a workgroup's stride over tiles and records; the buffers
 * cross launch boundaries.  KNOWN LIMIT: a vertex of valence k costs k sequential gathers per step in one lane.
 * One step reads 12 B of record, 12 B of position and, per star corner, 8 B of terms and 24 B of positions, and writes 12 B: with V
 * moving vertices and K star corners 36 V + 32 K bytes, on a closed manifold (V = n_rows / 2, K = 3 n_rows) 114 B per row.
 * Measured on one MI355X (profiles/r41/smooth_rates.txt; device events, median of 7 repeats, Taubin's pair), beside a
 * device-to-device copy of the bytes one step reads plus writes.  The Bunny scene at 1 272 140 rows (636 408 vertices, 145 MB per
 * step): a call of 1 step 0.447 ms, of 10 steps 1.051 ms, so 0.067 ms per step beside 0.021 ms for the copy, 3.2 times it.  A strip
 * of 10^6 rows with shuffled ids (every vertex on the border, 132 MB per step): 0.658 and 1.054 ms, 0.044 ms per step beside
 * 0.019 ms, 2.4 times -- beside 3.18 and 3.07 ms for the topology and 1.62 and 1.72 ms for the weld of the same rows.  Both copies run
 * out of the Infinity Cache (about 7 TB/s), and so do the steps (2.2 and 3.0 TB/s).  A call of one step is mostly the plan and
 * the fill: about 0.38 ms (0.61 ms on the strip) of it are not the step.  KNOWN LIMIT: the step is bound by its dependent
 * gathers, a record, then k pairs of terms, then 2 k positions of 12 B through 4-byte indices, in one lane; written down, not cured.
 * The LDS route at tile_rows_max = 832 rows (the tests' pool: 886 moving vertices, 1915 star corners): 100 steps 0.361 ms in one
 * launch beside 0.588 ms in 100 launches, 1.6 times; 1 step 0.074 beside 0.071 ms, so a step costs 2.9 us in LDS and 5.2 us as a
 * launch, and 100 steps cost 4.9 times what one does, not the same.  KNOWN LIMIT of that route: one workgroup of 512 lanes on one
 * CU, whose every step reads its records and terms from global memory again and reaches LDS through generic pointers (flat
 * loads and stores, not ds_ ones); the launches it saves are what it gains.  The two routes gave the same bits.
 *
 * Memory, streams, ordering and errors are those of ezrt_subdivide.h: every pointer is device memory of the scene's device, large
 * enough for its elements (anything else is rejected before any launch, never dereferenced); the work is enqueued on `stream` and
 * the call returns without synchronising or allocating; it may run beside ezrt_render_device and the other queries on other streams
 * and leaves ezrt_counters and ezrt_last_render_ms alone.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): a NULL argument; n_rows < 0 or above INT32_MAX / 3; steps outside
 * 1 .. EZRT_SMOOTH_STEPS_MAX; a non-finite lambda or mu; unknown flag bits; tile_rows < 0; a partial overlap of out with tri36;
 * work_bytes below ezrt_smooth_work_bytes(n_rows) or work not 8-byte aligned; a pointer that is not device memory of the scene's
 * device.  n_rows == 0 returns 0 and launches nothing (out and summary are then not written either). */
#ifndef EZRT_SMOOTH_H
#define EZRT_SMOOTH_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_SMOOTH_PIN_BORDER 1
#define EZRT_SMOOTH_STEPS_MAX 1024

/* the bytes of `work` for n_rows rows (pure, monotone, a multiple of 8; no device work; never fails) */
size_t ezrt_smooth_work_bytes(int n_rows);
/* the rows the LDS route holds, as compiled (a host pointer; no device work) */
void ezrt_smooth_limits(int* tile_rows_max);
int ezrt_smooth_rows_device(EzrtScene* s, const float* tri36 /* n_rows x 36, the caller's rows */, int n_rows,
                            const uint8_t* edge_class /* 3 n_rows */, const int32_t* vertex /* 3 n_rows */,
                            const int32_t* star_offsets /* 3 n_rows + 1 */, const int32_t* star /* 3 n_rows */,
                            const uint8_t* vert_flags /* 3 n_rows */, int steps, float lambda, float mu, int flags, int tile_rows,
                            float* out /* n_rows x 36, or tri36 itself */, int64_t* summary /* 8 */, void* work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
