/* ezrt_subdivide.h -- stream-ordered SUBDIVISION on device memory (libezrt_hip.so only): four triangle rows per row of the caller's
 * mesh, by midpoints or by Loop's scheme.
 *
 * The mesh calls of this library weld (ezrt_vertices.h), orient (ezrt_orient.h), find boundaries and cap (ezrt_boundary.h) and clip
 * (ezrt_clip.h), and every one of them returns at most the resolution it was given.  The call here refines: the caller's rows in,
 * four rows per row out.  MIDPOINT mode is the host's scenes.subdivide on the bits.  LOOP mode is Loop's scheme with Warren's weights;
 * its boundary and crease rules are read from the edge classes of ezrt_topology.h and the vertex flags of ezrt_vertices.h.  It is the
 * second call that writes TRIANGLE ROWS (after ezrt_clip.h) and the first whose output size is known before it runs: there is no
 * count / offsets / fill, and nothing to synchronise for.
 *
 * THE DEFINITION.  All arithmetic is fp32, one rounding per written operation, no contraction; division is IEEE.  Corner c = 3 t + k
 * is stored vertex k of row t; half-edge h = 3 t + e runs from stored vertex e to stored vertex (e + 1) % 3 (M3 of ezrt_topology.h).
 * "Key" is M1 of ezrt_topology.h.  Floats 0-8 of a row are p0 p1 p2 (p1 p2 p3 of ezrt_scene_create), 9-17 its corner normals, 18-35
 * its material.
 *
 * S1  Output shape.  Row t yields exactly four rows, in this order:
 *       4 t + 0 = (P0, E0, E2)    4 t + 1 = (E0, P1, E1)    4 t + 2 = (E2, E1, P2)    4 t + 3 = (E0, E1, E2)
 *     Pk the new point of corner k, Ee the new point of half-edge e.  Every piece keeps the winding of its row.  Rows with non-finite
 *     or repeated vertices get no special treatment: NaNs propagate.  Floats 18-35 of all four rows are the source row's on the bits.
 * S2  Midpoint mode.  Pk is pk on the bits.  Ee = (a + b) * 0.5f per component, a and b the two ends: fp32 addition is commutative, so
 *     both rows on an edge get the same bits whichever way they hold it.  (The arithmetic of scenes.subdivide.)  A kept corner keeps
 *     its corner normal on the bits; an edge point gets (na + nb) * 0.5f of its OWN row's two corner normals, not renormalised, as K5
 *     of ezrt_clip.h.
 * S3  Loop edge rule.  Half-edge h is INTERIOR when edge_class[h] is 2 or 3; g = twin[h] lies in 0 .. 3 n_rows - 1; g / 3 != t; and
 *     the unordered pair of keys of g's two ends, read from the CALLER's rows, equals that of h's.  Then, with c the third vertex of
 *     row t and d the third vertex of row g / 3,
 *       Ee = 0.375f * (a + b) + 0.125f * (c + d)
 *     (two sums, two products, one sum).  Otherwise Ee is S2's midpoint.  Both sides of an honest edge compute the same bits: a + b
 *     and c + d commute.
 * S4  Usable corner.  Corner c is USABLE when v = vertex[c] is in 0 .. 3 n_rows - 1; lo = star_offsets[v] and hi = star_offsets[v + 1]
 *     satisfy 0 <= lo < hi <= 3 n_rows; and every entry of star[lo .. hi) is in 0 .. 3 n_rows - 1.  Nothing out of bounds is read or
 *     written, whatever the arrays hold.
 * S5  Smooth vertex.  A USABLE corner with vert_flags[v] == 0.  k = hi - lo.  S is the sum, starting from +0, over the star in ascending
 *     order, of (pa(c') + pb(c')), the inner sum formed first; pa is the next stored vertex of c''s row and pb the one after.
 *     beta = 0.1875f when k == 3, else 0.375f / (float)k.
 *       Pk = (1.0f - (float)k * beta) * p + (beta * 0.5f) * S
 *     with p the corner's OWN position.  (On a manifold fan every neighbour is in S twice.)
 * S6  Border vertex.  A USABLE corner with vert_flags[v] == 1.  Walk the star in ascending order, from B = +0 and r = 0: add pa(c')
 *     when edge_class of the half-edge that LEAVES c' is 1, then add pb(c') when edge_class of the half-edge that ENTERS c' is 1,
 *     counting the terms in r.  When r == 2, Pk = 0.75f * p + 0.125f * B.  Otherwise S7.
 * S7  Kept vertex.  Every other corner has Pk = pk on the bits: a non-manifold edge, a pinched vertex, vertex[c] == -1, unusable arrays.
 * S8  Loop normals.  All three corners of an output row get N1 of ezrt_vertices.h for that OUTPUT row, the face normal.  No special
 *     cases: a degenerate piece gets NaN.  Smooth normals are a weld and ezrt_vertex_normals_device on a scene of the output.
 * S9  Summary (int64[8]).  [0] 4 n_rows; [1] corners under S5; [2] under S6; [3] under S7; [4] INTERIOR half-edges; [5] midpoint
 *     half-edges; [6] the mode; [7] 0.  [1] + [2] + [3] = [4] + [5] = 3 n_rows.  In midpoint mode [3] = [5] = 3 n_rows.
 *
 * What follows from S1 .. S9.
 * - Nothing depends on how the work was split, on the route of the fill, on the arrival order of threads or on what `work` held.
 * - Reversing every winding (p1 with p2, and the topology and weld of the reversed rows) gives the same triangles reversed: the
 *   midpoints and S3 are symmetric in their ends, and S5 adds pa + pb before anything else.  (S6's B adds the same two values in the
 *   other order, which commutes.)
 * - Rotating a row's vertices rotates the row's output -- pieces 0, 1, 2 and their vertices -- and changes no point.
 * - A permutation of the triangle ids changes the order of S5's sum, so it may change last bits: the limit of N2 of ezrt_vertices.h.
 * - On a closed manifold of F triangles, E edges and V vertices the output has 4 F triangles, 2 E + 3 F edges and V + E vertices, the
 *   same Euler characteristic, the same components and the same edge classes (a FLIPPED edge yields two FLIPPED edges).
 *   STATED LIMIT: that holds as long as no two new points coincide by value.  Loop's averages can round two points of a very thin
 *   or very small feature onto one value, and then the topology of the output sees a repeated vertex (M2) or a welded one; such
 *   rows are emitted and not filtered, as the clip states of its own.
 *
 * THE CALLS.
 * ezrt_subdivide_work_bytes(n_rows, mode) does no device work: the bytes of `work` a call needs -- a pure function, monotone in
 * n_rows, a multiple of 8, 8 for n_rows <= 0 or MIDPOINT, and in LOOP mode
 *   48 n_rows + 8
 * : four words per possible vertex, 3 n_rows of them -- the 12-byte term of S5 / S6 that does not depend on the corner (T = (beta *
 * 0.5f) * S or 0.125f * B) and one word for the rule and k -- and eight bytes to spare.  The corner's own p is multiplied in where the
 * row is written, which is what keeps S7 and a -0 on the corner's bits.
 * ezrt_subdivide_rows_device reads tri36 and writes out (S1 .. S8) and summary (S9).  In MIDPOINT mode the six topology / weld arrays
 * must all be NULL.  In LOOP mode they must all be given, at the full sizes that ezrt_mesh_topology_device and
 * ezrt_mesh_weld_device write (the weld with its flags group); entries that those calls leave untouched are not looked at.  `s` supplies
 * the device and the error slot only: n_rows need not be the scene's n_tri.  All arrays are taken BY VALUE, as
 * ezrt_vertex_normals_device takes a weld: the rows may have been moved since the weld and the topology were made, as long as the
 * moved rows keep the same coincidences.  work is scratch of at least ezrt_subdivide_work_bytes(n_rows, mode) bytes, 8-byte aligned,
 * whose contents before and after the call mean nothing; two calls in flight at once need two.
 *
 * How it is computed.  A memset of the summary.  VERTEX PASS (Loop mode): one lane per corner; the lane that is the first entry of
 * its vertex's star walks the star once -- O(k) per vertex, because S6 reads edge_class instead of counting multiplicities -- and
 * leaves T, the rule and k in `work`.  FILL, both modes, one launch after it: at most 2048 workgroups stride over tiles of 63
 * consecutive rows.  A workgroup loads a tile into LDS with the lanes laid over their float4s, computes the six new points of every
 * row into LDS, one lane per corner and half-edge (the twin's row and the vertex's slot are gathers), in Loop mode the four face
 * normals, and then lays the lanes over the tile's 2268 OUTPUT float4s -- lane i of 252 always holds part i % 9 of output row
 * 28 round + i / 9 -- so that a wave stores 1 KiB of consecutive addresses per instruction.  That route needs tri36 and out 16-byte
 * aligned; otherwise every lane reads its own row and writes its four rows float by float, to the same bits.  No floating-point
 * atomics; the summary is reduced over the wave and the workgroup and added with one int64 atomic per workgroup and term (MIDPOINT
 * mode counts nothing: its summary is known); no grid-wide barrier, no workgroup waits for another; the only loops not bounded by a
 * constant are the walk of a star, at most 3 n_rows steps, and a workgroup's stride over the tiles; the words of `work` cross a
 * launch boundary.
 * Measured on one MI355X (profiles/r35/subdivide_rates.txt; device events, median of 7 repeats), beside a device-to-device copy of the
 * 720 B per row that the fill reads plus writes.  A strip of 10^6 rows: MIDPOINT 0.144 ms beside 0.136 ms for the copy, 1.06 times it
 * (the Bunny scene at 1 272 140 rows: 0.171 beside 0.169 ms), and 2.04 ms on the per-lane route, 14 times the staged one; LOOP 0.46 ms
 * with the vertex pass and 0.38 ms without it, 2.8 times the copy (the Bunny: 0.41 and 0.33 ms, 2.0 times) -- beside 3.06 ms and
 * 1.72 ms for the topology and the weld of the same rows.  KNOWN LIMIT: LOOP mode's fill is bound by its gathers, not by its stores: a
 * corner reads vertex, star_offsets, star, vertex again and its slot one after the other, a half-edge its twin's row, in 189 of a
 * workgroup's 256 lanes; written down, not cured.
 *
 * Memory, streams, ordering and errors are those of ezrt_clip.h: every pointer is device memory of the scene's device, large enough
 * for its elements (anything else is rejected before any launch, never dereferenced); the work is enqueued on `stream` and the call
 * returns without synchronising or allocating; it may run beside ezrt_render_device and the other queries on other streams and
 * leaves ezrt_counters and ezrt_last_render_ms alone.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, tri36, out, summary or work; n_rows < 0 or above
 * INT32_MAX / 12 (the output still fits the topology's limit of INT32_MAX / 3 triangles); an unknown mode; a partly NULL array group,
 * arrays given in MIDPOINT mode or missing in LOOP mode; out overlapping tri36; work_bytes below
 * ezrt_subdivide_work_bytes(n_rows, mode) or work not 8-byte aligned; a pointer that is not device memory of the scene's device.
 * n_rows == 0 returns 0 and launches nothing (out and summary are then not written either). */
#ifndef EZRT_SUBDIVIDE_H
#define EZRT_SUBDIVIDE_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_SUBDIVIDE_MIDPOINT 0
#define EZRT_SUBDIVIDE_LOOP 1

/* the bytes of `work` for n_rows rows in `mode` (pure, monotone, a multiple of 8; no device work; never fails) */
size_t ezrt_subdivide_work_bytes(int n_rows, int mode);
int ezrt_subdivide_rows_device(EzrtScene* s, const float* tri36 /* n_rows x 36, the caller's rows */, int n_rows, int mode,
                               const int32_t* twin /* 3 n_rows, or NULL with the next five */, const uint8_t* edge_class /* 3 n_rows */,
                               const int32_t* vertex /* 3 n_rows */, const int32_t* star_offsets /* 3 n_rows + 1 */,
                               const int32_t* star /* 3 n_rows */, const uint8_t* vert_flags /* 3 n_rows */, float* out /* 4 n_rows x 36 */,
                               int64_t* summary /* 8 */, void* work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
