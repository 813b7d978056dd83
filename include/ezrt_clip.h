/* ezrt_clip.h -- stream-ordered PLANE CLIPPING on device memory (libezrt_hip.so only): the half of a mesh on one side of a plane, as
 * triangle rows.
 *
 * ezrt_plane.h returns the section of a mesh as segments, ezrt_plane_loops.h chains them into polylines, ezrt_boundary.h closes the
 * holes of a mesh that already has them.  None of them takes the caller's rows and a plane and returns the rows of the half-space
 * a x + b y + c z >= d.  With it the library cuts a part in two: clip, a new scene of the rows, topology, boundary, cap, a new scene of
 * the rows and the cap -- closed, so that ezrt_inside.h, ezrt_winding.h and the signed volume of ezrt_orient.h are valid on either
 * half.  Section views, the volume above or below a level, a scan trimmed to a box with six calls in a row.  It is the library's first
 * call that writes TRIANGLE ROWS as a variable-length answer; it uses the count / offsets / fill pattern of ezrt_plane.h and
 * ezrt_overlap_list.h.
 *
 * THE DEFINITION.  The arithmetic is that of ezrt_plane.h (P1, P2, P4), by the same device functions, and one interpolation (K5).  No
 * contraction anywhere; one rounding per written operation.
 *
 * K1  Inputs by value.  The call reads the CALLER's rows tri36, n_rows x 36 floats: floats 0-8 are p1 p2 p3, 9-17 n1 n2 n3, 18-35 the
 *     material -- the rows of ezrt_scene_create -- and one plane, plane4: 4 floats (a, b, c, d) in device memory.  `s` supplies the
 *     device and the error slot only: n_rows need not be the scene's n_tri, and the output of one call is the input of the next.  The
 *     plane is LIVE as in P1 of ezrt_plane.h.  A plane that is not live keeps nothing: T = 0 and summary[6] = 0.
 * K2  Sides.  s(v) is P2 of ezrt_plane.h (the device function plane_side).  A vertex is UP when s(v) >= 0 (-0 is >= 0) and DOWN when
 *     s(v) < 0.  A row with a non-finite coordinate among floats 0-8 takes no part: it emits nothing and is counted in summary[4].
 * K3  Pieces per row, from the three sides alone; v[0] v[1] v[2] are p1 p2 p3 and indices are mod 3.
 *     - all UP: one piece, the row itself, all 36 floats copied on the bits;
 *     - all DOWN: nothing;
 *     - one UP vertex U = v[i] with s(U) != 0: one piece (U, q0, q1), q0 P4's point of the edge v[i] -> v[i + 1] and q1 P4's point of
 *       the edge v[i + 2] -> v[i];
 *     - one UP vertex with s(U) == 0: nothing.  The row only touches the plane;
 *     - one DOWN vertex D = v[i], with a = v[i + 1] and b = v[i + 2]: let Pb be P4's point of b -> D and Pa P4's point of D -> a.  Piece
 *       (a, b, Pb) is emitted when s(b) != 0, then piece (a, Pb, Pa) when s(a) != 0.
 *     The count of a row is 0, 1 or 2.  It never depends on P4's arithmetic.  Every piece keeps the winding of its row.
 * K4  Points.  New positions are P4 of ezrt_plane.h (the device function plane_point): a function of the edge's two values and the
 *     plane ALONE, whichever way round the edge is held.  Kept vertices are copied on the bits.
 * K5  Normals and materials of a cut piece.  A kept vertex keeps its corner's normal on the bits.  A new vertex sits on the edge with
 *     the ends A < B, in P4's order of the VALUES of the positions, with P4's t = s(A) / (s(A) - s(B)).  If s(A) == 0 it gets A's normal
 *     on the bits; else if s(B) == 0 it gets B's; else per component
 *       (float)((double)nA + t * ((double)nB - (double)nA))
 *     with every operation rounded once, no contraction, NOT renormalised (the interpolated shading normal of the row at that point,
 *     which a renderer normalises where it uses it).  Floats 18-35 are the source row's on the bits.  The sign and payload of a NaN
 *     normal are not part of the contract.
 * K6  Order.  Output rows are in ascending source row, then in the piece order of K3.  offsets is int64 with n_rows + 1 entries: the
 *     exclusive prefix sum of the counts, T in offsets[n_rows].  src[r] is the source row of output row r.  cut_edge[r] is the edge of
 *     output row r (edge e runs from its vertex e to its vertex (e + 1) % 3) that lies on the plane as a result of the cut: 1 for
 *     (U, q0, q1) and for (a, Pb, Pa); 2 for (a, b, Pb) when s(a) == 0; otherwise -1.
 * K7  Summary (int64[8]).  [0] T; [1] rows kept whole; [2] rows that emit cut pieces; [3] rows with finite coordinates that emit
 *     nothing; [4] rows with a non-finite coordinate; [5] output rows with cut_edge >= 0; [6] 1 when the plane is live, else 0; [7] 0.
 *     [1] + [2] + [3] + [4] = n_rows.
 * K8  Fill trusts nothing.  The fill call recomputes a row's count c and writes the row's pieces only when offsets[k] >= 0,
 *     offsets[k] + c <= capacity and offsets[k + 1] - offsets[k] == c.  A SOURCE row is written whole or not at all: all of its pieces, or
 *     none.  Offsets that a count call left send every source row to output rows of its own; with other offsets several source rows
 *     may pass the three tests for one output row, and that row then holds, word by word, the word of any of them.  Output rows that belong
 *     to no source row are not touched, and nothing outside out, src, cut_edge [0 .. capacity) is written whatever offsets holds.  The
 *     caller sees an overflow in offsets[n_rows] > capacity and may call again with larger arrays; the count need not be repeated.
 *
 * STATED LIMIT.  P4 may round a point onto an end of its edge, so a piece may have two equal vertices.  The topology ignores such a
 * triangle (the M-rules of ezrt_topology.h).  They are emitted and not filtered.
 *
 * What follows from K1 .. K8.
 * - Nothing depends on how the work was split, on the route of the fill, on the arrival order of threads or on what `work` held.
 * - Rotating a row's vertices within its winding changes no cut piece to a bit: the pieces are named from U or D, and P4 does not
 *   depend on the direction of an edge.  (A row kept whole is the row as it is held.)
 * - Reversing the winding of a row (p2 with p3, n2 with n3) reverses every piece: the same triangles, each with the other winding.
 *   With one DOWN vertex the two pieces are then split along the other diagonal of the same quadrilateral.
 * - A clip and the clip by the negated plane together emit every vertex of every row with finite coordinates, a vertex ON the plane
 *   possibly in neither (a row that touches either plane from outside emits nothing).
 * - On a closed, consistently wound manifold the clipped rows have no FLIPPED and no NONMANIFOLD edge: a cut edge is shared, by P4 on
 *   the bits, by the two rows that shared the edge it lies on.
 * - The cut edge of an output row is q0 -> q1 of P5 of ezrt_plane.h for its source row, on the bits: a source row has exactly one
 *   output row with a cut edge when it emits cut pieces, and none otherwise.  A crossed row that emits nothing touches the plane from
 *   below, with a vertex (a segment of length zero) or with an edge.
 * - On such a mesh the BOUNDARY half-edges of the clipped rows, as (start, end) on the bits and in direction, are exactly the rows of
 *   non-zero length of the section of ezrt_plane.h for the same plane -- after the section's pairs of opposite rows are taken out: an
 *   edge IN the plane whose two triangles both lie below it is in the section once each way and bounds nothing above the plane (the
 *   lowest ring of a torus under the plane through it).  Held by the numpy restatement on a cube, the voxel solid and a torus of 2048
 *   triangles under some forty planes each, among them axis planes exactly through vertices, with both signs, and planes that put
 *   vertices within rounding of the plane (tests/test_clip_expected.py).
 * - ezrt_mesh_boundary_device on a scene of the clipped rows therefore returns the loops of ezrt_plane_loops.h, and
 *   ezrt_cap_rows_device closes them with caps that face -(a, b, c), which is outward.
 *
 * THE CALLS.
 * ezrt_clip_work_bytes(n_rows) does no device work: the bytes of `work` a count call over n_rows rows needs -- a pure function,
 * monotone in n_rows, a multiple of 8, 8 for n_rows <= 0:
 *   8 ceil(n_rows / 2048) + 8
 * (an int64 per scan tile of 2048 rows, and one for their total).
 * ezrt_clip_count_device writes offsets (K6) and summary (K7).  work is scratch of at least ezrt_clip_work_bytes(n_rows) bytes, 8-byte
 * aligned, whose contents before and after the call mean nothing; two calls in flight at once need two.
 * ezrt_clip_rows_device takes tri36, n_rows and plane4 as given to the count call and offsets as it left them, and writes rows
 * offsets[k] .. offsets[k + 1] of out, src and cut_edge for every source row k (K3 .. K6, K8).  src and cut_edge may be NULL.
 *
 * How it is computed.  COUNT: a memset of the summary, then one lane per row: nine coordinates, three sides, the K3 count as int64 into
 * offsets[k]; the summary's terms are reduced over the wave and added with one int64 atomic per wave and term.  SCAN: the tiled prefix
 * sum of ezrt_vertices.h in place (a tile's sum, a scan of the sums, the tile's scan: three launches).  FILL: a workgroup owns a tile of
 * 256 consecutive rows.  It classifies them one lane per row and puts the destination of every row kept whole into LDS; then the lanes
 * are laid over the tile's 2304 float4s -- entry f belongs to row f / 9, part f % 9 -- so that a wave loads 1 KiB of consecutive
 * addresses per instruction and stores consecutive addresses wherever kept rows follow one another; afterwards the cut rows, which
 * are few, are written by their own lanes.  That route needs tri36 and out 16-byte aligned; otherwise every lane copies its own row
 * float by float, to the same bits.  No floating-point atomics, no grid-wide barrier, no workgroup waits for another, and no loop
 * that is not bounded by a constant.
 * Measured on one MI355X (profiles/r34/clip_rates.txt): 10^6 rows kept whole, count 0.40 ms, fill 0.071 ms beside 0.055 ms for a
 * device-to-device copy of the bytes the fill reads plus writes, and 0.93 ms on the per-lane route.  KNOWN LIMIT: cut rows are written
 * by their own lanes float by float on both routes; 10^6 rows cut in every row (1.5 * 10^6 pieces) take 0.56 ms, 8 times their copy.
 *
 * Memory, streams, ordering and errors are those of ezrt_boundary.h: every pointer is device memory of the scene's device, large
 * enough for its elements (anything else is rejected before any launch, never dereferenced); the work is enqueued on `stream` and the
 * call returns without synchronising or allocating; it may run beside ezrt_render_device and the other queries on other streams and
 * leaves ezrt_counters and ezrt_last_render_ms alone.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): any NULL pointer (the stream, src and cut_edge excepted; out may be NULL
 * with capacity == 0); n_rows < 0 or above INT32_MAX / 2; capacity < 0 or beyond what an array can hold; work_bytes below
 * ezrt_clip_work_bytes(n_rows) or work not 8-byte aligned; out overlapping tri36; a pointer that is not device memory of the scene's
 * device.  n_rows == 0 returns 0 and launches nothing (offsets and summary are then not written either). */
#ifndef EZRT_CLIP_H
#define EZRT_CLIP_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the bytes of `work` for n_rows rows (pure, monotone, a multiple of 8; no device work; never fails) */
size_t ezrt_clip_work_bytes(int n_rows);
int ezrt_clip_count_device(EzrtScene* s, const float* tri36 /* n_rows x 36, the caller's rows */, int n_rows, const float* plane4 /* 4 */,
                           int64_t* offsets /* n_rows + 1 */, int64_t* summary /* 8 */, void* work, size_t work_bytes, void* stream);
int ezrt_clip_rows_device(EzrtScene* s, const float* tri36 /* n_rows x 36 */, int n_rows, const float* plane4 /* 4 */,
                          const int64_t* offsets /* n_rows + 1 */, int64_t capacity, float* out /* capacity x 36 */,
                          int32_t* src /* capacity, or NULL */, int8_t* cut_edge /* capacity, or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
