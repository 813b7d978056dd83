/* ezrt_plane_loops.h -- stream-ordered plane LOOPS on device memory (libezrt_hip.so only): a section's segments chained into polylines.
 *
 * ezrt_plane.h returns the cross-section of the mesh as a soup of oriented segments, one row per crossed triangle in ascending id, and
 * its rule P4 gives two triangles that share an edge by value the same end point ON THE BITS.  A slicer, a contour plot and a girth
 * need ordered loops.  The call here chains the rows of a section that is already on the device, by comparing bits and nothing else,
 * and returns the loops in CSR form: count / offsets / fill once more, with the loops as the rows.
 *
 * Input: a section as ezrt_query_plane_section_device leaves it -- offsets[n + 1] (int64) and seg[capacity x 6] (q0 then q1).  Row
 * indices below are GLOBAL row indices into seg.
 *
 * THE DEFINITION.  Every answer is a set of integers; no floating-point operation and no floating-point comparison occurs anywhere.
 *
 * L1  Key.  The key of an end point is its 12 bytes as three uint32 bit patterns, together with the plane index.  Comparison is on
 *     bits: -0 and +0 differ (as ezrt_plane.h says of a vertex stored both ways), and a NaN equals itself when its bits do.
 * L2  Chained planes.  Plane i is CHAINED when 0 <= offsets[i] <= offsets[i + 1] <= capacity and offsets[i + 1] - offsets[i] <= n_tri
 *     (the scene's triangles: no section of this scene has a longer row).  Any other plane has no loops, and none of its rows is
 *     read or written.  This covers a section that did not fit its capacity (the planes past the capacity are not chained, those
 *     before it are), and garbage in offsets.  Whatever offsets holds, nothing outside the output arrays' stated sizes is written
 *     and every loop in every kernel terminates.
 * L3  Degenerate rows.  A row whose q0 and q1 have equal bits is DEGENERATE: P3's zero-length segments (a triangle touching the plane
 *     with one vertex from below) and degenerate triangles.  Such a row belongs to no chain: its next is -1 and it does not appear
 *     in order.
 * L4  Pairing.  Within a chained plane and for a key k, OUT(k) is the non-degenerate rows with q0 == k in ascending row order, and
 *     IN(k) the non-degenerate rows with q1 == k in ascending row order.  For j < min(|IN(k)|, |OUT(k)|): next[IN(k)[j]] = OUT(k)[j].
 *     Every other non-degenerate row has next = -1.  Every row therefore has at most one successor and at most one predecessor, and
 *     the result is a function of the section alone, never of the order in which threads arrive.
 * L5  Chains.  The components of next are open paths and cycles.  The HEAD of a path is its row without a predecessor; the head of a
 *     cycle is its lowest row.  pos is the number of next steps from the head.
 * L6  Numbering and output.  Loops are numbered plane by plane and within a plane in ascending order of their head row -- for
 *     ascending offsets (every section's) that is the ascending order of head rows.
 *       plane_loops[i]                   the index of the first loop of plane i; plane_loops[n] is the total L
 *       loop_offsets[l]                  the exclusive prefix sum of the loop lengths; loop_offsets[L] is the number of chained rows
 *       order[loop_offsets[l] + p]       the row at position p of loop l
 *       closed[l]                        1 for a cycle, 0 for an open path
 *     The polyline of loop l is the q0 of its rows in that order; a closed loop returns to the first point, an open one appends the
 *     last row's q1.
 *
 * What follows from L1 .. L6.
 * - On a closed, consistently wound manifold in which no key has a multiplicity above 1 every non-degenerate row has exactly one
 *   successor and one predecessor (ezrt_plane.h, "Loops": every bit pattern occurs as often as a q0 as it does as a q1): EVERY LOOP
 *   IS CLOSED.
 * - Nothing depends on the tree or on `slices`: the section does not, and nothing else is read.
 * - Flipping every winding swaps q0 and q1 of every row (P5) and so IN and OUT of every key: every loop is REVERSED (the same rows,
 *   the opposite direction; heads of open paths become tails, heads of cycles stay).
 * - Permuting the triangle ids permutes the rows inside each plane.  Where no key repeats, next is the same relation on the
 *   segments, and the SET of cyclic point sequences is unchanged; heads, and with them the numbering and the starting points, change.
 *   Where a key repeats (two solids touching along an edge, a fan around a vertex on the plane) the pairing by ascending row does
 *   depend on the ids: it is pinned, not canonical.
 * - Orientation is P5's: for outward counter-clockwise windings outer loops run counter-clockwise seen from the side the plane's
 *   normal points to, and holes run clockwise; the signed area 1/2 sum n^ . (q0 x q1) of a closed loop is positive for the former.
 *
 * THE CALL.
 * ezrt_plane_loops_work_bytes(capacity) does no device work: the bytes of `work` a call with that capacity needs -- a pure function,
 * monotone in capacity, 8 for capacity <= 0.  ezrt_plane_loops_limits reports tile_rows_max as compiled.
 * ezrt_plane_loops_device reads offsets and seg and writes
 *   next          (capacity, or NULL) L4, for every row of a chained plane; rows of planes that are not chained, and rows that
 *                 belong to no plane, are not touched;
 *   order         (capacity) L6; entries at or beyond the number of chained rows, loop_offsets[L], are not touched;
 *   plane_loops   (n + 1) L6;
 *   loop_offsets  (loop_capacity + 1) and closed (loop_capacity, or NULL): loops with index >= loop_capacity are not written to
 *                 either, and loop_offsets[L] is written when L <= loop_capacity.  next, order and plane_loops do not depend on
 *                 loop_capacity: the caller sees the overflow in plane_loops[n] > loop_capacity and may call again.
 * `s` supplies the device, the error slot and n_tri.  work is scratch of at least ezrt_plane_loops_work_bytes(capacity) bytes,
 * 8-byte aligned, whose contents before and after the call mean nothing; two calls in flight at once need two.
 * tile_rows changes the time of a call and nothing of its answer: a chained plane of at most tile_rows rows is joined and ranked in
 * the LDS of one workgroup, a longer one in `work`; 0 is the library's choice, anything else is clamped to [1, tile_rows_max].
 *
 * How it is computed.  One workgroup per plane (two kernels: the LDS route and the global route; each leaves the other's planes
 * alone).  JOIN: an open-addressed table of 2 x rows slots; a slot is claimed for a key by atomicCAS with a representative row and
 * keys are compared by reading the representative's q0 in seg, which is read-only; only q0 keys are inserted (at most one per row:
 * the table is at most half full), q1 keys are looked up.  Each slot heads two lock-free lists, of its OUT rows and of its IN rows; a
 * row's rank is the number of list members with a lower row; next of the IN row of rank j is the OUT row of rank j.  With
 * multiplicity 1 that is one probe and one compare.  RANKING: ceil(log2(rows)) rounds of pointer jumping along the predecessor give
 * paths their head and pos; rows that have not reached a head by then lie on cycles, as many rounds of min-doubling along next find
 * each cycle's lowest row, the cycle is cut before it and ranked by as many rounds again (planes without a cycle skip both).
 * COMPACTION: the heads of a plane are counted and numbered by a workgroup scan; one workgroup sums the planes' counts into
 * plane_loops; the tail of every chain writes its loop's length; one workgroup sums the lengths; a last kernel scatters order,
 * next, loop_offsets and closed.  Probes are bounded by the table's size, list walks by the plane's rows, rounds by the row count,
 * and every index read back from `work` is checked against the plane's rows before it is used.
 *
 * Memory, streams, ordering, refit interaction and errors are those of ezrt_plane.h: every pointer is device memory of the scene's
 * device, large enough for its elements (anything else is rejected before any launch, never dereferenced); work is enqueued on
 * `stream` and the call returns without synchronising or allocating; the call may run beside ezrt_render_device and the other
 * queries on other streams and leaves ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for it.  The
 * call reads no geometry: after a refit it is the section that has to be taken again.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, offsets, plane_loops, loop_offsets or work; NULL seg or
 * order with capacity > 0; n < 0, capacity < 0, loop_capacity < 0, tile_rows < 0; a capacity beyond what an array can hold
 * (PTRDIFF_MAX / 64 rows); work_bytes below ezrt_plane_loops_work_bytes(capacity) or work not 8-byte aligned; a pointer that is not
 * device memory of the scene's device.  n == 0 returns 0 and launches nothing (plane_loops[0] is then not written either). */
#ifndef EZRT_PLANE_LOOPS_H
#define EZRT_PLANE_LOOPS_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the bytes of `work` for a call with this capacity (pure, monotone; no device work; never fails) */
size_t ezrt_plane_loops_work_bytes(int64_t capacity);
/* the limit as compiled (no device work; never fails) */
void ezrt_plane_loops_limits(int* tile_rows_max);
int ezrt_plane_loops_device(EzrtScene* s, const int64_t* offsets /* n + 1 */, int n, const float* seg /* capacity x 6 */, int64_t capacity,
                            int tile_rows /* 0: library's choice */, int64_t* next /* capacity, or NULL */, int64_t* order /* capacity */,
                            int64_t* plane_loops /* n + 1 */, int64_t loop_capacity, int64_t* loop_offsets /* loop_capacity + 1 */,
                            uint8_t* closed /* loop_capacity, or NULL */, void* work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
