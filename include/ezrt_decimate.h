/* ezrt_decimate.h -- stream-ordered DECIMATION on device memory (libezrt_hip.so only): the caller's mesh with its vertices clustered
 * on a uniform grid, as fewer triangle rows.
 *
 * ezrt_subdivide.h refines; every other mesh call of this library returns at most the resolution it was given, and none returns
 * less.  The call here coarsens: the caller's rows and a grid in, and out come the rows whose three vertices fall into three
 * different cells, every vertex moved to the representative point of its cell (vertex clustering, Rossignac and Borrel).  A level of
 * detail for ezrt_scene_create, a proxy for the clearance and overlap queries, a lighter mesh after two Loop levels or after a
 * clip and a cap.  It has the count / offsets / fill form of ezrt_clip.h, and the count also leaves the decimated mesh in INDEXED
 * form: cell (three indices per row) and cell_point (the points).
 *
 * THE DEFINITION.  All floating-point work is IEEE, one rounding per written operation, no contraction.  Corner c = 3 t + k is stored
 * vertex k of row t.  Floats 0-8 of a row are p0 p1 p2 (p1 p2 p3 of ezrt_scene_create), 9-17 its corner normals, 18-35 its material.
 *
 * D1  Grid.  grid4 is four floats (ox, oy, oz, h) in device memory: the origin and the edge of a cell.  It is LIVE when all four are
 *     finite and h > 0.  With a grid that is not live no row takes part: T = 0, every cell[c] = -1, summary[3] = n_rows, [4] = 0,
 *     [7] = 0.
 * D2  Fixed point.  For a coordinate x and its origin component o
 *       u = ((double)x - (double)o) / (double)h      w = u * 16777216.0 (exact)      U = floor(w)
 *     A row TAKES PART when its floats 0-8 are finite and all nine U lie in [-2^44, 2^44).  Then per axis the cell index is
 *     i = U >> 24 (arithmetic shift), in -2^20 .. 2^20 - 1, and the fraction is q = U & 0xFFFFFF: a corner exactly on a face of a cell
 *     belongs to the upper cell.  A row that does not take part has cell = -1 on its three corners, emits nothing and is counted in
 *     summary[3].
 * D3  Cells.  A cell is a triple (ix, iy, iz) that holds at least one corner of a row that takes part; the corners of rows that D6
 *     drops count.  Cells are numbered by their ascending LOWEST corner, as W2 of ezrt_vertices.h numbers vertices: cell[c] is the
 *     number of corner c's cell, cell_corner[j] the lowest corner of cell j, n_cells goes to summary[4].  Entries j >= n_cells of
 *     cell_corner and cell_point are not written.
 * D4  Representative point.  Per cell and axis, N is the number of corners in the cell and S the int64 sum of their q: exact, whatever
 *     the order.  m = (double)S / (double)N and
 *       x = (float)((double)o + ((double)i + m * 0x1p-24) * (double)h)
 * D5  Kept component.  Overrides D4, axis by axis: if every corner of the cell has the same key in that axis -- M1 of
 *     ezrt_topology.h: the bits, -0 as +0 -- the component is that value on the bits (+0 for a zero).  So a vertex alone in its cell is
 *     not moved, and an axis-aligned flat face stays flat.
 * D6  Survivors.  A row that takes part SURVIVES when its three cells are pairwise different; otherwise it has collapsed and is counted
 *     in summary[1].
 * D7  Duplicates.  With EZRT_DECIMATE_DEDUP in flags, among the survivors with the same UNORDERED triple of cells only the lowest row
 *     is kept; the others are counted in summary[2].  Without it every survivor is kept.  Any other bit of flags is an error.
 * D8  Output row.  A kept row t yields one row: floats 0-8 are cell_point of its three cells in stored order (the winding is kept);
 *     all three corner normals are N1 of ezrt_vertices.h, the face normal, of the OUTPUT positions -- a degenerate row gets NaN, as S8
 *     of ezrt_subdivide.h; floats 18-35 are the source row's on the bits.
 * D9  Order and summary.  Rows come out in ascending source row.  offsets is int64 with n_rows + 1 entries, the exclusive prefix sum
 *     of the keeps, T in offsets[n_rows]; src[r] is the source row of output row r.  summary (int64[8]): [0] T; [1] collapsed rows;
 *     [2] duplicates; [3] rows that take no part; [4] n_cells; [5] cells with all three components kept by D5; [6] flags; [7] 1 when
 *     the grid is live.  [0] + [1] + [2] + [3] = n_rows.
 * D10 Fill trusts nothing.  The fill writes row t only when offsets[t] >= 0, offsets[t] + 1 <= capacity, offsets[t + 1] - offsets[t]
 *     == 1 and its three cell entries lie in 0 .. 3 n_rows - 1 and are pairwise different.  A row is written whole or not at all.
 *     Nothing outside out and src [0 .. capacity) is written and nothing is read out of bounds, whatever cell and offsets hold.
 *     Offsets that a count call left send every source row to an output row of its own; with other offsets several source rows may
 *     pass the tests for one output row, and that row then holds, word by word, the word of any of them.  Output rows that belong to
 *     no source row are not touched.  The caller sees an overflow in offsets[n_rows] > capacity and may call again with larger
 *     arrays; the count need not be repeated.  The duplicate decision is carried by offsets: a choice, not a safety matter.
 *
 * STATED LIMITS.  Clustering does not preserve manifoldness: two sheets that pass through one cell are joined there, and the output of
 * a closed mesh may have non-manifold and boundary edges.  Two representatives may round to one float value, and a representative
 * may round onto a face of its cell (its upper face then belongs to the next cell).  Such rows are emitted, not filtered.
 *
 * What follows from D1 .. D10.
 * - Nothing depends on how the work was split, on the arrival order of threads, on the order of probing or on what `work` held.
 * - A permutation of the rows leaves cell_point as a SET of points, the set of unordered cell triples that are emitted and, without
 *   DEDUP, the multiset of output position triples unchanged.
 * - Rotating a row's vertices rotates its output row; reversing its winding reverses it.
 * - Identity.  If no two distinct vertex values share a cell, the output positions are the input's on the bits (-0 becomes +0), and T
 *   is n_rows minus the rows with a repeated vertex or a non-finite coordinate (and minus the duplicates, under DEDUP).
 * - Idempotence.  Decimating the output again with the same grid returns it on the bits -- but for the rounding limit above.
 * - n_cells is at most the number of distinct vertex values, and T <= n_rows.
 * Held by the numpy restatement (tests/decimate_expected.py, tests/test_decimate_expected.py) on the shipped meshes; with the origin at
 * the mesh minimum minus 0.013 and h the largest extent / div: the sphere of 320 rows at div 4, 8, 16 gives 112, 294, 320 rows in 58,
 * 149, 162 cells (closed at 4 and 8, the identity at 16); the bunny of 4968 rows at div 8, 16 gives 403 and 1446 rows in 200 and 722
 * cells with 25 and 35 duplicates, not closed, and is the identity at div 4096.
 *
 * THE CALLS.
 * ezrt_decimate_work_bytes(n_rows) does no device work: the bytes of `work` a count call over n_rows rows needs -- a pure function,
 * monotone in n_rows, a multiple of 8, 8 for n_rows <= 0:
 *   40 n_rows + 8 ceil(3 n_rows / 2048) + 64 P(6 n_rows) + 4 P(2 n_rows) + 16
 * with P(x) the smallest power of two that is at least x and at least 8: per slot of the cell table (P(6 n_rows) slots, at most half
 * full) the 64-bit key, three int64 sums, the count, the lowest corner and two D5 words per axis; a word per corner for its slot and
 * an int64 for the numbering; the table of D7 and a word per row; the scan's tiles.  Between 430 and 830 bytes per row: the table is
 * sized for one cell per corner, whatever the grid.
 * ezrt_decimate_count_device writes cell, cell_corner, cell_point (D3 .. D5), offsets (D9) and summary.  work is scratch of at least
 * ezrt_decimate_work_bytes(n_rows) bytes, 8-byte aligned, whose contents before and after the call mean nothing; two calls in flight
 * at once need two.
 * ezrt_decimate_rows_device takes tri36 and n_rows as given to the count call and cell, cell_point and offsets as it left them, and
 * writes row offsets[t] of out and src for every kept row t (D8, D10).  src may be NULL.  `s` supplies the device and the error slot
 * only: n_rows need not be the scene's n_tri, and the output of one call is the input of the next.
 *
 * How it is computed.  INIT: the tables, whatever `work` held.  INSERT, the hot kernel: one lane per corner; three 21-bit indices
 * packed are the 64-bit key of an open-addressed table, claimed by atomicCAS, and the sums, the count, the lowest corner (atomicMin)
 * and per axis the least and greatest M1 key (atomicMin, atomicMax) are integer atomics on the slot.  A RUN of neighbouring lanes of
 * a wave with the same cell is reduced by a segmented scan of shuffles first, and its last lane probes once and issues one set of
 * atomics for the run: on a coarse grid most neighbouring corners share a cell.  FLAG and the weld's tiled prefix sum number the
 * cells by lowest corner; CELLS finishes D4 and D5, one lane per cell, and translates corners to cell numbers.  CLASSIFY (under
 * DEDUP): a survivor claims the slot of its sorted triple in a second table of row ids (atomicCAS, lowered by atomicMin; keys are
 * compared by reading the row's three cells).  KEEP writes the flags into offsets and the summary -- one int64 atomic per workgroup
 * and term -- and the prefix sum runs again, in place.  FILL: a workgroup owns a tile of 256 rows; a lane per row tests D10, gathers
 * its three points, computes N1 and leaves them in LDS with the row's destination; then the lanes are laid over the tile's 2304
 * float4s -- entry f belongs to row f / 9, part f % 9 -- each reading its 16 bytes of material where its part has any and storing 16
 * bytes, at consecutive addresses wherever kept rows follow one another.  That route needs tri36 and out 16-byte aligned; otherwise
 * every lane writes its own row float by float, to the same bits.  No floating-point atomics, no grid-wide barrier, no workgroup
 * waits for another; the probing loops are bounded by the tables' capacities and every other loop by a constant or a workgroup's
 * stride.
 * Measured on one MI355X (profiles/r36/decimate_rates.txt; device events, median of 7 repeats), beside the weld (1.72 ms) and the topology
 * (3.06 ms) of the same rows and, for the fill, beside a device-to-device copy of the bytes it reads plus writes.  A strip of 10^6
 * rows with shuffled ids and about 100 corners per cell: count 0.82 ms, 0.48 of the weld (in its natural order, where the runs are
 * long: 0.37 ms); the Bunny scene at 1 272 140 rows in 729 cells: 0.47 ms.  The same strip with ONE vertex per cell: count 2.18 ms,
 * 1.27 times the weld and 0.71 of the topology, of which the insert is 1.57 ms; fill 0.079 ms beside 0.048 ms for the copy, 1.67
 * times it, and 0.52 ms on the per-lane route, 6.5 times the staged one.  KNOWN LIMIT: with one vertex per cell no run is longer
 * than one lane and the insert is 3 * 10^6 probes and 33 * 10^6 integer atomics at random places of a 537 MB table; it is bound by
 * them, written down, not cured (a 64-byte record per slot made that case 1.97 ms and the coarse ones up to 1.5 times slower: the
 * atomics of a contended cell then queue on one line).  KNOWN LIMIT: `work` is sized for one cell per corner whatever the grid.
 *
 * Memory, streams, ordering and errors are those of ezrt_clip.h: every pointer is device memory of the scene's device, large enough
 * for its elements (anything else is rejected before any launch, never dereferenced); the work is enqueued on `stream` and the call
 * returns without synchronising or allocating; it may run beside ezrt_render_device and the other queries on other streams and
 * leaves ezrt_counters and ezrt_last_render_ms alone.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): any NULL pointer (the stream and src excepted; out may be NULL with
 * capacity == 0); n_rows < 0 or above INT32_MAX / 3; a bit of flags other than EZRT_DECIMATE_DEDUP; capacity < 0 or beyond what an
 * array can hold; work_bytes below ezrt_decimate_work_bytes(n_rows) or work not 8-byte aligned; out overlapping tri36; a pointer that
 * is not device memory of the scene's device.  n_rows == 0 returns 0 and launches nothing (the outputs are then not written either). */
#ifndef EZRT_DECIMATE_H
#define EZRT_DECIMATE_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_DECIMATE_DEDUP 1

/* the bytes of `work` for n_rows rows (pure, monotone, a multiple of 8; no device work; never fails) */
size_t ezrt_decimate_work_bytes(int n_rows);
int ezrt_decimate_count_device(EzrtScene* s, const float* tri36 /* n_rows x 36, the caller's rows */, int n_rows,
                               const float* grid4 /* ox oy oz h, device */, int flags, int32_t* cell /* 3 n_rows */,
                               int32_t* cell_corner /* 3 n_rows */, float* cell_point /* 3 n_rows x 3 */, int64_t* offsets /* n_rows + 1 */,
                               int64_t* summary /* 8 */, void* work, size_t work_bytes, void* stream);
int ezrt_decimate_rows_device(EzrtScene* s, const float* tri36 /* n_rows x 36 */, int n_rows, const int32_t* cell /* 3 n_rows */,
                              const float* cell_point /* 3 n_rows x 3 */, const int64_t* offsets /* n_rows + 1 */, int64_t capacity,
                              float* out /* capacity x 36 */, int32_t* src /* capacity, or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
