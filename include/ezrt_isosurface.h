/* ezrt_isosurface.h -- stream-ordered ISOSURFACE EXTRACTION on device memory (libezrt_hip.so only): a grid of values as triangle rows.
 *
 * ezrt_inside.h, ezrt_winding.h and ezrt_closest_point.h answer questions about a mesh at points of the caller's choosing; ezrt_clip.h,
 * ezrt_subdivide.h, ezrt_decimate.h, ezrt_vertices.h and ezrt_orient.h take triangle rows and give triangle rows.  This call leads from
 * the first group to the second: a field sampled on a regular grid -- the signed distance of a part, the winding number of a scan
 * with holes, the min or max of two fields -- becomes the rows of the surface where the field crosses a level.  The offset surface of
 * a part, a watertight remesh (the winding number at level 0.5), the union or intersection of two parts and a morph between two are
 * then two calls away.  It is the library's first call that MAKES a mesh, in the format every other mesh call takes, and the third
 * that writes triangle rows as a variable-length answer, in the count / offsets / fill pattern of ezrt_clip.h.
 *
 * The method is MARCHING TETRAHEDRA on the Kuhn split of every grid cell: no table of 256 cases, no ambiguous faces, and away from the
 * grid's border a closed, consistently wound 2-manifold from the signs of the values alone.
 *
 * THE DEFINITION.  Every operation is rounded once; no contraction anywhere.
 *
 * G1  Inputs by value.  values is nz x ny x nx floats in device memory, x fastest: vertex (i, j, k) is element (k ny + j) nx + i.
 *     grid8 is 8 floats in device memory: the origin ox oy oz, the spacing hx hy hz, the level iso, and one float of padding that is
 *     not read.  material18 is 18 floats in device memory: floats 18-35 of every output row.  `s` supplies the device and the error
 *     slot only.  The grid is LIVE when all seven numbers are finite and the three spacings are > 0.  A grid that is not live emits
 *     nothing: T = 0 and summary[6] = 0.
 * G2  Positions.  Coordinate a of vertex index i is (float)((double)o_a + (double)i * (double)h_a).
 * G3  Inside.  A vertex is INSIDE when f < iso and OUTSIDE when f >= iso: half-open, like the side rule of ezrt_clip.h; a value
 *     exactly at the level is outside (-0 against a level of +0 is outside), and a NaN level puts every vertex outside.  The
 *     convention is that of the signed distance: negative is inside.  A cell is the cube between vertices (i, j, k) and
 *     (i + 1, j + 1, k + 1), i < nx - 1, j < ny - 1, k < nz - 1; its index is (k (ny - 1) + j) (nx - 1) + i.  A cell with a non-finite
 *     value among its eight takes no part: it emits nothing and is counted in summary[3].  The surface has a hole there.
 * G4  Tetrahedra.  A cell is split into six tets, one per permutation pi of the axes (x, y, z), in lexicographic order of pi: xyz, xzy,
 *     yxz, yzx, zxy, zyx.  The vertices of a tet are T0 = the cell's low corner, T1 = T0 + e_pi(0), T2 = T1 + e_pi(1), T3 = the high
 *     corner.  The local order T0 < T1 < T2 < T3 is also the order of the vertex indices of G1.  This split has the same diagonals on
 *     both sides of every cell face, so neighbouring cells agree.
 * G5  Pieces per tet, from the four sides alone.  q(a, b) is G6's point on the tet edge between local vertices a < b.
 *     - no vertex or all four INSIDE: nothing;
 *     - one INSIDE vertex i, the others j0 < j1 < j2: one piece (q(i,j0), q(i,j1), q(i,j2));
 *     - one OUTSIDE vertex o, the others j0 < j1 < j2: one piece (q(o,j0), q(o,j1), q(o,j2));
 *     - two INSIDE a < b and two OUTSIDE c < d: two pieces, (q(a,c), q(a,d), q(b,d)) then (q(a,c), q(b,d), q(b,c)).
 *     A piece is emitted as written, or with its second and third vertex exchanged: the winding is the one whose normal faces the
 *     OUTSIDE vertices.  Which of the two it is comes from a table of 6 x 14 bits indexed by (pi, the 4-bit mask of INSIDE vertices, T0
 *     the low bit), never from arithmetic on values: for the even permutations xyz, yzx, zxy the exchanged masks are 2, 5, 8, 10, 11,
 *     14; for the odd permutations xzy, yxz, zyx they are the other eight, 1, 3, 4, 6, 7, 9, 12, 13.  The count of a cell is 0 .. 12
 *     and never depends on G6.
 * G6  Points.  On the edge between A = T_a and B = T_b, a < b:
 *       t = ((double)iso - (double)fA) / ((double)fB - (double)fA)
 *     and per component (float)(pA + t * (pB - pA)), in double on the double values of G2 before their rounding to float.  The point
 *     is a function of the edge's two vertices and the level alone: up to six tets of up to four cells share an edge, and all compute
 *     the same bits.
 * G7  Output row.  Floats 0-8 are the piece.  Floats 9-17 are three times the face normal of the OUTPUT positions, N1 of
 *     ezrt_vertices.h by the device function the decimation calls; a degenerate row gets NaN, as there.  Floats 18-35 are material18
 *     on the bits.  cell[r] is the cell index of output row r; cell may be NULL.  Smooth normals come afterwards from
 *     ezrt_mesh_weld_device and ezrt_vertex_normals_device.
 * G8  Order, offsets, summary.  Rows are in ascending cell, then tet order, then piece order.  A BLOCK is EZRT_ISO_BLOCK = 256
 *     consecutive cells; offsets is int64 with n_blocks + 1 entries, n_blocks = ceil(n_cells / 256): the exclusive prefix sum of the
 *     blocks' counts, T in offsets[n_blocks].  Offsets are per block, not per cell, on purpose: a 256^3 grid then needs 0.5 MB of
 *     offsets instead of 133 MB, and the fill rebuilds the order inside a block by itself.  summary (int64[8]): [0] T; [1] cells
 *     that emit; [2] cells with finite values that emit nothing; [3] cells with a non-finite value; [4] blocks that emit; [5]
 *     n_cells; [6] 1 when the grid is live, else 0; [7] 0.  [1] + [2] + [3] = n_cells.
 * G9  Fill trusts nothing.  K8 of ezrt_clip.h with a block in the place of a source row: the fill recomputes the block's count c
 *     and writes the block's rows only when offsets[b] >= 0, offsets[b] + c <= capacity and offsets[b + 1] - offsets[b] == c.  A
 *     block is written whole or not at all.  Nothing outside out, cell [0 .. capacity) is written whatever offsets holds.  A block
 *     whose two offsets are equal may therefore be left without reading a value, which makes the cost of the fill follow the
 *     surface, not the volume.  The caller sees an overflow in offsets[n_blocks] > capacity and may call again with larger arrays.
 *
 * STATED LIMITS, emitted and not filtered.
 * - A value at the level, or a t that rounds to 0 or 1, puts a point on a grid vertex.  Several edges then share it by value and a
 *   row may have two equal vertices.  The topology ignores such rows (the M-rules of ezrt_topology.h); the rest stays closed.
 * - The surface is open where it meets the border of the grid.  A caller who wants it closed pads the field with one layer of
 *   outside values.
 * - A position that overflows is emitted as it is.
 *
 * What follows from G1 .. G9.
 * - Nothing depends on how the work was split, on the route of the fill, on the arrival order of threads or on what `work` held.
 * - Away from the border of the grid and from non-finite values, the rows are a closed 2-manifold by value: every edge is in exactly
 *   two rows, once each way, and the normals face the OUTSIDE, so the signed volume of a bounded inside is positive.  Held by the
 *   numpy restatement (tests/test_iso_expected.py): on 17^3 grids a sphere with an off-lattice centre, 3164 rows, V - E + F = 2, no
 *   degenerate row; a torus, 3584 rows, V - E + F = 0; Gaussian noise padded with one layer of outside values, 27636 rows, every
 *   edge in exactly two rows, once each way (V - E + F = -654); on a 19^3 grid an integer field with 258 grid values exactly at the
 *   level, 3384 rows of which 1536 are not degenerate, and those are still closed with V - E + F = 2.
 * - Every position of a row lies in the closed box of its cell.
 * - Adding a constant to values and iso alike, where exact, changes nothing.
 *
 * THE CALLS.
 * ezrt_iso_work_bytes(nx, ny, nz) does no device work: the bytes of `work` a count call needs -- a pure function, monotone in each
 * dimension, a multiple of 8:
 *   8 ceil(n_blocks / 2048) + 8
 * (an int64 per scan tile of 2048 blocks, and one for their total); 8 for no cells.
 * ezrt_iso_count_device writes offsets and summary (G8).  work is scratch of at least ezrt_iso_work_bytes(nx, ny, nz) bytes, 8-byte
 * aligned, whose contents before and after the call mean nothing; two calls in flight at once need two.
 * ezrt_iso_rows_device takes values, the dimensions and grid8 as given to the count call and offsets as it left them, and writes
 * rows offsets[b] .. offsets[b + 1] of out and cell for every block b (G5 .. G9).  cell may be NULL.
 *
 * How it is computed.  COUNT: a memset of the summary, then a workgroup of 256 lanes owns a block, one lane per cell: eight loads (a
 * wave reads runs of consecutive floats from four grid rows, because cells are consecutive in x), the eight sides as a byte, a tet's
 * count from the popcount of its four bits; the block's sum as int64 into offsets[b]; the summary's terms are reduced over the wave
 * and added with one int64 atomic per wave and term.  SCAN: the tiled prefix sum of ezrt_vertices.h in place.  FILL: a workgroup per
 * block, which leaves at once when the block's two offsets are equal.  Otherwise it recomputes the counts, takes an exclusive scan
 * over the 256 lanes in LDS, and every lane builds its pieces: points by G6, the normal by N1.  A block can hold up to 3072 rows
 * (432 KiB), so the rows are staged in LDS in at most 12 rounds of 256 rows (36 KiB) and each round is written with the lanes laid
 * over its float4s, 16 B per lane at consecutive addresses.  That route needs out 16-byte aligned; otherwise every lane writes its
 * own rows float by float, to the same bits.  No floating-point atomics, no grid-wide barrier, no workgroup waits for another, and no
 * loop that is not bounded by a constant.
 * Measured on one MI355X (profiles/r39/iso_rates.txt): a sphere on a 128^3 grid (198 156 rows in 2890 of 8002 blocks), count 0.68 ms,
 * fill 0.11 ms; on a 256^3 grid (798 556 rows) count 4.48 ms, fill 0.50 ms; dense noise on a 128^3 grid (15.4 * 10^6 rows, 2.2 GB),
 * count 1.03 ms, fill 1.57 ms beside 0.40 ms for a device-to-device copy of the bytes the fill must read plus write, and 3.5 ms on the
 * per-lane route.  The offset surface of a mesh of 4968 triangles on a 128^3 grid: 4.9 ms, of which signed_distance 3.7 ms and this
 * call 1.0 ms.  KNOWN LIMITS, written down, not cured.  The count is bound by its atomics, not by its loads: its copy takes 0.004 ms
 * at 128^3, and up to four int64 atomics per wave of 32 012 waves land on four words of one cache line.  The dense fill is 3.9 times
 * its copy: every lane builds up to twelve rows one after another, with a double division per point, while the lanes of its block
 * wait at the round's barrier.  The sparse fill is 20 times its copy, which moves only 37 MB: a block that emits builds its rows with
 * the few lanes whose cells the surface crosses, and there the per-lane route is as fast as the staged one (0.41 against 0.50 ms at
 * 256^3).
 *
 * Memory, streams, ordering and errors are those of ezrt_boundary.h: every pointer is device memory of the scene's device, large
 * enough for its elements (anything else is rejected before any launch, never dereferenced); the work is enqueued on `stream` and the
 * call returns without synchronising or allocating; it may run beside ezrt_render_device and the other queries on other streams and
 * leaves ezrt_counters and ezrt_last_render_ms alone.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): any NULL pointer (the stream and cell excepted; out may be NULL with
 * capacity == 0); a dimension < 1; nx ny nz above INT32_MAX; capacity < 0 or beyond what an array can hold; work_bytes below
 * ezrt_iso_work_bytes(nx, ny, nz) or work not 8-byte aligned; out overlapping values; a pointer that is not device memory of the
 * scene's device.  A grid with a dimension of 1 has no cells: it returns 0 and launches nothing (offsets and summary are then not
 * written either). */
#ifndef EZRT_ISOSURFACE_H
#define EZRT_ISOSURFACE_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_ISO_BLOCK 256 /* cells per entry of offsets */

/* the bytes of `work` for an nx x ny x nz grid (pure, monotone, a multiple of 8; no device work; never fails) */
size_t ezrt_iso_work_bytes(int nx, int ny, int nz);
int ezrt_iso_count_device(EzrtScene* s, const float* values /* nz x ny x nx */, int nx, int ny, int nz, const float* grid8 /* 8 */,
                          int64_t* offsets /* n_blocks + 1 */, int64_t* summary /* 8 */, void* work, size_t work_bytes, void* stream);
int ezrt_iso_rows_device(EzrtScene* s, const float* values /* nz x ny x nx */, int nx, int ny, int nz, const float* grid8 /* 8 */,
                         const float* material18 /* 18 */, const int64_t* offsets /* n_blocks + 1 */, int64_t capacity,
                         float* out /* capacity x 36 */, int32_t* cell /* capacity, or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
