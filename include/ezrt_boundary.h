/* ezrt_boundary.h -- stream-ordered BOUNDARY LOOPS on device memory (libezrt_hip.so only): the holes of a mesh as ordered cycles of
 * half-edges, how large each is, and the triangles that close them.
 *
 * ezrt_topology.h says that a mesh is open (summary[2] BOUNDARY edges), ezrt_orient.h that a patch is (EZRT_PATCH_OPEN), ezrt_vertices.h
 * which vertices lie on a border (EZRT_VERTEX_BORDER).  None of them says that the 42 BOUNDARY edges of the packaged Bunny are four
 * holes of 11, 12, 11 and 8 edges, in which order the edges run, how large each hole is, or which triangles close it -- and until they
 * are closed ezrt_inside.h is not valid on the mesh, the signed volume of ezrt_orient.h decides nothing and ezrt_plane_loops.h returns
 * open paths.  The repair chain: topology, orient, rewind, refit, topology, BOUNDARY (ezrt_mesh_boundary_device), CAP
 * (ezrt_cap_rows_device), then a new scene of the rows and the cap, closed, on which every query is valid.  A FLIPPED edge ends a
 * chain here: orient and rewind first.
 *
 * THE DEFINITION.  Every output of the loops call is an integer.  The only floating-point arithmetic is the fp64 cross product of B7;
 * it is pinned operation by operation and followed by an integer sum.
 *
 * B1  Inputs by value.  The call reads twin and edge_class (3 n_tri each), normally those of ezrt_mesh_topology_device on the same
 *     scene, and the scene's stored positions.  It builds no table of its own.  A triangle TAKES PART as in O1 of ezrt_orient.h: its
 *     three edge_class entries are all in 1 .. 4.  Half-edge h = 3 t + e runs from stored vertex e to stored vertex (e + 1) % 3 of
 *     triangle t; its index is also the corner index of ezrt_vertices.h of its start vertex, so vertex[h] of a weld names it.  h is a
 *     BOUNDARY half-edge when its triangle takes part and edge_class[h] == 1.
 * B2  Successor, by rotation about the end vertex.  For a BOUNDARY half-edge h start with c = 3 t + (e + 1) % 3, the half-edge of t
 *     that leaves the end vertex of h, and repeat: if edge_class[c] == 1, next[h] = c, stop.  If edge_class[c] != 2, next[h] = -1,
 *     stop.  Otherwise let g = twin[c]; the step is valid when 0 <= g < 3 n_tri, g / 3 != c / 3, triangle g / 3 takes part,
 *     edge_class[g] == 2 and twin[g] == c.  If it is not valid, next[h] = -1, stop.  If it is, c = 3 (g / 3) + (g % 3 + 1) % 3, the
 *     half-edge of the neighbour that leaves the same vertex, and repeat.  FLIPPED and NONMANIFOLD edges end the walk: no direction is
 *     implied across them.  The walk never leaves the fan of triangles it started in: at a pinched vertex each fan keeps its own
 *     boundary.  A half-edge that is not BOUNDARY has next = -1.  The step map is injective (twin[g] == c is tested) and the start
 *     has no predecessor under it (the half-edge before it in its triangle is h, of class 1), so the walk visits no half-edge twice
 *     whatever the arrays hold; it is bounded by 3 n_tri steps all the same (next[h] = -1 beyond them).
 *     Nothing out of bounds is read.  It follows that every BOUNDARY half-edge has at most one successor and at most one predecessor.
 * B3  Chains.  The components of next over BOUNDARY half-edges are therefore cycles and open paths.  The HEAD of a cycle is its lowest
 *     half-edge; the head of a path is its member without a predecessor.  pos[h] is the number of next steps from the head to h.
 * B4  Numbering and output.  Loops -- cycles and paths alike -- are numbered by ascending head, 0 .. L - 1.  loop[h] and pos[h] are
 *     written for every half-edge, -1 where h is not BOUNDARY.  order[loop_offsets[l] + p] is the half-edge at position p of loop l;
 *     loop_offsets[0] = 0 and loop_offsets[L] = B, the number of BOUNDARY half-edges (with L = 0 that is the one entry 0).
 * B5  Flags.  lflags[l] bit 0 is CLOSED (EZRT_LOOP_CLOSED): the loop is a cycle.  The other bits are 0.
 * B6  Scale.  A and E are as in O6 of ezrt_orient.h: A is the largest finite |coordinate| of the triangles that take part, compared
 *     on the bits, and E the frexp exponent of (double)A, 0 when A == 0.  S2 = 2 E - 30.
 * B7  Area vector.  This is the AREA GROUP: area2 is either a pointer or NULL, and if NULL nothing of B6 and B7 is computed and
 *     summary[5] is 0.  For a BOUNDARY half-edge with start a and end b (stored positions, converted to double) compute, with every
 *     operation rounded to fp64 as written and no contraction,
 *       c = (a.y * b.z - a.z * b.y,  a.z * b.x - a.x * b.z,  a.x * b.y - a.y * b.x).
 *     r_k = llrint(ldexp(c_k, -S2)), round to nearest even, and 0 when c_k is not finite.  area2[3 l + k] is the int64 sum of r_k over
 *     loop l.  |r_k| <= 2^31 and there are fewer than 2^32 half-edges, so no sum overflows and the order of summation does not
 *     matter.  Half of area2 * 2^S2 is the vector area of any surface that spans a closed loop (the sum of a x b round a closed
 *     polygon does not depend on the origin); it is exact whenever every c_k is a multiple of 2^S2 (small integer coordinates).
 * B8  Summary (int64[8]).  [0] B; [1] L; [2] closed loops; [3] the length of the longest loop; [4] BOUNDARY half-edges with
 *     next == -1; [5] S2 (0 without the area group); [6] and [7] 0.
 *
 * What follows from B1 .. B8.
 * - Nothing depends on the tree, on how the work was split, on the arrival order of threads, or on what `work` held.
 * - On a topology's own arrays B equals the topology's summary[2].
 * - On a mesh whose every edge is BOUNDARY or MANIFOLD, EVERY LOOP IS CLOSED and summary[4] is 0: the rotation about a vertex can
 *   only end at a BOUNDARY half-edge.
 * - The surface lies to the LEFT of a boundary half-edge seen from the side its normals point to: a hole is run through clockwise
 *   seen from there, the outer rim of a disc counter-clockwise.
 * - Reversing every stored winding reverses every loop as a cyclic sequence of undirected edges and negates every area2.
 * - A permutation of the triangle ids keeps the set of cyclic edge sequences and the multiset of area2.
 * - On a consistently wound mesh with every loop closed, the sum of area2 over all loops equals the sum over the triangles of
 *   (p2 - p1) x (p3 - p1), exactly whenever both sides are multiples of 2^S2.  This is Stokes: interior edges cancel.
 *
 * THE CAP.  ezrt_cap_rows_device takes the loops arrays by value and reads positions and materials from the CALLER's tri36, the rows
 * about to go into a scene, not from the scene.
 * C1  Valid rows.  Row j belongs to half-edge h = order[j], loop l = loop[h], position p = pos[h], length
 *     k = loop_offsets[l + 1] - loop_offsets[l].  The row is VALID when j < B, the loop is CLOSED, k >= 3, 1 <= p <= k - 2, every
 *     index read on the way is in range (0 <= h < 3 n_tri, 0 <= l < L, 0 <= loop_offsets[l] < B, the head's entry of order in
 *     0 .. 3 n_tri - 1) and loop_offsets[l] + p == j.  B and L are read from summary[0] and summary[1] on the device and clamped to
 *     [0, 3 n_tri].
 * C2  Triangle.  A valid row is the triangle (H, end(h), start(h)), H the start vertex of the loop's head order[loop_offsets[l]];
 *     positions are copied on the bits.  This is a fan from the head's start vertex, and it crosses every boundary edge against its
 *     direction: on truthful arrays the capped mesh has no BOUNDARY and no FLIPPED edge on that loop.  A loop of k edges gets k - 2
 *     triangles.
 * C3  Normals and materials.  Floats 9-17 are N1 of ezrt_vertices.h of the new triangle, three times (the same device function).
 *     Floats 18-35 are those of row h / 3 on the bits: the material of the triangle the cap closes against.
 * C4  Invalid rows and limit.  An invalid row with j < B is 36 times +0.0f and has cap_valid[j] = 0; a valid one has cap_valid[j] = 1.
 *     Rows at and beyond B are NOT TOUCHED.  KNOWN LIMIT: a fan closes a hole topologically; a non-planar or non-convex hole gets a
 *     folded cap, and a fan edge between two vertices of the loop that the mesh already joins by an edge (the diagonal of a corner
 *     cell of a grid, a hole pinched at the head's vertex) becomes an edge of four triangles, NONMANIFOLD in the next topology.
 *
 * THE CALLS.
 * ezrt_boundary_work_bytes(n_tri) does no device work: the bytes of `work` a loops call on a scene of n_tri triangles needs -- a pure
 * function, monotone in n_tri, a multiple of 8, 8 for n_tri <= 0:
 *   132 n_tri + 4 (n_tri mod 2) + 8 ceil(3 n_tri / 2048) + 56
 * (per half-edge two int64 of the prefix sums, two int64 of the ranking's double buffer and three ints -- predecessor, union-find,
 * compacted list: 44 bytes, 132 per triangle; padding to 8; an int64 per scan tile of 2048 half-edges; 56 bytes for the ends of the
 * sums and the counts).
 * ezrt_mesh_boundary_device reads twin, edge_class and the scene's triangles and writes
 *   next, loop, pos     (3 n_tri each) B2, B4, for every half-edge;
 *   order               (3 n_tri) B4: entries 0 .. B - 1; entries at and beyond B are NOT TOUCHED;
 *   loop_offsets        (3 n_tri + 1) B4: entries 0 .. L; entries beyond L are NOT TOUCHED;
 *   lflags              (3 n_tri) B5: entries 0 .. L - 1; entries at and beyond L are NOT TOUCHED;
 *   area2               (9 n_tri, or NULL) B7: entries 0 .. 3 L - 1; entries at and beyond 3 L are NOT TOUCHED;
 *   summary             (8) B8.
 * `s` supplies the device, the error slot and the positions.  work is scratch of at least ezrt_boundary_work_bytes(n_tri) bytes,
 * 8-byte aligned, whose contents before and after the call mean nothing; two calls in flight at once need two.  The topology is taken
 * BY VALUE: after a refit that changes the mesh it has to be made again, and so has this call.
 * ezrt_cap_rows_device reads the CALLER's rows and the loops arrays and writes cap (3 n_tri rows of 36 floats) and cap_valid
 * (3 n_tri): rows 0 .. B - 1, C1 to C4.  `s` supplies the device and the error slot, and n_tri must be the scene's.  The valid rows,
 * appended to the caller's rows, are the closed mesh; a new scene takes them.
 *
 * How it is computed.  Seventeen launches and the rounds of the ranking.  INIT.  NEXT: one lane per half-edge walks B2 and writes next
 * and, into `work`, the predecessor (one writer, by B2).  UNION: the lock-free union-find of the topology and the orientation
 * (parent <= h, the higher root hooked under the lower by atomicCAS, paths halved by atomicCAS) over half-edges, uniting h with
 * next[h]: the root is the chain's lowest member, for a cycle its head.  OPEN: the one member of a path without a successor marks its
 * root; a cycle is cut before its root.  COMPACT: a flag at each BOUNDARY half-edge and the vertex weld's tiled prefix sum (three
 * launches), so that the rounds that follow run over B entries and their lanes beyond B leave at once.  RANK: pointer jumping along
 * the predecessor, (ancestor, steps) -> (the ancestor's ancestor, the sum), in ceil(log2(3 n_tri)) rounds fixed by the host -- at most
 * 32, one launch each, from one buffer of `work` into the other; each member ends with (head, pos).  NUMBER: a flag at each head, the
 * prefix sum again over the compacted list, which is in ascending order; the last member of each chain writes its length and flag;
 * the prefix sum of the lengths; a scatter of order and loop_offsets.  AREA, in the scatter's launch: r_k summed over runs of
 * neighbouring lanes with one loop by a segmented wave scan, then one int64 atomicAdd per run and component.  Rounds are separated by
 * launch boundaries: there is no cooperative launch, no grid-wide barrier and no workgroup waits for another.  Words shared between
 * workgroups inside a launch are touched by device-scope atomics only.  Every loop is bounded: the walk by 3 n_tri steps, finds by the
 * strictly descending parent, unions by 3 n_tri retries.  No floating-point atomics; the fp64 cross product is compiled without
 * contraction.
 * KNOWN LIMIT: a border vertex of valence k costs its incoming boundary half-edge k serial steps in NEXT (a fan of 10^5 triangles
 * round one border vertex is walked by one lane), and a loop of length n costs log2 n rounds of gathers over its members; the rounds
 * are launched whatever B is, so a mesh without a boundary still pays ceil(log2(3 n_tri)) empty launches, a few microseconds each.
 * Measured on one MI355X (profiles/r33/boundary_rates.txt): the Bunny at 1.27 M triangles with 672 boundary half-edges takes 0.24 ms a
 * call beside 3.18 ms for the topology that feeds it, 0.11 ms of it in 22 rounds that move 672 entries; a strip of 10^6 triangles, one
 * loop of 1 000 002, takes 0.66 against 3.06 ms (the rounds 0.29); 333 333 islands 0.37 against 0.87 ms.  No mesh measured costs more
 * than its topology.  The cap writes 144 B per row from one lane: 0.56 ms for the strip's 10^6 rows.
 *
 * Memory, streams, ordering and errors are those of ezrt_orient.h: every pointer is device memory of the scene's device, large enough
 * for its elements (anything else is rejected before any launch, never dereferenced); the work is enqueued on `stream` and the call
 * returns without synchronising or allocating; it may run beside ezrt_render_device and the other queries on other streams and leaves
 * ezrt_counters and ezrt_last_render_ms alone; a later refit waits for it.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): any NULL pointer (the stream and area2 excepted); work_bytes below
 * ezrt_boundary_work_bytes(n_tri) or work not 8-byte aligned; a scene of more than INT32_MAX / 3 triangles; n_tri that is not the
 * scene's; a pointer that is not device memory of the scene's device.  A scene without triangles returns 0 and launches nothing. */
#ifndef EZRT_BOUNDARY_H
#define EZRT_BOUNDARY_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_LOOP_CLOSED 1

/* the bytes of `work` for a scene of n_tri triangles (pure, monotone, a multiple of 8; no device work; never fails) */
size_t ezrt_boundary_work_bytes(int n_tri);
int ezrt_mesh_boundary_device(EzrtScene* s, const int32_t* twin /* 3 * n_tri */, const uint8_t* edge_class /* 3 * n_tri */,
                              int32_t* next /* 3 * n_tri */, int32_t* loop /* 3 * n_tri */, int32_t* pos /* 3 * n_tri */,
                              int32_t* order /* 3 * n_tri: entries >= B are not touched */,
                              int32_t* loop_offsets /* 3 * n_tri + 1: entries > L are not touched */,
                              uint8_t* lflags /* 3 * n_tri: entries >= L are not touched */,
                              int64_t* area2 /* 9 * n_tri, or NULL: entries >= 3 L are not touched */, int64_t* summary /* 8 */, void* work,
                              size_t work_bytes, void* stream);
int ezrt_cap_rows_device(EzrtScene* s, const float* tri36 /* n_tri x 36, the caller's rows */, int n_tri, const int32_t* order,
                         const int32_t* loop, const int32_t* pos, const int32_t* loop_offsets, const uint8_t* lflags,
                         const int64_t* summary, float* cap /* 3 * n_tri x 36: rows >= B are not touched */,
                         uint8_t* cap_valid /* 3 * n_tri: likewise */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
