/* ezrt_vertices.h -- stream-ordered VERTEX WELD and SMOOTH NORMALS on device memory (libezrt_hip.so only): the indexed mesh of the
 * scene's triangles, the star of every vertex, its fans and flags, and the reference's smooth normals over the stars.
 *
 * ezrt_topology.h compares vertices by value on the bits, but the vertex itself is no object there.  The calls here make it one:
 * which corners are one vertex, which corners meet at it, whether the surface is pinched at it -- and, from that alone, the smooth
 * normals that the reference's readObj(..., smoothNormal = true) computes on the host, for rows that have been moved on the device and
 * are about to go into a refit (ezrt_refit.h reads floats 0-17 of a row: p1 p2 p3 n1 n2 n3).
 *
 * THE DEFINITION.  W1 to W7 are sets of integers: no floating-point arithmetic occurs, the only predicate is "is finite", on the bits.
 *
 * W1  Key, live.  The vertex key is M1 of ezrt_topology.h, and a triangle takes part when it is TOPO-live (M2 there): the same set as
 *     the topology's, so the two calls' counts combine.  Corner c = 3 t + k is stored vertex k of triangle t.  The corners of every
 *     other triangle have vertex[c] = -1 and are in no star.
 * W2  Vertices.  The distinct keys of live corners are numbered by the ascending LOWEST corner that carries them: vertex[c] in
 *     0 .. V - 1, and vert_corner[v] is that lowest corner.  So vert_corner is strictly ascending, vertex[vert_corner[v]] == v, and
 *     the position of v is read from any triangle array at corner vert_corner[v].
 * W3  Stars.  star[star_offsets[v] .. star_offsets[v + 1]) is the live corners with key v, ascending.  star_offsets[0] = 0 and
 *     star_offsets[V] = L, the number of live corners; the valence of v is the difference of two consecutive offsets.  All int32:
 *     3 n_tri <= INT32_MAX is the topology's limit already.
 * W4  Incident edges, from the star alone.  Corner c of v has two other keys a(c) (the next stored vertex of its triangle) and b(c)
 *     (the one after).  m(v, w) is the number of corners in the star of v that have w among their other keys.  It equals M4's
 *     multiplicity of the edge {v, w}: every triangle on that edge has a corner at v.
 * W5  Fans.  Two corners of one star are linked when their other keys share a value; take the closure.  fans[v] is the number of its
 *     classes: 1 at an ordinary interior or border vertex, 2 where two cones of triangles touch in the vertex only.
 * W6  Flags.  vert_flags[v] has bit 0 set when some m(v, w) == 1 (the vertex is on the border), bit 1 when some m(v, w) >= 3, bit 2
 *     when fans[v] > 1.  fans and vert_flags are the FLAGS GROUP: both, or both NULL, and then none of W4 to W6 is computed.
 * W7  Summary.  [0] L; [1] V; [2] the largest valence; [3] [4] [5] the vertices with bit 0, bit 1, bit 2 (0 when the flags group is
 *     NULL); [6] [7] 0.
 *
 * What follows from W1 .. W7.
 * - Nothing depends on the tree, on how the work was split, on the arrival order of threads, or on what `work` held.
 * - Reversing windings changes nothing except that a(c) and b(c) swap: no output of the call changes.
 * - A permutation of the triangle ids renumbers corners and vertices and keeps the partition of the corners by key, every valence,
 *   fans and flags of every key, and every count of W7.
 * - With T the summary of ezrt_mesh_topology_device on the same triangles, the Euler characteristic V - E + F is
 *   summary[1] - T[1] + T[0] (T[0] the live triangles, T[1] the undirected edges).
 * - A mesh is a CLOSED 2-MANIFOLD exactly when the topology says closed (T[2] == 0 && T[5] == 0) and summary[5] == 0: rule M6 does
 *   not connect triangles that meet only in a vertex, and bit 2 is what sees a surface pinched there.
 *
 * THE NORMALS.  fp32, the reference's operations in the reference's order, compiled without contraction.
 *
 * N1  Face normal.  Of triangle t of the CALLER's rows: normalize(cross(p2 - p1, p3 - p1)), the operations that the scene build and
 *     the refit share for the plane normal.
 * N2  Vertex sum.  S(v) = (((0, 0, 0) + fn(star[o] / 3)) + fn(star[o + 1] / 3)) + ..., componentwise fp32, over the star in ascending
 *     order from o = star_offsets[v], starting from +0.
 * N3  Corner normals.  A live corner gets normalize(S(vertex[c])), normalize(a) = a * (1.0f / sqrtf(dot(a, a))), into floats
 *     9 + 3 k .. 11 + 3 k of row t.  A corner with vertex[c] < 0 gets N1 of its own triangle, whatever that is.  There are no special
 *     cases: a live sliver whose cross product is 0 contributes NaN and poisons its vertices, as in the reference.
 * N4  Robustness.  The corner gets N1 whenever the weld arrays are not usable for it: vertex[c] outside -1 .. 3 n_tri - 1, an offsets
 *     pair outside 0 <= lo <= hi <= 3 n_tri, a star entry outside 0 .. 3 n_tri - 1.  Nothing out of bounds is read or written then.
 *
 * On an OBJ whose vertex lines are distinct by value, with the triangles in the file's order, N1 to N3 are readObj's smooth normals
 * on the bits (the star in ascending corner order is the order in which readObj adds the faces of a vertex).  They DIFFER from
 * readObj in two documented places: vertex lines that are equal by value are ONE vertex here (a cube stored with 24 vertex lines has
 * 8 vertices and rounded corners here, flat faces there), and a triangle with two equal vertices takes no part here and adds NaN to
 * its vertices there.
 *
 * THE CALLS.
 * ezrt_weld_work_bytes(n_tri) and ezrt_vertex_normals_work_bytes(n_tri) do no device work: the bytes of `work` a call on n_tri
 * triangles needs -- pure, monotone in n_tri, a multiple of 8, 8 for n_tri <= 0 (the weld: 144 to 168 B per triangle; the normals 12).
 * ezrt_mesh_weld_device reads the scene's triangles and writes
 *   vertex        (3 n_tri) W1, W2, for every corner;
 *   vert_corner   (3 n_tri) W2: entries 0 .. V - 1; entries at and beyond V are NOT TOUCHED;
 *   star_offsets  (3 n_tri + 1) W3: entries 0 .. V; entries beyond V are NOT TOUCHED;
 *   star          (3 n_tri) W3: entries 0 .. L - 1; entries at and beyond L are NOT TOUCHED;
 *   fans, vert_flags   (3 n_tri each, or both NULL) W5, W6: entries 0 .. V - 1; the others are NOT TOUCHED;
 *   summary       (8) W7.
 * `s` supplies the device, the error slot and the triangles.  work is scratch of at least ezrt_weld_work_bytes(n_tri) bytes, 8-byte
 * aligned, whose contents before and after the call mean nothing; two calls in flight at once need two.
 * ezrt_mesh_weld_at_device is the same rule for pairs already held, one lane per pair and no table: same[i] is 1 when corners
 * corner_a[i] and corner_b[i] carry one key, 0 when they do not, -1 when either is outside 0 .. 3 n_tri - 1 or belongs to a triangle
 * that is not live.
 * ezrt_vertex_normals_device reads the positions (floats 0-8) from the caller's tri36, the array about to go into a refit, NOT from
 * the scene, and writes floats 9-17 of every row and nothing else; `s` supplies the device and the error slot, and n_tri must be
 * the scene's.  vertex (3 n_tri), star_offsets (3 n_tri + 1) and star (3 n_tri) are a weld's arrays at their full size.  The weld is
 * taken BY VALUE: one made once serves every frame of a deformation that moves vertices and keeps which corners coincide; after a
 * deformation that tears or merges vertices it has to be made again (after the refit, from the scene).
 *
 * How it is computed.  JOIN: one lane per corner inserts into an open-addressed table of the next power of two of at least 6 n_tri
 * slots (at most half full); a slot is claimed by atomicCAS with a representative corner, keys are compared by reading the
 * representative's coordinates, which nobody writes, and an atomicMin on the claimed slot leaves the key's lowest corner.  IDS: a flag
 * at every lowest corner and a prefix sum (tiles of 2048 entries over many workgroups).  STARS: a count per vertex, the prefix sum
 * again, a scatter in arrival order into `work`, and a
 * rank launch in which every corner counts the lower corners of its star -- its rank is its position, so the star is ascending
 * whatever the arrival order.  FLAGS: one lane per corner walks its star for m of its two edges and unites itself, in a lock-free
 * union-find over corners kept in `work` (parent[c] <= c, the higher root hooked under the lower by atomicCAS), with every lower
 * corner that shares an edge; a root counts a fan.  NORMALS: the face normals go through `work`, then every corner sums its star in
 * order; no floating-point atomics.  Words shared between workgroups inside a launch are touched by device-scope atomics only;
 * everything else crosses a launch boundary.  Every loop is bounded: probes by the table's size, walks of a star by 3 n_tri, finds by
 * the strictly descending parent.  KNOWN LIMIT: a vertex of valence k costs O(k^2) steps -- k steps in each of the k lanes of its
 * own corners, in the rank and again in the flags (and k steps per corner in the normals), with k additions on one counter and the
 * star's unions on one chain of parents.  A mesh valence is about 6; the apex of a fan of 100 000 triangles is slow.
 *
 * Memory, streams, ordering and errors are those of ezrt_topology.h: every pointer is device memory of the scene's device, large
 * enough for its elements (anything else is rejected before any launch, never dereferenced); the work is enqueued on `stream` and
 * the call returns without synchronising or allocating; it may run beside ezrt_render_device and the other queries on other streams
 * and leaves ezrt_counters and ezrt_last_render_ms alone; a later refit waits for it.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, vertex, vert_corner, star_offsets, star, summary, tri36 or
 * work; a half-NULL flags group; work_bytes below the call's *_work_bytes(n_tri) or work not 8-byte aligned; a scene of more than
 * INT32_MAX / 3 triangles; n_tri that is not the scene's; a pointer that is not device memory of the scene's device; for the _at call
 * NULL scene, corner_a, corner_b or same, or n < 0.  A scene without triangles, and n == 0, return 0 and launch nothing. */
#ifndef EZRT_VERTICES_H
#define EZRT_VERTICES_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_VERTEX_BORDER 1
#define EZRT_VERTEX_NONMANIFOLD_EDGE 2
#define EZRT_VERTEX_PINCHED 4

/* the bytes of `work` for n_tri triangles (pure, monotone, a multiple of 8; no device work; never fails) */
size_t ezrt_weld_work_bytes(int n_tri);
int ezrt_mesh_weld_device(EzrtScene* s, int32_t* vertex /* 3 * n_tri */, int32_t* vert_corner /* 3 * n_tri: entries >= V are not touched */,
                          int32_t* star_offsets /* 3 * n_tri + 1: entries > V are not touched */,
                          int32_t* star /* 3 * n_tri: entries >= L are not touched */, int32_t* fans /* 3 * n_tri, or NULL with the next */,
                          uint8_t* vert_flags /* 3 * n_tri */, int64_t* summary /* 8 */, void* work, size_t work_bytes, void* stream);
int ezrt_mesh_weld_at_device(EzrtScene* s, const int32_t* corner_a, const int32_t* corner_b, int n,
                             int8_t* same /* n: 1 one vertex, 0 two, -1 no live corner */, void* stream);
size_t ezrt_vertex_normals_work_bytes(int n_tri);
int ezrt_vertex_normals_device(EzrtScene* s, float* tri36 /* n_tri x 36: floats 9-17 of every row are written, nothing else */, int n_tri,
                               const int32_t* vertex /* 3 * n_tri */, const int32_t* star_offsets /* 3 * n_tri + 1 */,
                               const int32_t* star /* 3 * n_tri */, void* work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
