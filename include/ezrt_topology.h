/* ezrt_topology.h -- stream-ordered mesh TOPOLOGY on device memory (libezrt_hip.so only): edge twins, edge classes and components.
 *
 * Every geometric query of this library treats the scene as a triangle soup, and several state an assumption about that soup:
 * ezrt_inside.h is right on a closed mesh, ezrt_plane_loops.h returns closed loops on a closed, consistently wound manifold,
 * ezrt_winding.h is negated by a flipped winding.  The call here answers, for the scene's triangles as they are stored: is this mesh
 * closed?  Is it consistently wound?  How many parts is it?  Which triangle lies across this edge?
 *
 * THE DEFINITION.  Every answer is a set of integers.  No floating-point arithmetic occurs; the only floating-point predicate is "is
 * finite", and it is taken from the bits.
 *
 * M1  Vertex key.  The three coordinates as uint32 bit patterns, with a -0 replaced by +0.  Two vertices are equal when their keys
 *     are.  For finite values that is the library's == on all three coordinates ("-0 == +0", ezrt_self_overlap.h).
 * M2  TOPO-live.  A triangle takes part when its nine coordinates are finite and its three keys are pairwise distinct.  This is
 *     deliberately WIDER than the LIVE of ezrt_tri_overlap.h: a collinear sliver with three distinct vertices has three edges and does
 *     take part here, while it is not LIVE there.  Every other triangle has twin = -1, edge_class = 0, mult = 0 and root = component
 *     = -1 on its entries, and is invisible to everyone else.
 * M3  Half-edges and edges.  Half-edge h = 3 t + e, e = 0, 1, 2, runs from stored vertex e to stored vertex (e + 1) % 3 of triangle
 *     t.  Its undirected edge E(h) is the unordered pair of its two keys.  H(E) is the half-edges of TOPO-live triangles on E, in
 *     ascending h, and m = |H(E)|.  Two half-edges of one edge run either the SAME way or OPPOSITE ways (compare the keys of their
 *     start vertices).
 * M4  Class, the same for every half-edge of E:
 *       1 BOUNDARY     m == 1
 *       2 MANIFOLD     m == 2, opposite
 *       3 FLIPPED      m == 2, the same way: the two neighbours are wound inconsistently
 *       4 NONMANIFOLD  m >= 3
 *     mult[h] = m.
 * M5  Twin.  Split H(E) by direction into F and B, each ascending; which of the two is called F does not matter.  For
 *     j < min(|F|, |B|): twin[F[j]] = B[j] and twin[B[j]] = F[j].  The U left over (all of one direction, ascending) pair among
 *     themselves: U[0] with U[1], U[2] with U[3], and so on; a last odd one has twin = -1.  So twin is an involution without fixed
 *     points (twin[twin[h]] == h wherever twin[h] >= 0), BOUNDARY is -1, MANIFOLD and FLIPPED name the other half-edge, and on a
 *     NONMANIFOLD edge the pairing is pinned, not canonical, as L4 of ezrt_plane_loops.h is.  The neighbour of t across e is
 *     twin[3 t + e] / 3.
 * M6  Components.  Two TOPO-live triangles are connected when they have half-edges on one undirected edge, of any class; take the
 *     closure.  root[t] is the lowest triangle id of t's component.  Components are numbered by ascending root: component[t] in
 *     0 .. C - 1, comp_root[c] is the root, comp_size[c] the component's triangles, and comp_flags[c] has bit 0 / 1 / 2 set when
 *     any half-edge of the component is BOUNDARY / FLIPPED / NONMANIFOLD.  Triangles that meet only in a vertex are not connected.
 * M7  Summary.  [0] TOPO-live triangles; [1] undirected edges; [2] [3] [4] [5] undirected edges that are BOUNDARY, MANIFOLD, FLIPPED,
 *     NONMANIFOLD; [6] C (0 when the component group is NULL); [7] the largest m (0 without a live triangle).
 *
 * What follows from M1 .. M7.
 * - Nothing depends on the tree, on how the work was split, on the arrival order of threads, or on what `work` held.
 * - Reversing EVERY triangle's winding changes nothing at all: every edge keeps its class, its multiplicity and its pairs, and root,
 *   component, comp_* and summary are the same arrays.  (A triangle stored as (p1, p3, p2) has its half-edge e on the edge that
 *   half-edge 2 - e was on: with r(3 t + e) = 3 t + 2 - e the new per-half-edge arrays are the old ones at r(h), and the new twin is
 *   r(twin[r(h)]).)  Reversing ONE triangle changes classes only on its three edges (MANIFOLD <-> FLIPPED where m == 2).
 * - A permutation of the triangle ids permutes the outputs and keeps the partition, the class of every edge and every count of M7.
 *   On edges with m <= 2 it keeps twin as a relation too; on a NONMANIFOLD edge the pairing follows the ids.
 * - A mesh is CLOSED exactly when [2] == 0 && [5] == 0.
 * - A mesh is CONSISTENTLY WOUND exactly when [4] == 0 && [5] == 0.  A Moebius band has a FLIPPED edge whatever its stored windings.
 *
 * THE CALL.
 * ezrt_topology_work_bytes(n_tri) does no device work: the bytes of `work` a call on a scene of n_tri triangles needs -- a pure
 * function, monotone in n_tri, a multiple of 8, 8 for n_tri <= 0 (about 100 B per triangle: 32 to 64 B of table, 44 B of arrays).
 * ezrt_mesh_topology_device reads the scene's triangles and writes
 *   twin, edge_class   (3 n_tri each) M5, M4, for every half-edge;
 *   mult               (3 n_tri, or NULL) M4;
 *   root, component    (n_tri each) M6, for every triangle;
 *   comp_root, comp_size, comp_flags   (n_tri each) M6: entries 0 .. C - 1; entries at and beyond C are NOT TOUCHED;
 *   summary            (8) M7.
 * root, component, comp_root, comp_size and comp_flags are the COMPONENT GROUP: all five, or all NULL, and then the union-find is not
 * run and summary[6] is 0.  `s` supplies the device, the error slot and the triangles.  work is scratch of at least
 * ezrt_topology_work_bytes(n_tri) bytes, 8-byte aligned, whose contents before and after the call mean nothing; two calls in flight
 * at once need two.
 * ezrt_mesh_topology_at_device is the same rule for pairs already held, one lane per pair and no table: for edge edge_a[i] of
 * triangle tri_a[i], shared[i] is the edge e of tri_b[i] that is the same undirected edge by M1 to M3 (at most one is), else -1, and
 * opposite[i] is 1 when the two half-edges run opposite ways, 0 when they run the same way, -1 without a shared edge.  An id out of
 * range, an edge not in 0 .. 2, or either triangle not TOPO-live gives -1 / -1.  tri_a[i] == tri_b[i] gives edge_a[i] / 0.
 *
 * How it is computed.  JOIN: one lane per half-edge inserts into an open-addressed table of the next power of two of at least
 * 6 n_tri slots (at most half full); a slot is claimed by atomicCAS with a representative half-edge, keys are compared by reading the
 * representative's vertices, which nobody writes, and each half-edge pushes itself and its direction onto its slot's lock-free list
 * by an atomic exchange.  RANK, a launch of its own so that the lists cross a launch boundary before anyone walks them: each
 * half-edge walks its slot's list for m, its direction group and its rank among lower h, and writes twin, edge_class and mult; the
 * lowest h of an edge counts it, one atomic per wave.  COMPONENTS: a lock-free union-find over triangles with parent[t] <= t, every
 * half-edge uniting its triangle with its slot's representative's, the higher root hooked under the lower by atomicCAS -- the
 * surviving root is the lowest id whatever the order; then a flatten, a prefix sum over the roots, and a scatter.  The table and the
 * union-find are shared by all workgroups of a launch: inside a launch they are touched by device-scope atomics only, everything
 * else crosses a launch boundary.  Every loop is bounded: probes by the table's size, walks by 3 n_tri, finds by the strictly
 * descending parent.  KNOWN LIMIT: an edge of multiplicity m <= 2 costs its half-edges one short walk each; on a NONMANIFOLD edge a
 * half-edge also searches the list for the holder of a rank, O(m^2) steps per half-edge.  Multiplicities above 2 are defects and are
 * rare; a mesh that stores one face thousands of times is slow.
 *
 * Memory, streams, ordering and errors are those of ezrt_plane.h: every pointer is device memory of the scene's device, large enough
 * for its elements (anything else is rejected before any launch, never dereferenced); the work is enqueued on `stream` and the call
 * returns without synchronising or allocating; it may run beside ezrt_render_device and the other queries on other streams and
 * leaves ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for it.  The topology is taken BY VALUE:
 * after a refit it can change, and the call has to be made again.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene, twin, edge_class, summary or work; a partly NULL
 * component group; work_bytes below ezrt_topology_work_bytes(n_tri) or work not 8-byte aligned; a scene of more than INT32_MAX / 3
 * triangles; a pointer that is not device memory of the scene's device; for the _at call NULL scene, tri_a, edge_a, tri_b, shared or
 * opposite, or n < 0.  A scene without triangles, and n == 0, return 0 and launch nothing. */
#ifndef EZRT_TOPOLOGY_H
#define EZRT_TOPOLOGY_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_EDGE_BOUNDARY 1
#define EZRT_EDGE_MANIFOLD 2
#define EZRT_EDGE_FLIPPED 3
#define EZRT_EDGE_NONMANIFOLD 4

/* the bytes of `work` for a scene of n_tri triangles (pure, monotone, a multiple of 8; no device work; never fails) */
size_t ezrt_topology_work_bytes(int n_tri);
int ezrt_mesh_topology_device(EzrtScene* s, int32_t* twin /* 3 * n_tri */, uint8_t* edge_class /* 3 * n_tri */, int32_t* mult /* 3 * n_tri, or NULL */,
                              int32_t* root /* n_tri, or NULL together with the next four */, int32_t* component /* n_tri */,
                              int32_t* comp_root /* n_tri: entries >= C are not touched */, int32_t* comp_size /* n_tri: likewise */,
                              uint8_t* comp_flags /* n_tri: likewise */, int64_t* summary /* 8 */, void* work, size_t work_bytes, void* stream);
int ezrt_mesh_topology_at_device(EzrtScene* s, const int32_t* tri_a, const int32_t* edge_a, const int32_t* tri_b, int n,
                                 int8_t* shared /* n: -1 no shared edge, else the edge e of tri_b */,
                                 int8_t* opposite /* n: 1 opposite directions, 0 same, -1 none */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
