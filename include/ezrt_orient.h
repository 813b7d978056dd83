/* ezrt_orient.h -- stream-ordered mesh ORIENTATION on device memory (libezrt_hip.so only): a consistent winding, the patches it is
 * consistent on, their signed volumes, and the kernel that reverses the marked rows.
 *
 * ezrt_topology.h says that a mesh is wound inconsistently: FLIPPED edges, comp_flags bit 1.  ezrt_plane_loops.h closes its loops only
 * on a consistently wound manifold, ezrt_winding.h is negated by a flipped winding, ezrt_vertices.h sums face normals and a reversed
 * neighbour subtracts its share.  The call here answers what the topology cannot: WHICH triangles to reverse, whether a consistent
 * winding exists at all, and whether the result faces outward.  ezrt_rewind_device reverses the marked rows of the caller's array and
 * ezrt_refit.h takes them back.
 *
 * THE DEFINITION.  Every output is an integer.  The only floating-point arithmetic is the fp64 determinant of O6; it is pinned
 * operation by operation and followed by an integer sum.
 *
 * O1  Inputs taken by value.  The call reads twin and edge_class (3 n_tri each), normally those of ezrt_mesh_topology_device on the
 *     same scene, and the scene's stored positions.  It builds no table of its own.  A triangle TAKES PART when its three edge_class
 *     entries are all in 1 .. 4.
 * O2  Links.  Half-edge h = 3 t + e of a triangle that takes part is a LINK to g = twin[h] when all of these hold: edge_class[h] is 2
 *     or 3; 0 <= g < 3 n_tri; g / 3 != t; triangle g / 3 takes part; edge_class[g] == edge_class[h]; twin[g] == h.  The link's sign
 *     is s(h) = 0 for class 2 (the two triangles agree) and 1 for class 3 (they disagree).  Everything else is no link: BOUNDARY
 *     edges, NONMANIFOLD edges (no winding is implied there), and any entry that fails a test above.  Nothing out of bounds is read,
 *     whatever the arrays hold.  A link is symmetric: g is then a link to h, with the same sign.  On a topology's own arrays every
 *     edge with m == 2 is a link, by M4 and M5.
 * O3  Patches.  A patch is the closure of links over triangles that take part.  patch_root[t] is the lowest id of t's patch.
 *     Patches are numbered by ascending root: patch[t] is in 0 .. P - 1, and proot[p] and psize[p] describe patch p.  A triangle that
 *     does not take part has patch_root = patch = -1 and flip = 0.  A patch lies inside one M6 component; a component splits into
 *     patches at NONMANIFOLD edges.
 * O4  Orientable, flip.  Patch p is ORIENTABLE when there is an f: p -> {0, 1} with f(a) xor f(b) = s for every link between a and
 *     b.  Then f0 is the unique such f with f(root) = 0.  Otherwise the patch is non-orientable (a Moebius band, a Klein bottle) and
 *     f0 = 0 on all of it.  Non-orientability is a property of the patch, not of the traversal.
 * O5  Closed.  Patch p is CLOSED when every half-edge of every triangle in it is a link.
 * O6  Volume.  A is the largest |coordinate| among the nine stored fp32 coordinates of the triangles that take part, over finite
 *     coordinates only, compared on the bits.  E is the frexp exponent of (double)A, so that A < 2^E; E = 0 when A == 0.
 *     S = 3 E - 30.  For a triangle t that takes part, convert a = p1, b = p2, c = p3 to double and compute, with every operation
 *     rounded to fp64 as written and no contraction,
 *       d = (a.x * (b.y * c.z - b.z * c.y) + a.y * (b.z * c.x - b.x * c.z)) + a.z * (b.x * c.y - b.y * c.x).
 *     q(t) = llrint(ldexp(d, -S)), round to nearest even; q(t) = 0 when d is not finite.  The inner products are exact in fp64, so
 *     storing the triangle as (p1, p3, p2) gives exactly -d and exactly -q.  |q| < 2^33 and n_tri < 2^30, so no int64 sum of q can
 *     overflow.  vol6_0[p] is the int64 sum of (f0(t) ? -q(t) : q(t)) over the patch: an integer sum, whose order does not matter.
 *     The volume in scene units is vol6 * 2^S / 6; it is exact whenever every d is a multiple of 2^S (small integer coordinates).
 * O7  Outward.  With outward == 0: flip = f0 and vol6 = vol6_0.  With outward != 0, on every patch that is orientable, closed and
 *     has vol6_0 < 0: flip = 1 - f0 and vol6 = -vol6_0.  Every other patch is as with outward == 0: the signed volume of an open
 *     patch depends on the origin and decides nothing.  Each patch is treated on its own: a cavity inside a solid comes out facing
 *     outward as well; which patch lies inside which is a question for ezrt_inside.h.
 * O8  Flags and summary.  pflags[p]: bit 0 OPEN, the patch is not closed; bit 1 NONORIENTABLE; bit 2 REWOUND, some flip[t] == 1 in
 *     the patch; bit 3 INWARD, the patch is orientable and closed and vol6_0 < 0 -- set whether or not `outward` acted on it.
 *     summary (int64): [0] triangles taking part; [1] P; [2] orientable patches; [3] closed patches; [4] triangles with flip == 1;
 *     [5] patches with bit 3; [6] S; [7] 0.
 *
 * What follows from O1 .. O8.
 * - Nothing depends on the tree, on how the work was split, on the arrival order of threads, or on what `work` held.
 * - Reversing EVERY stored winding: twin and edge_class change as ezrt_topology.h says; with outward == 0, flip, patch and pflags bits
 *   0 to 2 are the same arrays and every vol6 is negated; with outward != 0, the re-wound mesh of the next item is the same set of
 *   oriented triangles on every closed orientable patch with vol6 != 0.
 * - Take the caller's rows, rewind them with flip, refit the scene, and run the topology and this call again.  Then no FLIPPED edge
 *   lies inside an orientable patch, summary[4] is 0, no patch has bit 2, and with outward != 0 no patch has bit 3.
 * - A mesh can be made CONSISTENTLY WOUND exactly when summary[2] == summary[1].
 *
 * THE CALLS.
 * ezrt_orient_work_bytes(n_tri) does no device work: the bytes of `work` a call on a scene of n_tri triangles needs -- a pure
 * function, monotone in n_tri, a multiple of 8, 8 for n_tri <= 0:  32 n_tri + 8 ceil(n_tri / 2048) + 24  (an int64 flag-and-number
 * and an int64 volume per triangle, four ints per triangle, an int64 per scan tile of 2048, one more int64 for each of the two
 * sums, and 8 bytes for A).
 * ezrt_mesh_orient_device reads twin, edge_class and the scene's triangles and writes
 *   flip, patch_root, patch       (n_tri each) O7, O3, for every triangle;
 *   proot, psize, pflags, vol6    (n_tri each) O3, O8, O7: entries 0 .. P - 1; entries at and beyond P are NOT TOUCHED;
 *   summary                       (8) O8.
 * `s` supplies the device, the error slot and the positions.  work is scratch of at least ezrt_orient_work_bytes(n_tri) bytes,
 * 8-byte aligned, whose contents before and after the call mean nothing; two calls in flight at once need two.  The topology is taken
 * BY VALUE: after a refit that changes windings it has to be made again, and so has this call.
 * ezrt_rewind_device works on the CALLER's rows, the array about to go into a refit, in place: where flip[t] != 0 it exchanges floats
 * 3-5 with 6-8 (p2 <-> p3) and floats 12-14 with 15-17 (n2 <-> n3).  A normal travels with its vertex unchanged; the caller who wants
 * smooth normals of the new winding calls ezrt_vertex_normals_device afterwards.  It writes nothing else: floats 0-2, 9-11, 18-35 and
 * rows with flip == 0 are untouched on the bits.  Applied twice it restores the rows.  `s` supplies the device and the error slot,
 * and n_tri must be the scene's.
 *
 * How it is computed.  Nine launches.  INIT.  UNION: one lane per half-edge runs a lock-free union-find with parity over triangles;
 * one 32-bit word per triangle holds parent << 1 | parity(t -> parent) with parent <= t; a link (a, b, s), taken once at its lower
 * half-edge, finds (ra, pa) and (rb, pb), and if the roots differ the higher root is hooked under the lower by atomicCAS from its
 * root word to (lower << 1 | pa ^ pb ^ s), with a retry on failure; paths are halved by atomicCAS from the word read to
 * (grandparent, p1 ^ p2), a true relation forever in an orientable patch.  The surviving root is the lowest id whatever the order.
 * FLATTEN, a launch of its own: every triangle's (root, parity to root), the patch sizes, A by an integer atomicMax on the bits.
 * CHECK, a launch of its own and not the union's same-root branch: every link whose flattened parities violate s marks its root
 * NONORIENTABLE, every half-edge that is no link marks it OPEN; in an orientable patch the tree's relations satisfy every link, in a
 * non-orientable one no assignment does, so some link is caught.  NUMBERING: a flag at each root and the vertex weld's tiled prefix
 * sum (three launches).  VOLUME: q(t), signed by f0, is summed over runs of neighbouring lanes that share a root by a segmented wave
 * scan, then added to the root's int64 by one integer atomicAdd per run.  FINISH: O7, then flip, patch, the patches' rows and the
 * counts.  Words shared between workgroups inside a launch are touched by device-scope atomics only; everything else crosses a
 * launch boundary.  Every loop is bounded: finds by the strictly descending parent, unions by n_tri retries.  No floating-point
 * atomics; the fp64 determinant is compiled without contraction.
 * KNOWN LIMIT: a long thin patch (a strip of 10^6 triangles) gives long parent chains before the flatten, and a lane of the union or
 * of the flatten walks its chain alone.  Measured on one MI355X (profiles/r32/orient_rates.txt): the strip of 10^6 triangles with
 * shuffled ids takes 0.62 ms a call (union 0.17, flatten 0.19, check 0.21 ms) beside 3.07 ms for the topology that feeds it -- path
 * halving keeps the chains short enough that they do not show at this size.  What does cost is ONE LARGE PATCH: every lane of it
 * meets at one root.  A closed torus of 999 698 triangles takes 1.78 ms, 1.34 ms of it in the union (the hooks and halvings of 1.5
 * million links contend for the words near the root), and each of the root's accumulators is served one atomic after the other, about
 * 11 ns each: with one atomic per lane the volume launch alone took 12.0 ms and the patch sizes 11.3 ms; with one per run of
 * neighbouring lanes (a wave at the most) they take 0.19 and 0.18 ms.
 *
 * Memory, streams, ordering and errors are those of ezrt_topology.h: every pointer is device memory of the scene's device, large
 * enough for its elements (anything else is rejected before any launch, never dereferenced); the work is enqueued on `stream` and
 * the call returns without synchronising or allocating; it may run beside ezrt_render_device and the other queries on other streams
 * and leaves ezrt_counters and ezrt_last_render_ms alone; a later refit waits for it.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): any NULL pointer (the stream excepted); work_bytes below
 * ezrt_orient_work_bytes(n_tri) or work not 8-byte aligned; a scene of more than INT32_MAX / 3 triangles; n_tri that is not the
 * scene's; a pointer that is not device memory of the scene's device.  A scene without triangles returns 0 and launches nothing. */
#ifndef EZRT_ORIENT_H
#define EZRT_ORIENT_H

#include <stddef.h>
#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_PATCH_OPEN 1
#define EZRT_PATCH_NONORIENTABLE 2
#define EZRT_PATCH_REWOUND 4
#define EZRT_PATCH_INWARD 8

/* the bytes of `work` for a scene of n_tri triangles (pure, monotone, a multiple of 8; no device work; never fails) */
size_t ezrt_orient_work_bytes(int n_tri);
int ezrt_mesh_orient_device(EzrtScene* s, const int32_t* twin /* 3 * n_tri */, const uint8_t* edge_class /* 3 * n_tri */, int outward,
                            uint8_t* flip /* n_tri */, int32_t* patch_root /* n_tri */, int32_t* patch /* n_tri */,
                            int32_t* proot /* n_tri: entries >= P are not touched */, int32_t* psize /* n_tri: likewise */,
                            uint8_t* pflags /* n_tri: likewise */, int64_t* vol6 /* n_tri: likewise */, int64_t* summary /* 8 */, void* work,
                            size_t work_bytes, void* stream);
int ezrt_rewind_device(EzrtScene* s, float* tri36 /* n_tri x 36: floats 3-8 and 12-17 of the marked rows are exchanged, nothing else */,
                       int n_tri, const uint8_t* flip /* n_tri */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
