/* ezrt_inside.h -- stream-ordered inside and signed-distance queries on device memory (libezrt_hip.so only).
 *
 * Is a point inside the mesh, and how far is it from the surface with a sign: the question behind occupancy and signed distance
 * fields, voxelisation, containment and clearance checks, culling points inside an object.  The closest-point queries give |d|
 * only, and the hit count of ezrt_query_all_hits_device is hitTriangle's (it starts at t >= 0.0005 and both triangles of a shared
 * edge accept a ray through that edge), so its parity cannot be trusted.  The rule below can: it is consistent on shared edges and
 * vertices, it is defined on the triangle array alone, and it is cheap.
 *
 *   points3    n x 3 floats: the query points
 *   axis       0..5: the ray leaves the point along +x, -x, +y, -y, +z, -z
 *
 * THE DEFINITION.  No contraction anywhere (-ffp-contract=off, as everywhere in the library); one rounding per written operation.
 *
 * The frame of an axis.  c = axis >> 1 is the ray's coordinate (0 x, 1 y, 2 z) and g = (axis & 1) ? -1.0f : 1.0f.  Of a vector x,
 *   x.s = x[(c + 1) % 3],  x.t = x[(c + 2) % 3],  x.u = g * x[c]     (fp32; a product with +-1 is exact)
 * so in its frame every ray runs along +u, and (s, t) is the plane the mesh is projected to.
 *
 * Triangle k (p1 p2 p3 of triangle k of the array given to ezrt_scene_create, in the frame) is CROSSED by the ray of p when all of
 * G1 .. G6 hold.  G1 - G3 are fp32 comparisons on the three vertices in any order:
 *   G1  some vertex has s <= p.s and some vertex has not                         (the half-open straddle rule)
 *   G2  some vertex has t <= p.t and some vertex has t >= p.t
 *   G3  some vertex has u >  p.u
 * The vertices are then put in the order of their VALUES, v0 <= v1 <= v2, with
 *   less(x, y) = x.s < y.s || (x.s == y.s && (x.t < y.t || (x.t == y.t && x.u < y.u)))
 *   if less(p2, p1) swap(p1, p2);  if less(p3, p2) swap(p2, p3);  if less(p2, p1) swap(p1, p2);   (v0 v1 v2) = (p1 p2 p3)
 * -- after G1, v0.s <= p.s < v2.s -- and everything below is fp64 (IEEE binary64, round to nearest even) on the fp32 values
 * converted exactly; with d(x, y) = (double)x - (double)y:
 *   A   = d(v1.s,v0.s)*d(v2.t,v0.t) - d(v1.t,v0.t)*d(v2.s,v0.s)                  the projected area (twice, signed)
 *   G4  A is finite and A != 0                                                   an edge-on triangle never counts
 *   E02 = d(v2.s,v0.s)*d(p.t,v0.t) - d(v2.t,v0.t)*d(p.s,v0.s)                    the edge (v0, v2): it always straddles p.s
 *   E   = v1.s <= p.s ? d(v2.s,v1.s)*d(p.t,v1.t) - d(v2.t,v1.t)*d(p.s,v1.s)      the edge (v1, v2), or
 *                     : d(v1.s,v0.s)*d(p.t,v0.t) - d(v1.t,v0.t)*d(p.s,v0.s)      the edge (v0, v1): the other one that straddles
 *   G5  (E02 < 0) != (E < 0)                                                     exactly one of the two lies above p in t
 *   Ns  = d(v1.t,v0.t)*d(v2.u,v0.u) - d(v1.u,v0.u)*d(v2.t,v0.t)
 *   Nt  = d(v1.u,v0.u)*d(v2.s,v0.s) - d(v1.s,v0.s)*d(v2.u,v0.u)
 *   D   = (Ns*d(p.s,v0.s) + Nt*d(p.t,v0.t)) + A*d(p.u,v0.u)                      the plane of the triangle meets the ray at -D / A
 *   G6  D is finite and ((D < 0 && A > 0) || (D > 0 && A < 0))                   strictly ahead: a point on the triangle is not
 *                                                                                ahead of itself
 *   crossings(p) = the number of crossed k in [0, n_tri);  a p with a non-finite coordinate has crossings = 0
 *   inside(p)    = crossings & 1
 *
 * What the rule guarantees.
 * - Edge decisions belong to the edge, not the triangle.  An edge is "above p" when its expression is < 0, and that expression is
 *   written on the edge's two endpoints in the order of their values (the lower s first: a straddling edge has two different s) and
 *   on p -- on nothing else.  Two triangles that share an edge BY VALUE therefore evaluate the same operations on the same numbers,
 *   whichever way round each of them holds it: they never both claim and never both disclaim a point of its projection, and the same
 *   holds at a shared vertex through G1.  No welding and no adjacency: a triangle soup will do.  In exact arithmetic the rule is the
 *   plain point-in-triangle test for the point p + (e*e, e) of the (s, t) plane, e > 0 as small as needed, which lies on no
 *   projected edge and under no projected vertex: the projected triangles tile the plane without overlap or gap.
 * - The vertex order and the winding of a triangle do not matter to a single bit, and neither does the order of the triangles: the
 *   vertices are sorted before any arithmetic and the count is an integer sum.
 * - A triangle with a NaN or infinite vertex never counts: every coordinate enters A or D, and G4 / G6 are false for NaN and inf.
 *   From fp32 inputs no fp64 operation here overflows.
 * - Exactness.  A difference of two floats is exact in double unless their exponents lie more than 29 apart, and the product of
 *   two differences is exact when their significands have no more than 53 bits together -- always on integer or fixed-point
 *   coordinates up to 2^26 steps, and on any mesh whose coordinates (and p) share a few binades.  The difference of two exact
 *   products has the right sign and is zero only for equal products, so G4 and G5 are then THE exact predicates.  Beyond that every
 *   product is rounded once (2^-53): the answers are still pinned, operation by operation, and still consistent across a shared edge
 *   (same operations, same values), but a point within about 2^-50 (relative to the edge's extent) of an edge's line may be given
 *   to the other side of it.  D is a sum of three rounded products: its sign is right unless p lies within about 2^-50 of the
 *   triangle's plane, relative to the triangle's and the point's extent.
 * - G1 - G3 change nothing in exact arithmetic (a crossed triangle's projection holds p's, and the crossing lies on the triangle).
 *   They are part of the definition so that a traversal may skip a box on fp32 comparisons alone, with no slack and no proof, even
 *   where the fp64 predicates are no longer exact.  NOTHING DEPENDS ON THE TREE.
 * - Open meshes (the Stanford Bunny has holes): the answer is still the parity pinned above, it is not a topological fact, and it
 *   may differ between axes for points whose ray leaves through a hole.  Callers vote over several axes; none is built in.
 *
 * ezrt_query_inside_device writes inside (0 / 1) and, where asked for, crossings.
 * ezrt_query_signed_distance_device writes tri_id, point and bary exactly as ezrt_query_closest_point_device does for the same
 * points and d_max (ezrt_closest_point.h), bit for bit, and
 *   sdist    that call's dist with the sign bit set where inside is 1: |sdist| equals dist on the bits, and a miss (no triangle
 *            within d_max, or none at all) is +inf outside and -inf inside                     (may be NULL)
 *   inside   as ezrt_query_inside_device's for the same axis                                   (may be NULL)
 *
 * How it is computed.  Where the scene prunes (ezrt_scene_prune_info [0] is not -1; decided per call, a refit can change it) one
 * point per lane walks the 4-wide records depth-first and descends a slot when lo.s <= p.s <= hi.s, lo.t <= p.t <= hi.t and the box
 * reaches ahead of p (hi.u > p.u; for the negative axes lo[c] < p[c]) -- comparisons only: by G1 - G3 a crossed triangle's own
 * bounding box passes them, and so does every box that holds it.  Triangles below no leaf are swept after the walk.  Otherwise
 * (malformed or tiny scenes) the same per-triangle function sweeps all n_tri triangles.  The signed distance runs the crossing
 * walk and then the closest-point walk in one launch.
 *
 * Memory, streams, ordering and errors are those of ezrt_closest_point.h: every pointer is device memory of the scene's device, large
 * enough for its n elements (anything else is rejected before any launch, never dereferenced); work is enqueued on `stream` and the
 * call returns without synchronising; no scratch set is used; the calls may run beside ezrt_render_device and the other queries on
 * other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for them, and a call
 * issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene or points3; NULL inside (ezrt_query_inside_device) or
 * tri_id (ezrt_query_signed_distance_device); n < 0; axis outside 0..5; a pointer that is not device memory of the scene's device.
 * n == 0 returns 0 and launches nothing. */
#ifndef EZRT_INSIDE_H
#define EZRT_INSIDE_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_query_inside_device(EzrtScene* s, const float* points3 /* n x 3 */, int n, int axis, uint8_t* inside /* n */,
                             int32_t* crossings /* n or NULL */, void* stream);
int ezrt_query_signed_distance_device(EzrtScene* s, const float* points3 /* n x 3 */, const float* d_max /* n or NULL */, int n, int axis,
                                      int32_t* tri_id /* n */, float* point /* n x 3 or NULL */, float* sdist /* n or NULL */,
                                      float* bary /* n x 2 or NULL */, uint8_t* inside /* n or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
