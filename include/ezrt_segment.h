/* ezrt_segment.h -- stream-ordered segment queries on device memory (libezrt_hip.so only): the clearance of a line segment from the
 * mesh, and the triangles a capsule touches.
 *
 * The segment, and the capsule around it, is the shape most collision and clearance code is built on: a robot link, a character
 * controller, a cable, a drill shaft, a "thick ray", the whole path of a moving sphere.  Closest-point calls on sample points along the
 * segment are not exact and miss an edge that passes its middle; ezrt_tri_distance.h on a sliver triangle is not live when the sliver is
 * collinear and pays 15 sub-candidates and 29 directions for a 5-candidate problem; ezrt_sphere_cast.h stops at the first contact and
 * cannot say how close the path comes when it does not touch, nor list everything the swept volume touches.
 *
 *   segs6      n x 6 floats: THE TWO END POINTS a, b OF EVERY SEGMENT -- a.x a.y a.z b.x b.y b.z.  NOT AN ORIGIN AND A DIRECTION: every
 *              other 6-float input of this library is a ray (o, d); the segment of a ray up to t is (o, o + t d)
 *   d_max      n floats, or NULL (= +inf for every segment): only triangles within this distance are candidates
 *   radius     n floats: the radius of every capsule
 *
 * THE DEFINITION.  All arithmetic is fp32 (IEEE binary32, round to nearest even), one rounding per written operation, no contraction
 * (-ffp-contract=off, as everywhere in the library), with the conventions of ezrt_closest_point.h and ezrt_tri_distance.h: + - *
 * componentwise on vectors, dot(u, w) = u.x*w.x + u.y*w.y + u.z*w.z evaluated left to right, IEEE divisions, min(x, y) = (y < x) ? y : x
 * and max(x, y) = (x < y) ? y : x (ez_min, ez_max), clamp01(v) = min(max(v, 0), 1).  The only fp64 arithmetic is that of the two rules
 * called as they stand: LIVE of ezrt_tri_overlap.h and the segment test of ezrt_self_overlap.h.
 *
 * Liveness.  A query segment is LIVE when its six numbers are finite; a == b is live and is a point.  A scene triangle S = (p, q, r)
 * (the scene's p1 p2 p3 of triangle k) is LIVE by the rule of ezrt_tri_overlap.h -- nine finite coordinates and a normal N != (0, 0, 0)
 * of the sorted vertices --, which is what the segment test requires of its triangle.  A query that is not live misses
 * (ezrt_query_segment_distance_device) or has an empty row and a count of 0 (ezrt_query_capsule_overlap_device); a scene triangle that
 * is not live is never a candidate.  A capsule's radius must be finite and >= 0, else the query is not live.
 *
 * Sub-candidates.  The distance of the pair ([a, b], S) is taken over FIVE sub-candidates in this order; each yields a point x on the
 * segment, a point y on S and d2 = dot(e, e), e = x - y.  THE VERTICES OF S AND THE END POINTS ARE TAKEN IN THE ORDER GIVEN.
 *    0, 1     end point a, then b, against S: closest_point_triangle of ezrt_closest_point.h as it stands, with p the end point and
 *             (a, b, c) = (p, q, r).  x = the end point, y = its q (already clamped to S's bounding box), d2 = its dist2.
 *    2 .. 4   the segment against the edges (p, q), (q, r), (r, p) of S: the closest points of two closed segments of
 *             ezrt_tri_distance.h as they stand (s, t, the clamps of x and y into the bounding boxes of their segments), with [a, b] AS
 *             THE FIRST segment [P1, Q1] and the edge as the second [P2, Q2].  (For a == b: a = dot(d1, d1) = 0, den <= 0, s = 0 or the
 *             clamp of a 0/0 -- a NaN, which the clamp of x to [a, a] does not mend: such a d2 is not finite and is skipped.)
 * A sub-candidate whose d2 is not finite (NaN, +inf) is skipped.  dist2 of the pair is the smallest finite d2; the FIRST sub-candidate in
 * the order above wins on equality and supplies the pair's (x, y).  If no d2 is finite the pair is no candidate.  The five are complete:
 * the minimum of a segment against a triangle is attained at an end point of the segment, or at an interior point of the segment
 * against an edge of the triangle -- or the two cross.
 *
 * Crossing.  crosses = T1 && seg_meets(lo, hi; S), where
 *   T1         min(a, b) <= max(p, q, r) && min(p, q, r) <= max(a, b) on all three axes: the closed fp32 comparison of the segment's
 *              bounding box with the triangle's
 *   seg_meets  the test of a closed segment against a closed live triangle of ezrt_self_overlap.h, unchanged (the normal, g x axis_j
 *              for the segment and the three edges, and d x f_j: 16 directions in fp64 on the sorted vertices); (lo, hi) = (a, b) in
 *              the order of their values (x, then y, then z), as that rule takes its segment.
 * Where crosses holds the pair's dist2 is 0 and its `crosses` is 1; (x, y) stay those of the 5-way minimum: THEY ARE THE NEAREST
 * FEATURES, NOT A COMMON POINT -- a segment that pierces the interior of a face has five positive d2.  T1 IS NOT OPTIONAL: seg_meets
 * is a rounded fp64 test and may fail to separate a near miss whose boxes are disjoint; dist2 = 0 would then sit under a node whose
 * lower bound is positive, and the answer would depend on the tree.  With T1 a crossing pair has overlapping boxes and a bound of 0.
 * For a == b the six directions built from d = b - a are zero vectors and separate nothing; the normal of S and the nine g x axis_j
 * of its edges remain -- the plane, and the three edge tests in each coordinate projection --, and with T1 they are complete for a
 * point (tests/test_segment_expected.py holds them against the exact answer).
 *
 * ezrt_query_segment_distance_device.  B = d_max*d_max (fp32; +inf when d_max is NULL; a d_max that is not >= 0 -- NaN, negative --
 * gives no candidates).  The candidates are the pairs with a dist2 <= B.  The smallest dist2 wins.  Among equal dist2 a pair that
 * crosses comes before a pair that does not, and then the smallest scene index k wins, for the reason given in ezrt_tri_distance.h: all
 * crossed triangles have 0, and so has a triangle whose nearest sub-candidate rounds to 0.  So `crosses` is 1 EXACTLY when the segment
 * crosses some live triangle of the scene, and tri_id is then the lowest index among them.  THE ANSWER NEVER DEPENDS ON THE TREE.
 *   tri_id        the winning scene triangle, -1 for a miss
 *   dist          sqrtf(dist2) of the winner, +inf for a miss                                         (may be NULL)
 *   point_query   x of the winner, on the segment; zeros for a miss                                   (may be NULL)
 *   point_scene   y of the winner, on the scene triangle; zeros for a miss                            (may be NULL)
 *   crosses       uint8: 1 when the winner crosses or touches the segment, else 0; 0 for a miss       (may be NULL)
 *
 * ezrt_segment_distance_at_device evaluates the pair rule for (segment i, triangle tri_id[i]) the caller holds -- winners of an
 * earlier call, rows of ezrt_query_capsule_overlap_device or ezrt_query_nearest_device -- and writes dist, point_query, point_scene and
 * crosses as above (no d_max).  An id outside the scene, a segment or a triangle that is not live or a pair without a finite
 * sub-candidate writes the miss values (+inf, zeros, zeros, 0).  At least one output is required.
 *
 * ezrt_query_capsule_overlap_device.  Triangle k is in the capsule of query i when the pair is a candidate and dist2 <= R2, with
 * R2 = radius*radius in fp32 (an R2 that overflows to +inf admits every candidate).  radius = 0 lists the crossed triangles AND any
 * triangle whose nearest sub-candidate rounds to 0.  Rows and counts are those of ezrt_box_overlap.h:
 *   n_overlap[i]    the full number of triangles in the capsule, even past max_k                    (may be NULL when max_k > 0)
 *   tri_id row i    the min(max_k, n_overlap[i]) LOWEST indices of them in ascending order, then -1
 * max_k is in 0 .. EZRT_CAPSULE_OVERLAP_MAX; with max_k == 0 tri_id is ignored and n_overlap is required: a count-only call.
 *
 * What follows, on the bits.  ezrt_query_segment_distance_device with d_max = r finds a triangle exactly where
 * ezrt_query_capsule_overlap_device with radius = r counts > 0; while the count is <= max_k that winner is in the row; and
 * ezrt_segment_distance_at_device on a capsule's row gives a dist whose dist2 <= R2 (dist itself is sqrtf(dist2): dist*dist may differ
 * from dist2 by the rounding of the root and the product).
 *
 * What is NOT promised.  Invariance under swapping a and b (the end points come in another order and the segment formula starts from
 * a); bit-equality with ezrt_closest_point.h for a == b (an edge-pair sub-candidate may round lower than the point's q); agreement of
 * `crosses` with the fp32 ray test of ezrt_query_closest_device / ezrt_query_occluded_device; bit-agreement with ezrt_sphere_cast.h.
 *
 * How it is computed.  Where the scene prunes (ezrt_scene_prune_info [0] is not -1; decided per call, a refit can change it) one
 * segment per lane walks the 4-wide records best-first with the lower bound of a box [lo, hi] taken against the segment's fp32
 * bounding box [qlo, qhi] = [min(a, b), max(a, b)]:
 *   g = max(lo - qhi, 0, qlo - hi) per axis;  lb = dot(g, g)
 * A subtree is skipped only when lb > the radius (or lb is not finite) and descended on equality; the radius is the best dist2 so far
 * (segment distance) or R2 (capsule overlap).  WHY NO MARGIN IS NEEDED: every x is an end point or is clamped into [qlo, qhi]; every y
 * is clamped into the bounding box of S or of an edge of S, which lies in every box above S.  Per axis either g = 0 <= |e|, or
 * g = fl(lo - qhi) with y >= lo > qhi >= x: y - x >= lo - qhi in the reals, rounding is monotone and |fl(x - y)| = fl(y - x), so |e| >= g
 * (the same on the other side).  fl(x*x) is monotone in |x| and fl(fl(X + Y) + Z) in each of X, Y, Z >= 0, so lb <= d2 ON THE BITS for
 * every sub-candidate with a finite d2, hence lb <= the pair's dist2; a pair that crosses passes T1, so lb = 0 = dist2.  THE CAPSULE'S
 * WALK DOES NOT INFLATE THE SEGMENT'S BOX BY THE RADIUS: fl(qhi + r) can round below qhi + r and would cut off a triangle whose
 * dist2 <= R2; lb <= R2 is the necessary condition with no slack.  The same lb of S's own bounding box gates the pair before its five
 * sub-candidates and the fp64 test.  Triangles below no leaf are swept after the walk.  Otherwise (malformed or tiny scenes) the same
 * pair function sweeps all n_tri triangles without a tree.  Both give the answer defined above, bit for bit.
 *
 * Memory, streams, ordering and errors are those of ezrt_closest_point.h: every pointer is device memory of the scene's device, large
 * enough for its n (or n x 3, n x 6, n x max_k) elements (anything else is rejected before any launch, never dereferenced); work is
 * enqueued on `stream` and the call returns without synchronising; no scratch set is used; the calls may run beside ezrt_render_device
 * and the other queries on other streams and leave ezrt_counters and ezrt_last_render_ms alone; a later refit (ezrt_refit.h) waits for
 * them, and a call issued after the refit returned sees the new geometry.
 *
 * Return 0 or EZRT_ERR_INVALID (message in ezrt_last_error()): NULL scene or segs6; NULL tri_id (the two distance calls); NULL radius;
 * n < 0; no output at all (ezrt_segment_distance_at_device); max_k outside 0 .. EZRT_CAPSULE_OVERLAP_MAX; max_k > 0 with NULL tri_id;
 * max_k == 0 with NULL n_overlap; a pointer that is not device memory of the scene's device.  n == 0 returns 0 and launches nothing. */
#ifndef EZRT_SEGMENT_H
#define EZRT_SEGMENT_H

#include <stdint.h>

#include "ezrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EZRT_CAPSULE_OVERLAP_MAX 64

int ezrt_query_segment_distance_device(EzrtScene* s, const float* segs6 /* n x 6: a, b */, const float* d_max /* n or NULL */, int n,
                                       int32_t* tri_id /* n */, float* dist /* n or NULL */, float* point_query /* n x 3 or NULL */,
                                       float* point_scene /* n x 3 or NULL */, uint8_t* crosses /* n or NULL */, void* stream);
int ezrt_segment_distance_at_device(EzrtScene* s, const float* segs6 /* n x 6: a, b */, const int32_t* tri_id /* n */, int n,
                                    float* dist /* n or NULL */, float* point_query /* n x 3 or NULL */, float* point_scene /* n x 3 or NULL */,
                                    uint8_t* crosses /* n or NULL */, void* stream);
int ezrt_query_capsule_overlap_device(EzrtScene* s, const float* segs6 /* n x 6: a, b */, const float* radius /* n */, int n, int max_k,
                                      int32_t* tri_id /* n x max_k, or NULL when max_k == 0 */, int32_t* n_overlap /* n, or NULL */,
                                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
