/* ezrt_build.h -- GPU scene-build entry points of libezrt_hip.so.
 *
 * ezrt_build_lbvh replaces, for scenes where the host build dominates end-to-end time, the pair
 *   buildBVHwithSAH(triangles, nodes, 0, n-1, leaf_n)        P3/main.cpp:457-588, called at 707-715
 *   + the encode loops                                        P3/main.cpp:720-748
 * with a linear BVH built on the GPU (Morton order, Karras 2012).  Input and output use the
 * reference's encoded layouts: triangles as 36 floats (P3/main.cpp:61-72), nodes as 12 floats
 * (74-78; node 0 = the testNode sentinel, root = node 1, child ids > parent id, leaves of at most
 * leaf_n triangles over a contiguous range of tri_out).  It is an ALTERNATIVE builder: tree shape
 * and node numbering differ from the reference's, so images rendered with it agree with the
 * oracle run on the same arrays, not with images rendered from a buildBVHwithSAH tree.
 *
 * tri_out must hold n_tri * 36 floats, nodes_out nodes_capacity * 12 floats; 2 * n_tri nodes always
 * suffice.  *n_nodes receives the node count (including node 0), *build_ms (optional) the device
 * time of the build without the host<->device copies.  Returns 0 or a negative EZRT_ERR_* code
 * (message in ezrt_last_error()).  EZRT_ERR_INVALID: a NULL pointer (build_ms excepted), n_tri <= 0, leaf_n < 1 (> 128 for
 * ezrt_build_lbvh), or nodes_capacity below the tree's node count -- nodes_out is then left untouched.
 * EZRT_ERR_UNSUPPORTED: n_tri >= 2^24, refused before anything is read.  An entry that fails has written no partial tree.
 *
 * Input in contract (tests/test_gpu_build_edges.py):
 *   ezrt_build_sah, ezrt_build_median  equal the host builder on the bits for ANY input without NaN centroids: +-inf, +-0 and
 *       subnormal coordinates, coordinates beyond the builder's INF = 114514 and 1145141919 start values, centroid sums that
 *       overflow, and any depth -- n identical triangles, or triangles whose box has two zero extents, make every SAH cost tie
 *       and peel one triangle per level (depth n - leaf_n + 1; the level loop runs until no range is left to split, n levels
 *       at most).  With a NaN centroid the host comparator `a < b` is no strict weak order and the result is unspecified.
 *   ezrt_build_lbvh  accepts NaN vertices as well.  Its boxes are the exact min/max of the triangles below for every finite
 *       input, up to FLT_MAX; the fold is minNum/maxNum, so a NaN coordinate does not enter a box, and it orders the zeros:
 *       a zero lower bound is -0 if any zero below it is, a zero upper bound +0 if any is. */
#ifndef EZRT_BUILD_H
#define EZRT_BUILD_H

#ifdef __cplusplus
extern "C" {
#endif

int ezrt_build_lbvh(const float* tri, int n_tri, int leaf_n, float* tri_out, float* nodes_out, int nodes_capacity,
                    int* n_nodes, float* build_ms);

/* buildBVHwithSAH itself on the GPU: same arguments as ezrt_build_lbvh, and EXACTLY the arrays the host
 * sequence `nodes = {testNode}; buildBVHwithSAH(triangles, nodes, 0, n-1, leaf_n); encode` produces
 * (ezrt::buildBVHwithSAH of include/ezrt_scene.hpp: same triangle order, same nodes, same ids) -- the
 * parity builder, level by level with radix sorts and segmented scans instead of O(nodes) std::sort calls. */
int ezrt_build_sah(const float* tri, int n_tri, int leaf_n, float* tri_out, float* nodes_out, int nodes_capacity,
                   int* n_nodes, float* build_ms);
/* buildBVH (the median-split builder, P3/main.cpp:394-454) on the GPU, same contract: exactly the arrays of
 * `nodes = {testNode}; buildBVH(triangles, nodes, 0, n-1, leaf_n); encode`. */
int ezrt_build_median(const float* tri, int n_tri, int leaf_n, float* tri_out, float* nodes_out, int nodes_capacity,
                      int* n_nodes, float* build_ms);

/* Number of HIP devices this process can see (0 when there is none or the runtime cannot initialise): lets a host
 * decide between ezrt_build_sah and the host buildBVHwithSAH -- both produce the same arrays -- without touching a
 * device.  The Python layer picks the GPU builder for scenes of >= 100 000 triangles when this is > 0. */
int ezrt_build_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
