// bucket_tree.hpp -- the Morton-bucket tree over a point set, shared by color.hip (knn colour fill) and
// meshcompare.hip (nearest neighbour): Morton-sorted buckets of kBucket points under an implicit complete
// binary tree of bucket boxes (heap order, leaves at P + b), and the float32 lower bound its searches prune
// on.  The build (bucket_tree.hip owns its kernels) runs on the caller's stream into the caller's storage;
// points are addressed through an index array (`ids`: the subset color.hip samples) or taken in order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_prims.hpp"

namespace mqr {

constexpr int kBucket = 16;

struct BucketTree {
    const float4 *lo, *hi;  // [2 P] node boxes, heap order (node 1 is the root, leaf b is node P + b)
    const float4* pts;      // [n] the points in Morton order: x, y, z, index bits
    const uint32_t* bb;     // [6] the points' bounds as ordered keys: the frame of the Morton keys
    int64_t n, P;           // points; leaves, a power of two >= the buckets
    int depth;              // levels below the root
};

// leaves of the tree over n points
inline int64_t bucket_tree_leaves(int64_t n) { return pow2_at_least((n + kBucket - 1) / kBucket); }
// bytes of each of `lo` and `hi` for n points (`pts` takes sizeof(float4) n, `bb` six words)
inline size_t bucket_tree_node_bytes(int64_t n) { return sizeof(float4) * 2 * (size_t)bucket_tree_leaves(n); }

// bytes of build scratch (keys x2, sorted ids, optional identity ids, sort temp) for n points; 0 when the
// sort cannot be sized
size_t bucket_tree_scratch_bytes(int64_t n, bool identity_ids, hipStream_t s);
// enqueue the whole build on s into caller-provided storage; no synchronisation, no allocation.  The first
// error of a copy, the sort or a launch, else hipSuccess.
hipError_t bucket_tree_build(hipStream_t s, const float* V, const int32_t* ids /* nullptr: identity */, int64_t n,
                             void* scratch, size_t scratch_bytes, float4* lo, float4* hi, float4* pts, uint32_t* bb,
                             BucketTree* out);
// The build's first two steps on their own.  Bounds of V[ids[0..n)] accumulated into bb (initialised by the
// caller to {~0, ~0, ~0, 0, 0, 0}): mesh measure's bounding box.  Morton keys of Q[ids[0..n)] in the frame
// bb: a searcher sorts its queries by them, so a wave's queries are neighbours in the tree.
void bucket_tree_enqueue_bounds(hipStream_t s, const float* V, const int32_t* ids, int64_t n, uint32_t* bb);
void bucket_tree_enqueue_keys(hipStream_t s, const float* Q, const int32_t* ids, int64_t n, const uint32_t* bb,
                              uint64_t* keys);

// A lower bound of the squared distance from q to a box, in float32: every operation is correctly rounded
// (relative error <= 2^-24 each, <= 2^-21 for the whole sum of three squares of differences), so shrinking
// by 2^-18 leaves a bound below the exact value; underflow only lowers it.  Pruning on it skips no box the
// exact float64 test would keep, and the visiting order cannot change the result (the list is a total
// order on (d2, index)).  Overflow is outside the proof: a difference beyond ~1.8e19 squares to +inf, which
// is no lower bound of a finite float64 distance.  meshcompare.hip rejects coordinates beyond 1e18; the
// colour fill's vertices are metres of a scanned room.
__device__ inline float box_d2_lb(const float q[3], float4 lo, float4 hi) {
    const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = fmaxf(fmaxf(l[a] - q[a], q[a] - h[a]), 0.f);
        s += t * t;
    }
    return s * (1.0f - 0x1p-18f);
}

}  // namespace mqr
