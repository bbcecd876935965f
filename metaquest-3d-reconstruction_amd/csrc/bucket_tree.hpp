// bucket_tree.hpp -- the Morton-bucket tree over a point set, shared by color.hip (knn colour fill) and
// meshcompare.hip (nearest neighbour): Morton-sorted buckets of kBucket points under an implicit complete
// binary tree of bucket boxes (heap order, leaves at P + b), and the float32 lower bound its searches prune
// on.  The caller radix-sorts (key, id) pairs between k_cm_morton and k_cm_leaf_boxes.  Points are addressed
// through an index array (`ids`: the subset color.hip samples, or an identity array).  The kernels are static:
// each including file gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mqr {

constexpr int kBucket = 16;

__device__ inline uint32_t ordered_u32(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float from_ordered(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// Bounds of the sampled vertices: grid-stride with a capped grid, wave then workgroup reduction, one
// atomic per bound word and workgroup (256 threads).
static __global__ __launch_bounds__(256) void k_cm_bounds(const float* __restrict__ V, const int32_t* __restrict__ ids,
                                                          int64_t n, uint32_t* __restrict__ bb /* min x y z (ordered), max */) {
    __shared__ uint32_t part[4][6];
    uint32_t lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = ids[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t o = ordered_u32(V[3 * (int64_t)v + a]);
            lo[a] = min(lo[a], o);
            hi[a] = max(hi[a], o);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        uint32_t l = lo[a], h = hi[a];
        for (int o = 32; o >= 1; o >>= 1) {
            l = min(l, (uint32_t)__shfl_xor((int)l, o, 64));
            h = max(h, (uint32_t)__shfl_xor((int)h, o, 64));
        }
        if (lane == 0) {
            part[wave][a] = l;
            part[wave][3 + a] = h;
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        uint32_t r = part[0][c];
        for (int w = 1; w < 4; ++w) r = c < 3 ? min(r, part[w][c]) : max(r, part[w][c]);
        if (c < 3) atomicMin(&bb[c], r);
        else atomicMax(&bb[c], r);
    }
}

__device__ inline uint64_t spread21(uint32_t v) {
    uint64_t x = v & 0x1fffff;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

static __global__ void k_cm_morton(const float* __restrict__ V, const int32_t* __restrict__ ids, int64_t n,
                                   const uint32_t* __restrict__ bb, uint64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t v = ids[i];
    uint32_t c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = from_ordered(bb[a]), hi = from_ordered(bb[3 + a]);
        const float t = hi > lo ? (V[3 * (int64_t)v + a] - lo) / (hi - lo) : 0.f;
        c[a] = (uint32_t)fminf(fmaxf(t * 2097151.0f, 0.f), 2097151.f);
    }
    keys[i] = spread21(c[0]) | spread21(c[1]) << 1 | spread21(c[2]) << 2;
}

// leaf boxes (bucket b = sorted points [kBucket b, kBucket (b + 1)) ); empty leaves get an inverted box.
// Also the points themselves in that order, packed (x, y, z, vertex index bits), for the leaf scans.
static __global__ void k_cm_leaf_boxes(const float* __restrict__ V, const int32_t* __restrict__ sorted, int64_t n,
                                       int64_t P, float4* __restrict__ lo, float4* __restrict__ hi,
                                       float4* __restrict__ pts) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P) return;
    float l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t j = b * kBucket; j < min(n, (b + 1) * kBucket); ++j) {
        const int32_t v = sorted[j];
        const float p[3] = {V[3 * (int64_t)v], V[3 * (int64_t)v + 1], V[3 * (int64_t)v + 2]};
        pts[j] = make_float4(p[0], p[1], p[2], __int_as_float(v));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            l[a] = fminf(l[a], p[a]);
            h[a] = fmaxf(h[a], p[a]);
        }
    }
    lo[P + b] = make_float4(l[0], l[1], l[2], 0.f);
    hi[P + b] = make_float4(h[0], h[1], h[2], 0.f);
}

static __global__ void k_cm_level(int64_t first, int64_t count, float4* __restrict__ lo, float4* __restrict__ hi) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t n = first + i, a = 2 * n, b = a + 1;
    lo[n] = make_float4(fminf(lo[a].x, lo[b].x), fminf(lo[a].y, lo[b].y), fminf(lo[a].z, lo[b].z), 0.f);
    hi[n] = make_float4(fmaxf(hi[a].x, hi[b].x), fmaxf(hi[a].y, hi[b].y), fmaxf(hi[a].z, hi[b].z), 0.f);
}

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
