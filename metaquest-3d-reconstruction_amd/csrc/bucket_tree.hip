// bucket_tree.hip -- the build of bucket_tree.hpp's Morton-bucket tree, for color.hip's knn colour fill and
// meshcompare.hip's nearest neighbour: bounds of the points (ordered-key atomics) -> 63-bit Morton keys in
// that frame -> radix sort of (key, id) -> leaf boxes and the points in sorted order -> the inner levels
// bottom-up, one launch per level.  Everything is enqueued on the caller's stream into the caller's storage.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "bucket_tree.hpp"
#include "device_block.hpp"
#include "device_cub.hpp"

namespace mqr {

// Bounds of the addressed points: grid-stride with a capped grid, one atomic per bound word and workgroup
// (block_bounds_atomic).
__global__ __launch_bounds__(256) void k_cm_bounds(const float* __restrict__ V, const int32_t* __restrict__ ids,
                                                   int64_t n, uint32_t* __restrict__ bb /* min x y z (ordered), max */) {
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
    block_bounds_atomic(lo, hi, bb);
}

// (raycast.hip's k_morton quantises differently -- 2097152 with a clamp, x in the highest bits -- and its
// BVH's shape depends on that: the two stay apart)
__global__ void k_cm_morton(const float* __restrict__ V, const int32_t* __restrict__ ids, int64_t n,
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
__global__ void k_cm_leaf_boxes(const float* __restrict__ V, const int32_t* __restrict__ sorted, int64_t n, int64_t P,
                                float4* __restrict__ lo, float4* __restrict__ hi, float4* __restrict__ pts) {
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

__global__ void k_cm_level(int64_t first, int64_t count, float4* __restrict__ lo, float4* __restrict__ hi) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t n = first + i, a = 2 * n, b = a + 1;
    lo[n] = make_float4(fminf(lo[a].x, lo[b].x), fminf(lo[a].y, lo[b].y), fminf(lo[a].z, lo[b].z), 0.f);
    hi[n] = make_float4(fmaxf(hi[a].x, hi[b].x), fmaxf(hi[a].y, hi[b].y), fmaxf(hi[a].z, hi[b].z), 0.f);
}

// The build's scratch, stated once for bucket_tree_scratch_bytes and bucket_tree_build: the pieces, and the
// sort (written once: its size query is part of the layout).  `ids` is read when the sort runs.
struct BuildScratch {
    uint64_t* keys;  // unsorted, then sorted
    int32_t *sorted, *iota;
    CubTemp tmp;
    ScratchLayout L;
    auto sort(const int32_t* const& ids, int64_t n, hipStream_t s) const {
        return [this, &ids, n, s](void* t, size_t& b) {
            return hipcub::DeviceRadixSort::SortPairs(t, b, (const uint64_t*)keys, keys + n, ids, sorted, (int)n, 0, 63, s);
        };
    }
    hipError_t lay_out(const int32_t* const& ids, int64_t n, bool identity_ids, hipStream_t s) {
        L.add(keys, 2 * n);
        L.add(sorted, n);
        L.add(iota, n, identity_ids);
        return tmp.lay_out(L, sort(ids, n, s));
    }
};

size_t bucket_tree_scratch_bytes(int64_t n, bool identity_ids, hipStream_t s) {
    BuildScratch b;
    const int32_t* ids = nullptr;
    return b.lay_out(ids, n, identity_ids, s) == hipSuccess ? b.L.total() : 0;
}

void bucket_tree_enqueue_bounds(hipStream_t s, const float* V, const int32_t* ids, int64_t n, uint32_t* bb) {
    hipLaunchKernelGGL(k_cm_bounds, dim3(std::min(nb(n), 4096u)), dim3(256), 0, s, V, ids, n, bb);
}

void bucket_tree_enqueue_keys(hipStream_t s, const float* Q, const int32_t* ids, int64_t n, const uint32_t* bb,
                              uint64_t* keys) {
    hipLaunchKernelGGL(k_cm_morton, dim3(nb(n)), dim3(256), 0, s, Q, ids, n, bb, keys);
}

hipError_t bucket_tree_build(hipStream_t s, const float* V, const int32_t* ids, int64_t n, void* scratch,
                             size_t scratch_bytes, float4* lo, float4* hi, float4* pts, uint32_t* bb, BucketTree* out) {
    BuildScratch b;
    hipError_t err = b.lay_out(ids, n, !ids, s);
    if (err != hipSuccess) return err;
    // the buffer is the caller's: the carve has to fit it
    if (!scratch || !b.L.valid() || b.L.total() > scratch_bytes) return hipErrorInvalidValue;
    b.L.bind(scratch);

    const int64_t P = bucket_tree_leaves(n);
    auto step = [&](hipError_t e) {
        if (err == hipSuccess) err = e;
    };
    const uint32_t init[6] = {~0u, ~0u, ~0u, 0u, 0u, 0u};
    step(hipMemcpyAsync(bb, init, sizeof init, hipMemcpyHostToDevice, s));
    if (!ids) {
        hipLaunchKernelGGL(k_iota, dim3(nb(n)), dim3(256), 0, s, b.iota, n);
        ids = b.iota;
    }
    bucket_tree_enqueue_bounds(s, V, ids, n, bb);
    bucket_tree_enqueue_keys(s, V, ids, n, bb, b.keys);
    step(hipGetLastError());
    step(b.tmp.run(b.sort(ids, n, s)));
    hipLaunchKernelGGL(k_cm_leaf_boxes, dim3(nb(P)), dim3(256), 0, s, V, (const int32_t*)b.sorted, n, P, lo, hi, pts);
    for (int64_t first = P / 2; first >= 1; first /= 2)
        hipLaunchKernelGGL(k_cm_level, dim3(nb(first)), dim3(256), 0, s, first, first, lo, hi);
    step(hipGetLastError());
    *out = BucketTree{lo, hi, pts, bb, n, P, ceil_log2(P)};
    return err;
}

}  // namespace mqr
