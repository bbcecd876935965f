// mesh_edges.hpp -- the edge list of a triangle list, shared by meshfilter.hip and meshquality.hip.
//
// Entry 3 t + e is the edge (i_e, i_{e+1}) of triangle t as the key (min << 32 | max), with its slot
// 3 t + e as the value.  The caller radix-sorts the pairs (stably, so a run of equal keys lists its
// triangles in ascending order), then walks the runs: one run is one distinct edge, its length the number
// of triangles on it.  A lock-free union-find hooked on the runs gives the connected components: the
// filter unites the triangles of a run, the quality pass the two vertices of a key.  The kernels are
// static: each including file gets its own copy.  nb() and k_iota are device_prims.hpp's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_prims.hpp"

namespace mqr {
namespace edges {

// A loop edge (u == v, a degenerate triangle's) is a real key for the filter: Open3D's
// ClusterConnectedTriangles counts it as adjacency, so two triangles that share one are one cluster.  The
// reference's edge metrics skip it, so the quality pass (DROP_LOOPS) gives it `none`, a key past every
// real one: the dropped entries sort to the end.
template <bool DROP_LOOPS>
static __global__ void k_edge_keys(const int32_t* __restrict__ tri, int64_t nt, uint64_t none, uint64_t* keys,
                                   int32_t* slot) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * nt) return;
    const int64_t t = i / 3;
    const int k = (int)(i % 3);
    const uint32_t a = (uint32_t)tri[3 * t + k], b = (uint32_t)tri[3 * t + (k + 1) % 3];
    keys[i] = DROP_LOOPS && a == b ? none : a < b ? ((uint64_t)a << 32 | b) : ((uint64_t)b << 32 | a);
    slot[i] = (int32_t)i;
}

// ---- runs of equal keys in the sorted array keys[0..m)
// entry i + d exists and has entry i's key
__device__ inline bool same_key(const uint64_t* __restrict__ keys, int64_t m, int64_t i, int d) {
    return (d < 0 ? i + d >= 0 : i + d < m) && keys[i + d] == keys[i];
}
// entry i, whose key is k, is the head of its run
__device__ inline bool run_head(const uint64_t* __restrict__ keys, int64_t i, uint64_t k) {
    if (i > 0 && keys[i - 1] == k) return false;  // the run began before i
    return true;
}
// length of the run that starts at head i, capped at 3
__device__ inline int run_length3(const uint64_t* __restrict__ keys, int64_t m, int64_t i) {
    return !same_key(keys, m, i, 1) ? 1 : same_key(keys, m, i, 2) ? 3 : 2;
}
// entry i (anywhere in its run) belongs to a run of more than two
__device__ inline bool run_over_two(const uint64_t* __restrict__ keys, int64_t m, int64_t i) {
    const bool p1 = same_key(keys, m, i, -1), n1 = same_key(keys, m, i, 1);
    return (p1 && same_key(keys, m, i, -2)) || (p1 && n1) || (n1 && same_key(keys, m, i, 2));
}

// ---- union-find over parent[] (k_iota first)
__device__ inline int32_t uf_find(int32_t* p, int32_t x) {
    while (true) {
        const int32_t px = p[x];
        if (px == x) return x;
        const int32_t gx = p[px];
        if (gx != px) p[x] = gx;  // path halving (benign race: any ancestor is a valid parent)
        x = gx;
    }
}

// Hook the larger root under the smaller, so a component's root is its lowest member.
__device__ inline void uf_union(int32_t* parent, int32_t a, int32_t b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(&parent[b], b, a) == b) return;
    }
}

}  // namespace edges
}  // namespace mqr
