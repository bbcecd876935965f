// device_prims.hpp -- the small building blocks the device modules share, each defined here once: launch
// arithmetic (nb, ceil_log2, pow2_at_least), the order-preserving float <-> uint32 key, the workgroup
// reduction of per-lane bounds into six atomics (block_bounds_atomic), the Morton bit spread (spread21), the
// order-fixed "sums + min + max into a slab" reduction with its final kernel (on pair_reduce.hpp), and the
// input checks every entry point runs before a kernel gathers through an index or prunes on a coordinate.
// Everything is inline, a template or a static kernel (maybe_unused: no including file launches all of them),
// so each including file compiles what it uses.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "pair_reduce.hpp"

namespace mqr {

// ------------------------------------------------------------------ host arithmetic
// workgroups of `per` items that cover n (at least one)
inline unsigned nb(int64_t n, int per = 256) { return (unsigned)((n > 0 ? n + per - 1 : per) / per); }

// the smallest b with 2^b >= n (0 for n <= 1)
inline int ceil_log2(int64_t n) {
    int b = 0;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}

// the smallest power of two >= n (1 for n <= 1)
inline int64_t pow2_at_least(int64_t n) { return (int64_t)1 << ceil_log2(n); }

[[maybe_unused]] static __global__ void k_iota(int32_t* a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (int32_t)i;
}

// ------------------------------------------------------------------ ordered keys, bounds
// Order-preserving float <-> uint32: a < b as floats iff ordered_u32(a) < ordered_u32(b), so integer
// atomicMin / atomicMax reduce float bounds (order-independent, hence bit-identical between runs).
__host__ __device__ inline uint32_t ordered_u32(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float from_ordered(uint32_t u) {
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// Min of lo[] / max of hi[] over a workgroup of 256 lanes into out6[0..2] / out6[3..5]: a wave butterfly,
// the four waves through LDS, then ONE atomic per word and workgroup.  Every lane calls it, once per kernel;
// the kernels that use it run a capped grid-stride grid, so the six words take at most 4096 atomics each.
// Per-wave atomics on the same six words serialise: they made the ray caster's triangle gather 44 ms for
// C5's 41 M triangles (profiles/r05_c5_kernel_stats.csv) and were the quality pass's vertex box's whole
// cost, 1.13 ms against 0.12 for C5's 20.6 M vertices.
__device__ inline void block_bounds_atomic(uint32_t (&lo)[3], uint32_t (&hi)[3], uint32_t* out6) {
    __shared__ uint32_t part[4][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        uint32_t l = lo[a], h = hi[a];
#pragma unroll
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
        if (c < 3) atomicMin(&out6[c], r);
        else atomicMax(&out6[c], r);
    }
}

// the low 21 bits of v, two zero bits between each: one axis of a 63-bit Morton key
__device__ inline uint64_t spread21(uint32_t v) {
    uint64_t x = v & 0x1fffff;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// ------------------------------------------------------------------ order-fixed slab reductions
// The workgroup's NS sums (pair_reduce.hpp: butterfly 32 -> 1, then ((w0 + w1) + w2) + w3), its min and its
// max into slab[0 .. NS + 2).  Every lane of the kThreads-lane workgroup calls it, once per kernel.
template <int NS>
__device__ inline void block_sums_minmax_to_slab(const double (&acc)[NS], double mn, double mx,
                                                 double* __restrict__ slab) {
    __shared__ double sh[pairsum::kWaves][NS];
    __shared__ double shm[pairsum::kWaves][2];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, off, 64));
        mx = fmax(mx, __shfl_xor(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6][0] = mn, shm[threadIdx.x >> 6][1] = mx;
    pairsum::block_sums_to_slab(acc, sh, slab);  // its barrier also covers shm
    const int j = (int)threadIdx.x - NS;
    if (j == 0) slab[NS] = fmin(fmin(shm[0][0], shm[1][0]), fmin(shm[2][0], shm[3][0]));
    else if (j == 1) slab[NS + 1] = fmax(fmax(shm[0][1], shm[1][1]), fmax(shm[2][1], shm[3][1]));
}

// One workgroup: lane l adds slabs l, l + kThreads, ... in that order, then the workgroup reduces as above.
template <int NS>
__global__ void __launch_bounds__(pairsum::kThreads) k_reduce_slabs(const double* __restrict__ slabs, int64_t nblk,
                                                                    double* __restrict__ out) {
    double acc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.0;
    double mn = INFINITY, mx = -INFINITY;
    for (int64_t b = threadIdx.x; b < nblk; b += pairsum::kThreads) {
        const double* s = slabs + b * (NS + 2);
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[j] += s[j];
        mn = fmin(mn, s[NS]);
        mx = fmax(mx, s[NS + 1]);
    }
    block_sums_minmax_to_slab(acc, mn, mx, out);
}

// ------------------------------------------------------------------ input checks
// Both only read the array they check and raise *flag (zeroed by the caller); nothing gathers through an
// index, or prunes on a coordinate, before the host has seen the flag.
[[maybe_unused]] static __global__ void k_check_indices(const int32_t* __restrict__ tri, int64_t n, int64_t nv,
                                                        int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (tri[i] < 0 || (int64_t)tri[i] >= nv)) *flag = 1;
}

// A value passes when |a| <= limit (a NaN fails the comparison): FLT_MAX asks for finite values.  Grid-stride:
// launch it on a capped grid.
[[maybe_unused]] static __global__ void k_check_finite(const float* __restrict__ a, int64_t n, float limit,
                                                       int32_t* flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        bad |= !(fabsf(a[i]) <= limit);
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) *flag = 1;
}

}  // namespace mqr
