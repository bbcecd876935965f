// Order-fixed float64 reductions of the batched pair kernels (registration.hip, odometry.hip).
//
// A workgroup of kThreads lanes reduces NS per-lane sums with a fixed butterfly over the lanes of
// each wave, then the four waves in order through LDS, and writes one slab of NS partials; a
// per-pair kernel sums a pair's slabs in workgroup order.  No float atomics anywhere, so a repeated
// call -- and a pair computed alone or inside a batch -- gives bit-identical sums.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mqr {
namespace pairsum {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kInfoSums = 22;  // count, 21 unique entries of sum G^T G (upper triangle, row by row)

// The workgroup's sums of acc[0..NS) into slab[0..NS).  Every lane of the workgroup calls it.
template <int NS>
__device__ inline void block_sums_to_slab(const double (&acc)[NS], double (&sh)[kWaves][NS], double* __restrict__ slab) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double v = acc[j];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) sh[wave][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int j = threadIdx.x;
        slab[j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
    }
}

// G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]]: the kInfoSums sums of `count`
// points from their coordinate sums (s*) and second moments (upper triangle of G^T G row by row).
__device__ inline void info_sums(double count, double sx, double sy, double sz, double xx, double yy, double zz,
                                 double xy, double xz, double yz, double (&acc)[kInfoSums]) {
    acc[0] = count;
    acc[1] = zz + yy, acc[2] = -xy, acc[3] = -xz;
    acc[4] = 0.0, acc[5] = -sz, acc[6] = sy;
    acc[7] = zz + xx, acc[8] = -yz, acc[9] = sz, acc[10] = 0.0, acc[11] = -sx;
    acc[12] = yy + xx, acc[13] = -sy, acc[14] = sx, acc[15] = 0.0;
    acc[16] = count, acc[17] = 0.0, acc[18] = 0.0;
    acc[19] = count, acc[20] = 0.0;
    acc[21] = count;
}

// One workgroup (>= 36 lanes) per pair: the pair's nblk slabs from slab_off on, summed in workgroup
// order into S (LDS; S[0] is the count afterwards), and the 21 sums spread over the symmetric 6x6.
__device__ inline void info_from_slabs(const double* __restrict__ slabs, int64_t slab_off, int nblk,
                                       double (&S)[kInfoSums], double* __restrict__ info36) {
    if (threadIdx.x < kInfoSums) {
        double v = 0.0;
        for (int b = 0; b < nblk; ++b) v += slabs[(slab_off + b) * kInfoSums + threadIdx.x];
        S[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x >= 36) return;
    const int a = threadIdx.x / 6, b = threadIdx.x % 6;
    const int r = a < b ? a : b, c = a < b ? b : a;
    info36[threadIdx.x] = S[1 + r * 6 - r * (r - 1) / 2 + (c - r)];
}

}  // namespace pairsum
}  // namespace mqr
