// odometry.hip -- batched odometry information matrices (DESIGN §2 row `odometry`).
//
// Reference: make_fragments.py:106-240 calls o3d.t.pipelines.odometry.compute_odometry_information_matrix
// once per image pair of a fragment (99 odometry pairs and up to 45 key-frame pairs of two VGA depth
// maps each).  Here the fragment's N decoded frames sit in HBM once and every pair of the fragment
// runs in ONE launch, grid = (pixel tiles, pairs), the way registration.hip uses (blocks, pairs).
//
// Everything that decides a result is float64, computed from the float32 depth and the float64 K and
// T (DESIGN "odometry information rules"):
//   validity     d = depth / depth_scale; valid iff 0 < d <= depth_max and d finite
//   source       s = d ((x - cx) / fx, (y - cy) / fy, 1);  q = R s + t;  rejected if q.z <= 0
//   projection   u = fx q.x / q.z + cx, v = fy q.y / q.z + cy, rounded half away from zero; rejected
//                unless 0 <= u < W and 0 <= v < H (tested in float64, so a NaN or a huge value never
//                becomes an index)
//   target       g = the target depth at (u, v), valid by the same rule, unprojected the same way;
//                accepted iff |g - q|^2 <= dist_threshold^2
//   sums         the count and G^T G of g (pair_reduce.hpp); each lane sums its kPix pixels in pixel
//                order, the workgroup and the per-pair kernel reduce in a fixed order.  No float atomics.
// The source frame is a coalesced stream (lane l of pass k reads pixel tile * kTile + k * 256 + l); the
// target read is a gather that stays near the source pixel for small motions.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "device_block.hpp"
#include "mqr_common.hpp"
#include "pair_reduce.hpp"

namespace mqr {
namespace odo {

using pairsum::kInfoSums;
using pairsum::kThreads;
using pairsum::kWaves;
constexpr int kPix = 4;                   // pixels per lane
constexpr int kTile = kThreads * kPix;    // pixels per workgroup
constexpr int kMaxPairs = 65535;          // grid.y

struct Pair {
    double T[12];  // source camera -> target camera, rows of [R | t]
    int32_t src, tgt;
};

struct Params {
    double fx, fy, cx, cy;
    double thr2, depth_scale, depth_max;
    int32_t H, W;
};

__device__ inline bool metric_depth(float raw, const Params& P, double& d) {
    d = (double)raw / P.depth_scale;
    return d > 0.0 && d <= P.depth_max && fabs(d) <= 1.7976931348623157e308;
}

__global__ __launch_bounds__(kThreads) void k_odometry_info(const float* __restrict__ depths,
                                                           const Pair* __restrict__ pairs, Params P,
                                                           double* __restrict__ slabs) {
    __shared__ double sh[kWaves][kInfoSums];
    const Pair& pr = pairs[blockIdx.y];
    const uint32_t HW = (uint32_t)P.H * (uint32_t)P.W, W = (uint32_t)P.W;  // the host requires H * W < 2^31
    const float* __restrict__ src = depths + (int64_t)pr.src * HW;
    const float* __restrict__ tgt = depths + (int64_t)pr.tgt * HW;
    const double* T = pr.T;
    double n = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, xx = 0.0, yy = 0.0, zz = 0.0, xy = 0.0, xz = 0.0, yz = 0.0;
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        const uint32_t i = blockIdx.x * (uint32_t)kTile + (uint32_t)(k * kThreads) + threadIdx.x;  // < HW + kTile < 2^32
        if (i >= HW) continue;
        const uint32_t y = i / W, x = i - y * W;
        double d;
        if (!metric_depth(src[i], P, d)) continue;
        const double px = d * (((double)x - P.cx) / P.fx), py = d * (((double)y - P.cy) / P.fy), pz = d;
        const double qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
        const double qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
        const double qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
        if (!(qz > 0.0)) continue;
        const double u = round((P.fx * qx) / qz + P.cx), v = round((P.fy * qy) / qz + P.cy);
        if (!(u >= 0.0 && u < (double)P.W && v >= 0.0 && v < (double)P.H)) continue;  // NaN fails too
        const int ui = (int)u, vi = (int)v;
        double dt;
        if (!metric_depth(tgt[(uint32_t)vi * W + (uint32_t)ui], P, dt)) continue;
        const double gx = dt * ((u - P.cx) / P.fx), gy = dt * ((v - P.cy) / P.fy), gz = dt;
        const double ex = gx - qx, ey = gy - qy, ez = gz - qz;
        if (!((ex * ex + ey * ey) + ez * ez <= P.thr2)) continue;
        n += 1.0;
        sx += gx, sy += gy, sz += gz;
        xx += gx * gx, yy += gy * gy, zz += gz * gz;
        xy += gx * gy, xz += gx * gz, yz += gy * gz;
    }
    double acc[kInfoSums];
    pairsum::info_sums(n, sx, sy, sz, xx, yy, zz, xy, xz, yz, acc);
    pairsum::block_sums_to_slab<kInfoSums>(acc, sh, slabs + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kInfoSums);
}

// one workgroup per pair: its slabs in workgroup order, the symmetric 6x6 and the count
__global__ __launch_bounds__(64) void k_odometry_finalize(const double* __restrict__ slabs, int nblk,
                                                          double* __restrict__ info, int64_t* __restrict__ counts) {
    __shared__ double S[kInfoSums];
    const int pair = blockIdx.x;
    pairsum::info_from_slabs(slabs, (int64_t)pair * nblk, nblk, S, info + 36 * (int64_t)pair);
    if (threadIdx.x == 0) counts[pair] = (int64_t)S[0];
}

// grow-only device scratch per device (GrowBuf), kept between calls for the life of the process: 0 host
// frames (a copy of the whole stack), 1 pairs, 2 slabs, 3 outputs
struct Cache {
    std::mutex mu;
    GrowBuf buf[4];

    void* get(int slot, size_t bytes) {  // nullptr when the device is out of memory
        (void)buf[slot].reserve(bytes, std::max<size_t>(bytes + bytes / 2, 4096));
        return buf[slot].p;
    }
};
Cache g_cache[kMaxDevices];

}  // namespace odo
}  // namespace mqr

using namespace mqr;
using namespace mqr::odo;

extern "C" int mqr_odometry_information_pairs(int device, const float* depths, int depth_loc, int N, int H, int W,
                                              const double* K, int n_pairs, const int32_t* src, const int32_t* tgt,
                                              const double* T, double dist_threshold, double depth_scale,
                                              double depth_max, double* info, int64_t* counts) {
    MQR_REQUIRE(n_pairs >= 0 && n_pairs <= kMaxPairs, "n_pairs must be in [0, 65535]");
    if (n_pairs == 0) return 0;
    MQR_REQUIRE(depths && K && src && tgt && T && info, "null argument");
    MQR_REQUIRE(depth_loc == MQR_HOST || depth_loc == MQR_DEVICE, "depth_loc must be MQR_HOST or MQR_DEVICE");
    MQR_REQUIRE(N > 0 && H > 0 && W > 0, "bad shape");
    MQR_REQUIRE(device >= 0 && device < kMaxDevices, "bad device");
    const int64_t HW = (int64_t)H * W;
    MQR_REQUIRE(HW < ((int64_t)1 << 31), "frame too large");
    for (int a = 0; a < 9; ++a) MQR_REQUIRE(std::isfinite(K[a]), "non-finite intrinsic matrix");
    MQR_REQUIRE(std::isfinite(dist_threshold) && std::isfinite(depth_scale) && depth_scale != 0.0 &&
                    !std::isnan(depth_max),
                "dist_threshold and depth_scale must be finite (depth_scale non-zero), depth_max not NaN");
    std::vector<Pair> hp((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        MQR_REQUIRE(src[p] >= 0 && src[p] < N && tgt[p] >= 0 && tgt[p] < N, "frame index out of range");
        for (int a = 0; a < 16; ++a) MQR_REQUIRE(std::isfinite(T[16 * (size_t)p + a]), "non-finite transformation");
        std::memcpy(hp[(size_t)p].T, T + 16 * (size_t)p, sizeof(double) * 12);
        hp[(size_t)p].src = src[p];
        hp[(size_t)p].tgt = tgt[p];
    }
    MQR_CHECK_HIP(hipSetDevice(device));
    const int nblk = (int)((HW + kTile - 1) / kTile);
    Cache& c = g_cache[device];
    std::lock_guard<std::mutex> lock(c.mu);
    // the caller's stream when it is this device's (then nothing needs ordering), else the null stream
    // behind a host drain of the caller's
    hipStream_t s = copy_stream(device);
    if (caller_stream() && s != caller_stream()) MQR_CHECK_HIP(hipStreamSynchronize(caller_stream()));
    const float* d_depths = depths;
    if (depth_loc == MQR_HOST) {
        const size_t bytes = sizeof(float) * (size_t)N * (size_t)HW;
        void* d = c.get(0, bytes);
        MQR_REQUIRE(d, "odometry: device allocation failed");
        if (copy_to_device(device, d, depths, bytes, s)) return 1;
        d_depths = static_cast<const float*>(d);
    }
    Pair* d_pairs = static_cast<Pair*>(c.get(1, sizeof(Pair) * (size_t)n_pairs));
    double* d_slabs = static_cast<double*>(c.get(2, sizeof(double) * kInfoSums * (size_t)n_pairs * (size_t)nblk));
    const size_t info_bytes = sizeof(double) * 36 * (size_t)n_pairs;
    ScratchLayout L;  // the outputs
    double* d_info;
    int64_t* d_counts;
    L.add(d_info, 36 * (int64_t)n_pairs);
    L.add(d_counts, n_pairs);
    void* d_out = c.get(3, L.total());
    MQR_REQUIRE(d_pairs && d_slabs && d_out, "odometry: device allocation failed");
    L.bind(d_out);
    MQR_CHECK_HIP(hipMemcpyAsync(d_pairs, hp.data(), sizeof(Pair) * (size_t)n_pairs, hipMemcpyHostToDevice, s));
    Params P;
    P.fx = K[0], P.fy = K[4], P.cx = K[2], P.cy = K[5];
    P.thr2 = dist_threshold * dist_threshold;
    P.depth_scale = depth_scale;
    P.depth_max = depth_max;
    P.H = H, P.W = W;
    hipLaunchKernelGGL(k_odometry_info, dim3((unsigned)nblk, (unsigned)n_pairs), dim3(kThreads), 0, s, d_depths,
                       d_pairs, P, d_slabs);
    hipLaunchKernelGGL(k_odometry_finalize, dim3((unsigned)n_pairs), dim3(64), 0, s, d_slabs, nblk, d_info, d_counts);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(hipMemcpyAsync(info, d_info, info_bytes, hipMemcpyDeviceToHost, s));
    if (counts) MQR_CHECK_HIP(hipMemcpyAsync(counts, d_counts, sizeof(int64_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));  // `hp` is pageable host memory; the outputs are filled
    return 0;
}
