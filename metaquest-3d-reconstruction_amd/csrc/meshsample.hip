// meshsample.hip -- area-weighted surface samples of a triangle mesh (TriangleMesh.sample_points_uniformly).
//
// Reference: reconstruct_scene.py:151-171 ends the colour stage with
// colored_mesh.sample_points_uniformly(int(vertex_count * ratio)).  Open3D draws from std::mt19937, which is
// neither matched nor pinned here; the rule is this package's own and is counter-based: sample i
// depends on (mesh, seed, i) alone -- not on n, the launch shape or an atomic's arrival order.
//   area_t   0.5 sqrt((x x + y y) + z z) of (b - a) x (c - a), float64 on the widened float32 corners;
//   w_t      floor(area_t 2^(32 - e)) with max area = m 2^e, m in [0.5, 1): integer weights below 2^32, so the
//            selection table (their inclusive uint64 prefix sum) is the same under any parallel scan;
//   r_j(i)   output 3 i + j + 1 of SplitMix64 seeded with `seed` (j = 0, 1, 2);
//   triangle the first k with cum[k] > mulhi64(r_0, total);
//   point    s = sqrt(u1), weights (1 - s, s (1 - u2), s u2) with u = (r >> 11) 2^-53, p = (wa a + wb b) + wc c.
// Passes: checks (device_prims.hpp, before anything gathers through an index), areas + their maximum, weights,
// the scan (hipcub), a coarse table of every kSeg-th prefix sum, then one thread per sample.  The file is built
// with -ffp-contract=off.  Scratch is one block of the device-block cache per call.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <mutex>
#include <string>

#include "device_block.hpp"
#include "device_cub.hpp"
#include "device_prims.hpp"
#include "mqr_common.hpp"

namespace mqr {
namespace ms {

constexpr int kT = 256;
constexpr int kSeg = 256;        // prefix sums per coarse-table entry
constexpr unsigned kGridCap = 2048;  // grid-stride kernels: 8 workgroups per CU

// Per-device timing events of the last call (mqr_mesh_sample_last_ms) and the search shape (a measurement hook).
struct SampleCtx {
    std::mutex mu;
    hipEvent_t ev[4] = {};  // call start, table start (checks read), table done, samples done
    bool timed = false;
};
static SampleCtx g_ctx[kMaxDevices];
static std::atomic<int> g_flat_search{0};  // read once per call

struct Ctrl {
    int32_t bad_index;
    int32_t bad_coord;
    unsigned long long amax_bits;  // the largest area's bit pattern (areas are non-negative: the patterns order)
};

__host__ __device__ inline uint64_t splitmix64(uint64_t seed, uint64_t k) {
    uint64_t z = seed + k * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Tri {
    double a[3], b[3], c[3];
};

__device__ inline Tri load_tri(const float* __restrict__ pos, const int32_t* __restrict__ tri, int64_t t) {
    const int64_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    Tri r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.a[k] = (double)pos[3 * i0 + k];
        r.b[k] = (double)pos[3 * i1 + k];
        r.c[k] = (double)pos[3 * i2 + k];
    }
    return r;
}

// (b - a) x (c - a), each product rounded on its own
__device__ inline void tri_cross(const Tri& q, double (&n)[3]) {
    const double u[3] = {q.b[0] - q.a[0], q.b[1] - q.a[1], q.b[2] - q.a[2]};
    const double w[3] = {q.c[0] - q.a[0], q.c[1] - q.a[1], q.c[2] - q.a[2]};
    n[0] = u[1] * w[2] - u[2] * w[1];
    n[1] = u[2] * w[0] - u[0] * w[2];
    n[2] = u[0] * w[1] - u[1] * w[0];
}

// PASS 1: area[t], and the maximum through one atomicMax per workgroup
__global__ void __launch_bounds__(kT) k_areas(const float* __restrict__ pos, const int32_t* __restrict__ tri, int64_t nt,
                                              double* __restrict__ area, Ctrl* ctrl) {
    __shared__ double part[kT / 64];
    double mx = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x; t < nt; t += (int64_t)gridDim.x * kT) {
        double n[3];
        tri_cross(load_tri(pos, tri, t), n);
        const double a = 0.5 * sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        area[t] = a;
        mx = fmax(mx, a);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = fmax(fmax(part[0], part[1]), fmax(part[2], part[3]));
        atomicMax(&ctrl->amax_bits, (unsigned long long)__double_as_longlong(mx));
    }
}

// PASS 2: w[t] = floor(area[t] 2^(32 - e)), max area = m 2^e (the scaling by a power of two is exact)
__global__ void __launch_bounds__(kT) k_weights(const double* __restrict__ area, int64_t nt, const Ctrl* __restrict__ ctrl,
                                                uint64_t* __restrict__ w) {
    int e = 0;
    (void)frexp(__longlong_as_double((long long)ctrl->amax_bits), &e);
    for (int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x; t < nt; t += (int64_t)gridDim.x * kT)
        w[t] = (uint64_t)floor(ldexp(area[t], 32 - e));
}

// coarse[j] = the last prefix sum of segment j
__global__ void __launch_bounds__(kT) k_coarse(const uint64_t* __restrict__ cum, int64_t nt, int64_t nseg,
                                               uint64_t* __restrict__ coarse) {
    const int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (j < nseg) coarse[j] = cum[min((j + 1) * kSeg, nt) - 1];
}

// the first index in [lo, hi) whose entry exceeds target (hi when none does)
__device__ inline int64_t first_above(const uint64_t* __restrict__ a, int64_t lo, int64_t hi, uint64_t target) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ inline void store3(float* __restrict__ out, int64_t i, double wa, double wb, double wc,
                              const float* __restrict__ src, const int32_t (&v)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = (double)src[3 * (int64_t)v[0] + k], b = (double)src[3 * (int64_t)v[1] + k],
                     c = (double)src[3 * (int64_t)v[2] + k];
        out[3 * i + k] = (float)((wa * a + wb * b) + wc * c);
    }
}

// PASS 4: one thread per sample, grid-stride.  FLAT searches the whole table; the default narrows to a
// segment on the coarse table (L2-resident: 8 bytes per 256 triangles) and finishes in that segment.
template <bool FLAT>
__global__ void __launch_bounds__(kT) k_sample(const float* __restrict__ pos, const float* __restrict__ nrm,
                                               const float* __restrict__ col, const int32_t* __restrict__ tri, int64_t nt,
                                               const uint64_t* __restrict__ cum, const uint64_t* __restrict__ coarse,
                                               int64_t nseg, int64_t n, uint64_t seed, int tri_normal,
                                               float* __restrict__ o_pos, float* __restrict__ o_nrm,
                                               float* __restrict__ o_col, int32_t* __restrict__ o_tri) {
    const uint64_t total = cum[nt - 1];
    if (total == 0) return;  // every triangle degenerate: the host reports it
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
        const uint64_t c0 = 3 * (uint64_t)i + 1;
        const uint64_t r0 = splitmix64(seed, c0), r1 = splitmix64(seed, c0 + 1), r2 = splitmix64(seed, c0 + 2);
        const uint64_t target = __umul64hi(r0, total);  // < total = cum[nt - 1]: the search ends inside the table
        int64_t k;
        if (FLAT) {
            k = first_above(cum, 0, nt, target);
        } else {
            const int64_t seg = min(first_above(coarse, 0, nseg, target), nseg - 1);
            k = first_above(cum, seg * kSeg, min((seg + 1) * kSeg, nt), target);
        }
        k = min(k, nt - 1);
        const double u1 = (double)(r1 >> 11) * 0x1p-53, u2 = (double)(r2 >> 11) * 0x1p-53;
        const double s = sqrt(u1);
        const double wa = 1.0 - s, wb = s * (1.0 - u2), wc = s * u2;
        const int32_t v[3] = {tri[3 * k], tri[3 * k + 1], tri[3 * k + 2]};
        store3(o_pos, i, wa, wb, wc, pos, v);
        if (o_nrm) {
            if (tri_normal) {
                double nn[3];
                tri_cross(load_tri(pos, tri, k), nn);
                const double len = sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
#pragma unroll
                for (int a = 0; a < 3; ++a) o_nrm[3 * i + a] = (float)(nn[a] / len);
            } else {
                store3(o_nrm, i, wa, wb, wc, nrm, v);
            }
        }
        if (o_col) store3(o_col, i, wa, wb, wc, col, v);
        if (o_tri) o_tri[i] = (int32_t)k;
    }
}

}  // namespace ms
}  // namespace mqr

using namespace mqr;
using namespace mqr::ms;

extern "C" {

int mqr_mesh_sample_points(int device, const float* vertices, int64_t nv, const float* normals, const float* colors,
                           const int32_t* triangles, int64_t nt, int in_loc, int64_t n, uint64_t seed,
                           int use_triangle_normal, float* out_positions, float* out_normals, float* out_colors,
                           int32_t* out_triangle, int out_loc) {
    MQR_REQUIRE(nt > 0, "mesh sample: the mesh has no triangles");
    MQR_REQUIRE(n >= 0, "mesh sample: the number of points is negative");
    MQR_REQUIRE(nv > 0, "mesh sample: the mesh has no vertices");
    MQR_REQUIRE(nt < ((int64_t)1 << 31) && nv < ((int64_t)1 << 31), "mesh sample: mesh too large (nt or nv >= 2^31)");
    MQR_REQUIRE((in_loc == MQR_HOST || in_loc == MQR_DEVICE) && (out_loc == MQR_HOST || out_loc == MQR_DEVICE),
                "mesh sample: in_loc and out_loc must be MQR_HOST or MQR_DEVICE");
    MQR_REQUIRE(vertices && triangles, "null argument");
    MQR_REQUIRE(device >= 0 && device < kMaxDevices, "device index out of range");
    if (n == 0) return 0;
    MQR_REQUIRE(out_positions, "null argument");
    MQR_REQUIRE(!out_normals || use_triangle_normal || normals,
                "mesh sample: normals are asked for, but the mesh has none and use_triangle_normal is off");
    MQR_REQUIRE(!out_colors || colors, "mesh sample: colours are asked for, but the mesh has none");
    MQR_CHECK_HIP(hipSetDevice(device));
    // the caller's stream when it is this device's (then nothing needs ordering), else the null stream
    // behind a host drain of the caller's; the module keeps no stream of its own
    hipStream_t s = copy_stream(device);
    if (caller_stream() && s != caller_stream()) MQR_CHECK_HIP(hipStreamSynchronize(caller_stream()));
    SampleCtx& ctx = g_ctx[device];
    std::lock_guard<std::mutex> lock(ctx.mu);
    for (hipEvent_t& e : ctx.ev)
        if (!e) MQR_CHECK_HIP(hipEventCreate(&e));
    ctx.timed = false;

    const bool host_in = in_loc == MQR_HOST, host_out = out_loc == MQR_HOST;
    const bool in_nrm = out_normals && !use_triangle_normal;  // the only reader of the vertex normals
    const int64_t nseg = (nt + kSeg - 1) / kSeg;
    const size_t b_v = sizeof(float) * 3 * nv, b_t = sizeof(int32_t) * 3 * nt, b_o = sizeof(float) * 3 * n;
    ScratchLayout L;
    float *d_v, *d_n, *d_c, *h_pos, *h_nrm, *h_col;
    int32_t *d_t, *h_tri;
    Ctrl* ctrl;
    uint64_t *w, *cum, *coarse;
    L.add(d_v, 3 * nv, host_in);
    L.add(d_t, 3 * nt, host_in);
    L.add(d_n, 3 * nv, host_in && in_nrm);
    L.add(d_c, 3 * nv, host_in && out_colors);
    L.add(h_pos, 3 * n, host_out);
    L.add(h_nrm, 3 * n, host_out && out_normals);
    L.add(h_col, 3 * n, host_out && out_colors);
    L.add(h_tri, n, host_out && out_triangle);
    L.add(ctrl, 1);
    L.add_each(nt, w, cum);
    L.add(coarse, nseg);
    auto scan_weights = [&](void* t, size_t& b) {
        return hipcub::DeviceScan::InclusiveSum(t, b, (const uint64_t*)w, cum, (int)nt, s);
    };
    CubTemp tmp;
    MQR_CHECK_HIP(tmp.lay_out(L, scan_weights));
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed("mesh sample", L.total());
    const float *pos = vertices, *nrm = in_nrm ? normals : nullptr, *col = out_colors ? colors : nullptr;
    const int32_t* tri = triangles;
    if (host_in) {
        if (copy_to_device(device, d_v, vertices, b_v, s) || copy_to_device(device, d_t, triangles, b_t, s) ||
            (d_n && copy_to_device(device, d_n, normals, b_v, s)) || (d_c && copy_to_device(device, d_c, colors, b_v, s)))
            return 1;
        pos = d_v, tri = d_t, nrm = d_n, col = d_c;
    }
    float *o_pos = out_positions, *o_nrm = out_normals, *o_col = out_colors;
    int32_t* o_tri = out_triangle;
    if (host_out) o_pos = h_pos, o_nrm = h_nrm, o_col = h_col, o_tri = h_tri;
    StreamDrain drain{s};

    // ---- checks: nothing gathers through an index before the flags are read
    MQR_CHECK_HIP(hipEventRecord(ctx.ev[0], s));
    MQR_CHECK_HIP(hipMemsetAsync(ctrl, 0, sizeof(Ctrl), s));
    hipLaunchKernelGGL(k_check_indices, dim3(nb(3 * nt)), dim3(kT), 0, s, tri, 3 * nt, nv, &ctrl->bad_index);
    hipLaunchKernelGGL(k_check_finite, dim3(std::min<unsigned>(nb(3 * nv), 4096)), dim3(kT), 0, s, pos, 3 * nv, FLT_MAX,
                       &ctrl->bad_coord);
    MQR_CHECK_HIP(hipGetLastError());
    Ctrl hc;
    MQR_CHECK_HIP(hipMemcpyAsync(&hc, ctrl, sizeof hc, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    MQR_REQUIRE(!hc.bad_index, "mesh sample: a triangle index is outside [0, nv)");
    MQR_REQUIRE(!hc.bad_coord, "mesh sample: a vertex coordinate is not finite");

    // ---- the selection table (the areas pass through `cum`, which the scan then overwrites)
    MQR_CHECK_HIP(hipEventRecord(ctx.ev[1], s));
    const unsigned gt = std::min<unsigned>(nb(nt), kGridCap);
    double* area = (double*)cum;
    hipLaunchKernelGGL(k_areas, dim3(gt), dim3(kT), 0, s, pos, tri, nt, area, ctrl);
    hipLaunchKernelGGL(k_weights, dim3(gt), dim3(kT), 0, s, (const double*)area, nt, (const Ctrl*)ctrl, w);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(tmp.run(scan_weights));
    hipLaunchKernelGGL(k_coarse, dim3(nb(nseg)), dim3(kT), 0, s, (const uint64_t*)cum, nt, nseg, coarse);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(hipEventRecord(ctx.ev[2], s));

    // ---- the samples (the kernel returns at once when the total is zero; the host reads it below)
    const unsigned gs = std::min<unsigned>(nb(n), kGridCap);
    if (g_flat_search.load(std::memory_order_relaxed))
        hipLaunchKernelGGL(k_sample<true>, dim3(gs), dim3(kT), 0, s, pos, nrm, col, tri, nt, (const uint64_t*)cum,
                           (const uint64_t*)coarse, nseg, n, seed, use_triangle_normal, o_pos, o_nrm, o_col, o_tri);
    else
        hipLaunchKernelGGL(k_sample<false>, dim3(gs), dim3(kT), 0, s, pos, nrm, col, tri, nt, (const uint64_t*)cum,
                           (const uint64_t*)coarse, nseg, n, seed, use_triangle_normal, o_pos, o_nrm, o_col, o_tri);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(hipEventRecord(ctx.ev[3], s));
    uint64_t total = 0;
    MQR_CHECK_HIP(hipMemcpyAsync(&total, cum + (nt - 1), sizeof total, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    MQR_REQUIRE(total != 0, "mesh sample: every triangle is degenerate (the total area weight is zero)");
    ctx.timed = true;
    if (host_out) {
        if (copy_to_host(device, out_positions, o_pos, b_o, s)) return 1;
        if (out_normals && copy_to_host(device, out_normals, o_nrm, b_o, s)) return 1;
        if (out_colors && copy_to_host(device, out_colors, o_col, b_o, s)) return 1;
        if (out_triangle && copy_to_host(device, out_triangle, o_tri, sizeof(int32_t) * n, s)) return 1;
    }
    return 0;
}

int mqr_mesh_sample_last_ms(int device, float* call_ms, float* table_ms, float* sample_ms) {
    MQR_REQUIRE(call_ms && table_ms && sample_ms, "null argument");
    MQR_REQUIRE(device >= 0 && device < kMaxDevices, "device index out of range");
    SampleCtx& ctx = g_ctx[device];
    std::lock_guard<std::mutex> lock(ctx.mu);
    MQR_REQUIRE(ctx.timed, "no completed mqr_mesh_sample_points call on this device");
    MQR_CHECK_HIP(hipEventElapsedTime(call_ms, ctx.ev[0], ctx.ev[3]));
    MQR_CHECK_HIP(hipEventElapsedTime(table_ms, ctx.ev[1], ctx.ev[2]));
    MQR_CHECK_HIP(hipEventElapsedTime(sample_ms, ctx.ev[2], ctx.ev[3]));
    return 0;
}

int mqr_mesh_sample_set_flat_search(int flat) {
    g_flat_search.store(flat ? 1 : 0, std::memory_order_relaxed);
    return 0;
}

}  // extern "C"
