// colormap.hip -- rigid colour-map optimisation: batched keyframe pose refinement.
//
// The reference hands its mesh, colour keyframes and their colour-aligned depth to Open3D's
// run_rigid_optimizer (optimize_color_pose.py:70-73), which refines every keyframe pose against a
// per-vertex proxy intensity on CPU threads, one keyframe per thread.  Here the whole loop is device
// resident: the handle (mqr_colormap) holds the vertices, the keyframes' utility images, both visibility
// lists and the poses in HBM, and one iteration is three launches with no host read in between:
//   k_cmo_systems  a workgroup per 256-term chunk of one keyframe's image->vertex list: the photometric
//                  residual and 6-vector Jacobian of each term in float64, 29 sums per chunk written as
//                  one slab (pair_reduce.hpp; no float atomics)
//   k_cmo_solve    a workgroup per keyframe: its slabs in chunk order, the 6x6 LDL^T solve and the pose
//                  update in one lane, r2 and the count into the iteration's record
//   k_cmo_proxy    a thread per vertex over its vertex->image list: the mean nearest-pixel intensity
// The rules (utility images, visibility, terms, the kept-pose rule) are DESIGN §2.4's, restated from
// Open3D 0.19 RigidOptimizer.cpp / ColorMapUtils.cpp as recalled -- VERIFY.
//
// Utility images: grey, d/dx and d/dy interleaved as one float4 per pixel (gray, dx, dy, 0), so the four
// bilinear taps of a term are four 16-byte loads instead of twelve 4-byte ones.
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "mqr_common.hpp"
#include "device_block.hpp"
#include "device_cub.hpp"
#include "color_shared.hpp"
#include "pair_reduce.hpp"

namespace mqr {
namespace cmo {

using pairsum::kThreads;
using pairsum::kWaves;
constexpr int kSums = 29;  // count, r2, JTr (6), upper triangle of JTJ row by row (21)
constexpr int kMaxKeyframes = 65535;  // grid.y of the visibility kernels

struct Params {
    double max_depth, vis_thr;
    float depth_trunc;
    int32_t margin, N, H, W;
    int64_t nv;
};

struct Chunk {
    int64_t off;  // first entry of the chunk in the image->vertex list
    int32_t c;    // its keyframe
    int32_t pad;
};

// float (u, v, d) of a float64 projection, as k_cm_vertices computes them
__device__ inline void project_f(const ColorCam& cm, double X, double Y, double Z, float& u, float& v, float& d) {
    const double vx = cm.E[0] * X + cm.E[1] * Y + cm.E[2] * Z + cm.E[3];
    const double vy = cm.E[4] * X + cm.E[5] * Y + cm.E[6] * Z + cm.E[7];
    const double vz = cm.E[8] * X + cm.E[9] * Y + cm.E[10] * Z + cm.E[11];
    u = (float)((vx * cm.fx) / vz + cm.cx);
    v = (float)((vy * cm.fy) / vz + cm.cy);
    d = (float)vz;
}

// the rounded pixel of (u, v) when it lies inside the image (tested on the floats: NaN and huge values
// never become an index)
__device__ inline bool rounded_pixel(float u, float v, int H, int W, int& ui, int& vi) {
    const float ru = roundf(u), rv = roundf(v);
    if (!(ru >= 0.0f && ru < (float)W && rv >= 0.0f && rv < (float)H)) return false;
    ui = (int)ru;
    vi = (int)rv;
    return true;
}

__device__ inline bool in_margin(float u, float v, int H, int W, int margin) {
    return u >= margin && u < W - margin && v >= margin && v < H - margin;
}

// k_cm_vertices' visibility rule without its margin test
__device__ inline bool visible(const ColorCam& cm, const float* __restrict__ V, int64_t i, const float* __restrict__ t_hit,
                               const uint8_t* __restrict__ mask, int c, const Params& P) {
    float u, v, d;
    project_f(cm, V[3 * i], V[3 * i + 1], V[3 * i + 2], u, v, d);
    int ui, vi;
    if (!(d >= 0.0f) || !rounded_pixel(u, v, P.H, P.W, ui, vi)) return false;
    const int64_t px = (int64_t)c * P.H * P.W + (int64_t)vi * P.W + ui;
    const float th = t_hit[px] / 1.0f;
    const float ds = th >= P.depth_trunc ? 0.0f : th;
    if (ds > P.max_depth) return false;
    if (mask[px] == 255) return false;
    return (double)fabsf(d - ds) < P.vis_thr;
}

// ------------------------------------------------------------------ utility images
__device__ inline float grey_of(const uint8_t* __restrict__ p) {
    return (0.2990f * (float)p[0] + 0.5870f * (float)p[1] + 0.1140f * (float)p[2]) / 255.0f;
}

// Gaussian3 along x of the grey image -> plane a
__global__ void k_cmo_gray_h(const uint8_t* __restrict__ images, int64_t total, int W, float* __restrict__ a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const int64_t row = i - x;
    const float k[3] = {0.25f, 0.5f, 0.25f};
    double s = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int xs = min(max(x + t - 1, 0), W - 1);
        s += (double)(grey_of(images + 3 * (row + xs)) * k[t]);
    }
    a[i] = (float)s;
}

// Gaussian3 along y of plane a -> util[i].x (gray)
__global__ void k_cmo_gray_v(const float* __restrict__ a, int64_t total, int H, int W, float* __restrict__ util) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t HW = (int64_t)H * W, f = i / HW;
    const int p = (int)(i - f * HW), y = p / W, x = p % W;
    const float k[3] = {0.25f, 0.5f, 0.25f};
    double s = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int ys = min(max(y + t - 1, 0), H - 1);
        s += (double)(a[f * HW + (int64_t)ys * W + x] * k[t]);
    }
    util[4 * i] = (float)s;
}

// horizontal passes of both Sobel filters from gray: a = {-1, 0, 1} along x, b = {1, 2, 1} along x
__global__ void k_cmo_sobel_h(const float* __restrict__ util, int64_t total, int W, float* __restrict__ a,
                              float* __restrict__ b) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const int64_t row = i - x;
    float g[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) g[t] = util[4 * (row + min(max(x + t - 1, 0), W - 1))];
    double sa = 0, sb = 0;
    sa += (double)(g[0] * -1.0f);
    sa += (double)(g[1] * 0.0f);
    sa += (double)(g[2] * 1.0f);
    sb += (double)(g[0] * 1.0f);
    sb += (double)(g[1] * 2.0f);
    sb += (double)(g[2] * 1.0f);
    a[i] = (float)sa;
    b[i] = (float)sb;
}

// vertical passes: dx = {1, 2, 1} along y of a, dy = {-1, 0, 1} along y of b -> util[i].yzw = (dx, dy, 0)
__global__ void k_cmo_sobel_v(const float* __restrict__ a, const float* __restrict__ b, int64_t total, int H, int W,
                              float* __restrict__ util) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t HW = (int64_t)H * W, f = i / HW;
    const int p = (int)(i - f * HW), y = p / W, x = p % W;
    const float ka[3] = {1.0f, 2.0f, 1.0f}, kb[3] = {-1.0f, 0.0f, 1.0f};
    double sa = 0, sb = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int ys = min(max(y + t - 1, 0), H - 1);
        const int64_t q = f * HW + (int64_t)ys * W + x;
        sa += (double)(a[q] * ka[t]);
        sb += (double)(b[q] * kb[t]);
    }
    util[4 * i + 1] = (float)sa;
    util[4 * i + 2] = (float)sb;
    util[4 * i + 3] = 0.0f;
}

// ------------------------------------------------------------------ visibility lists
// image -> vertex: grid (vertex blocks, keyframes).  Count per (keyframe, block), scan, emit in vertex
// order -- so a keyframe's list is ascending and every sum over it has one order.
__global__ __launch_bounds__(kThreads) void k_cmo_vis_block_count(const float* __restrict__ V,
                                                                 const float* __restrict__ t_hit,
                                                                 const uint8_t* __restrict__ mask,
                                                                 const ColorCam* __restrict__ cams, Params P,
                                                                 int64_t* __restrict__ bcnt) {
    const int c = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool vis = i < P.nv && visible(cams[c], V, i, t_hit, mask, c, P);
    const int n = __syncthreads_count(vis);
    if (threadIdx.x == 0) bcnt[(int64_t)c * gridDim.x + blockIdx.x] = n;
}

__global__ __launch_bounds__(kThreads) void k_cmo_vis_block_emit(const float* __restrict__ V,
                                                                const float* __restrict__ t_hit,
                                                                const uint8_t* __restrict__ mask,
                                                                const ColorCam* __restrict__ cams, Params P,
                                                                const int64_t* __restrict__ boff,
                                                                int32_t* __restrict__ i2v) {
    __shared__ int wcnt[kWaves];
    const int c = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool vis = i < P.nv && visible(cams[c], V, i, t_hit, mask, c, P);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(vis);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (!vis) return;
    int64_t at = boff[(int64_t)c * gridDim.x + blockIdx.x];
    for (int w = 0; w < wave; ++w) at += wcnt[w];
    at += __popcll(m & ((uint64_t{1} << lane) - 1));
    i2v[at] = (int32_t)i;
}

// vertex -> image: a thread per vertex, keyframes in ascending order
__global__ __launch_bounds__(kThreads) void k_cmo_vis_vertex_count(const float* __restrict__ V,
                                                                  const float* __restrict__ t_hit,
                                                                  const uint8_t* __restrict__ mask,
                                                                  const ColorCam* __restrict__ cams, Params P,
                                                                  int64_t* __restrict__ vcnt) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P.nv) return;
    int64_t n = 0;
    for (int c = 0; c < P.N; ++c) n += visible(cams[c], V, i, t_hit, mask, c, P) ? 1 : 0;
    vcnt[i] = n;
}

__global__ __launch_bounds__(kThreads) void k_cmo_vis_vertex_emit(const float* __restrict__ V,
                                                                 const float* __restrict__ t_hit,
                                                                 const uint8_t* __restrict__ mask,
                                                                 const ColorCam* __restrict__ cams, Params P,
                                                                 const int64_t* __restrict__ voff,
                                                                 int32_t* __restrict__ v2i) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P.nv) return;
    int64_t at = voff[i];
    for (int c = 0; c < P.N; ++c)
        if (visible(cams[c], V, i, t_hit, mask, c, P)) v2i[at++] = c;
}

// per-keyframe list offsets (N + 1) from the block offsets, and the chunk table
__global__ void k_cmo_kf_offsets(const int64_t* __restrict__ boff, int N, int64_t nvb, int64_t* __restrict__ kf_off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c <= N) kf_off[c] = boff[(int64_t)c * nvb];
}

__global__ void k_cmo_chunk_starts(const int64_t* __restrict__ kf_off, int N, int64_t* __restrict__ chunk_start) {
    if (blockIdx.x || threadIdx.x) return;
    int64_t at = 0;
    for (int c = 0; c < N; ++c) {
        chunk_start[c] = at;
        at += (kf_off[c + 1] - kf_off[c] + kThreads - 1) / kThreads;
    }
    chunk_start[N] = at;
}

__global__ void k_cmo_chunk_table(const int64_t* __restrict__ kf_off, const int64_t* __restrict__ chunk_start,
                                  Chunk* __restrict__ chunks) {
    const int c = blockIdx.x;
    const int64_t first = chunk_start[c], n = chunk_start[c + 1] - first;
    for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
        Chunk ch;
        ch.off = kf_off[c] + k * kThreads;
        ch.c = c;
        ch.pad = 0;
        chunks[first + k] = ch;
    }
}

// ------------------------------------------------------------------ proxy intensities
__global__ __launch_bounds__(kThreads) void k_cmo_proxy(const float* __restrict__ V, const int32_t* __restrict__ v2i,
                                                       const int64_t* __restrict__ voff,
                                                       const ColorCam* __restrict__ cams,
                                                       const float4* __restrict__ util, Params P,
                                                       double* __restrict__ proxy) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P.nv) return;
    const double X = V[3 * i], Y = V[3 * i + 1], Z = V[3 * i + 2];
    const int64_t HW = (int64_t)P.H * P.W;
    double sum = 0.0;
    int cnt = 0;
    for (int64_t e = voff[i]; e < voff[i + 1]; ++e) {
        const int c = v2i[e];
        float u, v, d;
        project_f(cams[c], X, Y, Z, u, v, d);
        int ui, vi;
        if (!in_margin(u, v, P.H, P.W, P.margin) || !rounded_pixel(u, v, P.H, P.W, ui, vi)) continue;
        sum += (double)util[c * HW + (int64_t)vi * P.W + ui].x;
        ++cnt;
    }
    proxy[i] = cnt ? sum / cnt : 0.0;
}

// ------------------------------------------------------------------ the systems
__global__ __launch_bounds__(kThreads) void k_cmo_systems(const float* __restrict__ V, const int32_t* __restrict__ i2v,
                                                         const int64_t* __restrict__ kf_off,
                                                         const Chunk* __restrict__ chunks,
                                                         const ColorCam* __restrict__ cams,
                                                         const float4* __restrict__ util,
                                                         const double* __restrict__ proxy, Params P,
                                                         double* __restrict__ slabs) {
    __shared__ double sh[kWaves][kSums];
    const Chunk ch = chunks[blockIdx.x];
    const ColorCam& cm = cams[ch.c];
    const int64_t e = ch.off + threadIdx.x;
    double acc[kSums];
#pragma unroll
    for (int j = 0; j < kSums; ++j) acc[j] = 0.0;
    if (e < kf_off[ch.c + 1]) {
        const int64_t i = i2v[e];
        const double X = V[3 * i], Y = V[3 * i + 1], Z = V[3 * i + 2];
        const double gx = cm.E[0] * X + cm.E[1] * Y + cm.E[2] * Z + cm.E[3];
        const double gy = cm.E[4] * X + cm.E[5] * Y + cm.E[6] * Z + cm.E[7];
        const double gz = cm.E[8] * X + cm.E[9] * Y + cm.E[10] * Z + cm.E[11];
        const double u = (gx * cm.fx) / gz + cm.cx, v = (gy * cm.fy) / gz + cm.cy;
        const int W = P.W, H = P.H;
        // the margin test and FloatValueAt's validity, both false for NaN
        if (u >= (double)P.margin && u < (double)(W - P.margin) && v >= (double)P.margin &&
            v < (double)(H - P.margin) && u >= 0.0 && u <= (double)(W - 1) && v >= 0.0 && v <= (double)(H - 1)) {
            const int ui = min(max((int)u, 0), W - 2), vi = min(max((int)v, 0), H - 2);
            const double pu = u - ui, pv = v - vi;
            const float4* __restrict__ p = util + ((int64_t)ch.c * H + vi) * W + ui;
            const float4 a00 = p[0], a10 = p[1], a01 = p[W], a11 = p[W + 1];
            auto lerp = [&](float f00, float f01, float f10, float f11) {
                return ((double)f00 * (1.0 - pv) + (double)f01 * pv) * (1.0 - pu) +
                       ((double)f10 * (1.0 - pv) + (double)f11 * pv) * pu;
            };
            const double gray = lerp(a00.x, a01.x, a10.x, a11.x);
            const double dIdx = lerp(a00.y, a01.y, a10.y, a11.y);
            const double dIdy = lerp(a00.z, a01.z, a10.z, a11.z);
            const double invz = 1.0 / gz;
            const double v0 = dIdx * cm.fx * invz, v1 = dIdy * cm.fy * invz;
            const double v2 = -(v0 * gx + v1 * gy) * invz;
            double J[6];
            J[0] = -gz * v1 + gy * v2;
            J[1] = gz * v0 - gx * v2;
            J[2] = -gy * v0 + gx * v1;
            J[3] = v0;
            J[4] = v1;
            J[5] = v2;
            const double r = gray - proxy[i];
            acc[0] = 1.0;
            acc[1] = r * r;
            int k = 8;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                acc[2 + a] = J[a] * r;
#pragma unroll
                for (int b = a; b < 6; ++b) acc[k++] = J[a] * J[b];
            }
        }
    }
    pairsum::block_sums_to_slab<kSums>(acc, sh, slabs + (int64_t)blockIdx.x * kSums);
}

// One workgroup per keyframe: its slabs in chunk order into sys[c][29]; then (update) the LDL^T solve of
// JTJ x = -JTr and E <- delta(x) E in lane 0, and (r2, count) into rec[c].  The keyframe keeps its pose
// when count < 6, a pivot is non-positive or non-finite, or x is non-finite.
__global__ __launch_bounds__(64) void k_cmo_solve(const double* __restrict__ slabs,
                                                  const int64_t* __restrict__ chunk_start, ColorCam* __restrict__ cams,
                                                  double* __restrict__ sys, double* __restrict__ rec, int update) {
    __shared__ double S[kSums];
    const int c = blockIdx.x;
    if (threadIdx.x < kSums) {
        // chunk order, one running sum; the loads of 8 slabs are issued together (a load per add made the
        // loop one memory latency per chunk: 377 us for C5's up to 1480 chunks per keyframe)
        double v = 0.0;
        const int64_t b1 = chunk_start[c + 1];
        int64_t b = chunk_start[c];
        for (; b + 8 <= b1; b += 8) {
            double t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = slabs[(b + k) * kSums + threadIdx.x];
#pragma unroll
            for (int k = 0; k < 8; ++k) v += t[k];
        }
        for (; b < b1; ++b) v += slabs[b * kSums + threadIdx.x];
        S[threadIdx.x] = v;
        sys[(int64_t)c * kSums + threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0 || !update) return;
    rec[2 * c] = S[1];
    rec[2 * c + 1] = S[0];
    if (S[0] < 6.0) return;
    double A[6][6], L[6][6], D[6], x[6];
    {
        int k = 8;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) {
                A[a][b] = S[k];
                A[b][a] = S[k];
                ++k;
            }
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
        D[j] = d;
        if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) ok = false;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k] * D[k];
            L[i][j] = s / d;
        }
    }
    if (!ok) return;
#pragma unroll
    for (int i = 0; i < 6; ++i) {  // L z = -JTr
        double s = -S[2 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * x[k];
        x[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] /= D[i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {  // L^T x = y
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
        x[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (!(fabs(x[i]) <= 1.7976931348623157e308)) ok = false;
    if (!ok) return;
    const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sg = sin(x[2]), cg = cos(x[2]);
    // Rz(x2) Ry(x1) Rx(x0)
    const double R[3][3] = {{cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa},
                            {sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa},
                            {-sb, cb * sa, cb * ca}};
    ColorCam& cm = cams[c];
    double E[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) E[k] = cm.E[k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double s = (R[r][0] * E[k] + R[r][1] * E[4 + k]) + R[r][2] * E[8 + k];
            if (k == 3) s += x[3 + r];
            cm.E[4 * r + k] = s;
        }
}

// the float64 colour means over the visibility pairs at the current poses (SetGeometryColorAverage)
__global__ __launch_bounds__(kThreads) void k_cmo_color_avg(const float* __restrict__ V, const int32_t* __restrict__ v2i,
                                                           const int64_t* __restrict__ voff,
                                                           const ColorCam* __restrict__ cams,
                                                           const uint8_t* __restrict__ images, Params P,
                                                           double* __restrict__ avg, int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P.nv) return;
    const double X = V[3 * i], Y = V[3 * i + 1], Z = V[3 * i + 2];
    const int64_t HW = (int64_t)P.H * P.W;
    double sr = 0.0, sg = 0.0, sb = 0.0;
    int cnt = 0;
    for (int64_t e = voff[i]; e < voff[i + 1]; ++e) {
        const int c = v2i[e];
        float u, v, d;
        project_f(cams[c], X, Y, Z, u, v, d);
        int ui, vi;
        if (!in_margin(u, v, P.H, P.W, P.margin) || !rounded_pixel(u, v, P.H, P.W, ui, vi)) continue;
        const uint8_t* p = images + 3 * (c * HW + (int64_t)vi * P.W + ui);
        sr += (double)((float)p[0] / 255.0f);
        sg += (double)((float)p[1] / 255.0f);
        sb += (double)((float)p[2] / 255.0f);
        ++cnt;
    }
    avg[3 * i] = cnt ? sr / cnt : 0.0;
    avg[3 * i + 1] = cnt ? sg / cnt : 0.0;
    avg[3 * i + 2] = cnt ? sb / cnt : 0.0;
    counts[i] = cnt;
}

}  // namespace cmo
}  // namespace mqr

using namespace mqr;
using namespace mqr::cmo;

struct mqr_colormap {
    int device = 0;
    Params P{};
    bool empty = true;  // N == 0 or nv == 0: nothing on the device
    hipStream_t s = nullptr;
    std::vector<void*> owned;  // hipMalloc'ed for the life of the handle
    const float* V = nullptr;
    const uint8_t* images = nullptr;
    ColorCam* cams = nullptr;
    float4* util = nullptr;
    double* proxy = nullptr;
    int32_t* i2v = nullptr;
    int32_t* v2i = nullptr;
    int64_t* voff = nullptr;
    int64_t* kf_off = nullptr;
    int64_t* chunk_start = nullptr;
    Chunk* chunks = nullptr;
    double* slabs = nullptr;
    double* sys = nullptr;
    int64_t pairs = 0, n_chunks = 0;
    std::vector<int64_t> h_kf_off;
    std::vector<ColorCam> h_cams;
    bool proxy_stale = true;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the last optimize's launches (mqr_colormap_optimize_ms)
    float last_ms = 0.f;

    void* dmalloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        owned.push_back(p);
        return p;
    }
};

namespace {

unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

void release(mqr_colormap* h) {
    if (!h) return;
    if (h->s) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->s);
    }
    for (void* p : h->owned) (void)hipFree(p);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->s) (void)hipStreamDestroy(h->s);
    delete h;
}

bool all_finite(const double* a, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

void enqueue_proxy(mqr_colormap* h) {
    hipLaunchKernelGGL(k_cmo_proxy, dim3(blocks_of(h->P.nv)), dim3(kThreads), 0, h->s, h->V, h->v2i, h->voff, h->cams,
                       h->util, h->P, h->proxy);
    h->proxy_stale = false;
}

// one evaluation of every keyframe's system at the current poses and proxies (sys[N][29]); with `update`
// also the pose updates and the (r2, count) record
void enqueue_systems(mqr_colormap* h, double* rec, int update) {
    if (h->n_chunks > 0)
        hipLaunchKernelGGL(k_cmo_systems, dim3((unsigned)h->n_chunks), dim3(kThreads), 0, h->s, h->V, h->i2v, h->kf_off,
                           h->chunks, h->cams, h->util, h->proxy, h->P, h->slabs);
    hipLaunchKernelGGL(k_cmo_solve, dim3((unsigned)h->P.N), dim3(64), 0, h->s, h->slabs, h->chunk_start, h->cams, h->sys,
                       rec, update);
}

}  // namespace

extern "C" {

int mqr_colormap_create(int device, const float* vertices, int64_t nv, int vloc, const uint8_t* images,
                        const float* t_hit, int img_loc, int N, int H, int W, const double* K, const double* T_wc,
                        double max_depth, double visibility_threshold, int margin, double disc_threshold,
                        int half_dilation, double depth_trunc, mqr_colormap** out) {
    MQR_REQUIRE(out, "null argument");
    *out = nullptr;
    MQR_REQUIRE(nv >= 0 && N >= 0 && N <= kMaxKeyframes && H >= 2 && W >= 2 && half_dilation >= 0 && margin >= 0,
                "mqr_colormap_create: bad sizes");
    MQR_REQUIRE(nv < (int64_t{1} << 31), "mqr_colormap_create: vertex ids are int32");
    MQR_REQUIRE((int64_t)H * W < (int64_t{1} << 31) && W < (1 << 24) && H < (1 << 24), "mqr_colormap_create: frame too large");
    MQR_REQUIRE((vloc == MQR_HOST || vloc == MQR_DEVICE) && (img_loc == MQR_HOST || img_loc == MQR_DEVICE),
                "mqr_colormap_create: locations must be MQR_HOST or MQR_DEVICE");
    mqr_colormap* h = new (std::nothrow) mqr_colormap();
    MQR_REQUIRE(h, "mqr_colormap_create: out of memory");
    h->device = device;
    h->P.max_depth = max_depth;
    h->P.vis_thr = visibility_threshold;
    h->P.depth_trunc = (float)depth_trunc;
    h->P.margin = margin;
    h->P.N = N, h->P.H = H, h->P.W = W, h->P.nv = nv;
    if (N == 0 || nv == 0) {
        *out = h;
        return 0;
    }
    auto bail = [&](int rc, const char* msg) {
        if (msg) set_error(msg);
        release(h);
        return rc;
    };
    if (!(vertices && images && t_hit && K && T_wc)) return bail(2, "null argument");
    if (!all_finite(K, 9 * (size_t)N) || !all_finite(T_wc, 16 * (size_t)N))
        return bail(2, "mqr_colormap_create: non-finite intrinsic or extrinsic matrix");
    const int64_t HW = (int64_t)H * W, NHW = HW * N;
    const int64_t nvb = (nv + kThreads - 1) / kThreads;
    if (nvb * N + 1 >= (int64_t{1} << 31)) return bail(2, "mqr_colormap_create: too many (keyframe, vertex block) pairs");
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking) != hipSuccess) {
        h->s = nullptr;
        return bail(1, "mqr_colormap_create: no device or stream");
    }
    hipStream_t s = h->s;
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess)
        return bail(1, "mqr_colormap_create: event creation failed");
    if ((vloc == MQR_DEVICE || img_loc == MQR_DEVICE) && order_after_caller(device, s)) return bail(2, nullptr);
    h->empty = false;
    h->h_cams.resize(N);
    fill_color_cams(K, T_wc, N, h->h_cams.data());

    // what the handle keeps
    if (vloc == MQR_DEVICE) {
        h->V = vertices;
    } else {
        void* p = h->dmalloc(sizeof(float) * 3 * nv);
        if (!p || copy_to_device(device, p, vertices, sizeof(float) * 3 * nv, s)) return bail(1, "mqr_colormap_create: vertex upload failed");
        h->V = static_cast<const float*>(p);
    }
    if (img_loc == MQR_DEVICE) {
        h->images = images;
    } else {
        void* p = h->dmalloc((size_t)3 * NHW);
        if (!p || copy_to_device(device, p, images, (size_t)3 * NHW, s)) return bail(1, "mqr_colormap_create: image upload failed");
        h->images = static_cast<const uint8_t*>(p);
    }
    h->cams = static_cast<ColorCam*>(h->dmalloc(sizeof(ColorCam) * N));
    h->util = static_cast<float4*>(h->dmalloc(sizeof(float4) * NHW));
    h->proxy = static_cast<double*>(h->dmalloc(sizeof(double) * nv));
    h->voff = static_cast<int64_t*>(h->dmalloc(sizeof(int64_t) * (nv + 1)));
    h->kf_off = static_cast<int64_t*>(h->dmalloc(sizeof(int64_t) * (N + 1)));
    h->chunk_start = static_cast<int64_t*>(h->dmalloc(sizeof(int64_t) * (N + 1)));
    h->sys = static_cast<double*>(h->dmalloc(sizeof(double) * kSums * N));
    if (!h->cams || !h->util || !h->proxy || !h->voff || !h->kf_off || !h->chunk_start || !h->sys)
        return bail(1, "mqr_colormap_create: device allocation failed");
    if (copy_to_device(device, h->cams, h->h_cams.data(), sizeof(ColorCam) * N, s))
        return bail(1, "mqr_colormap_create: upload failed");

    // scratch of this call, from the device-block cache (returned after the final synchronisation)
    const int64_t nb = nvb * N + 1;
    const bool hi = img_loc != MQR_DEVICE;
    ScratchLayout L;
    float *d_t, *hx, *hy;
    uint8_t *m0, *mask;
    int64_t *bcnt, *boff, *vcnt;
    L.add(d_t, NHW, hi);
    L.add_each(NHW, hx, hy, m0, mask);
    L.add_each(nb, bcnt, boff);
    L.add(vcnt, nv + 1);
    auto scan_blocks = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, bcnt, boff, (int)nb, s); };
    auto scan_vertices = [&](void* t, size_t& b) {
        return hipcub::DeviceScan::ExclusiveSum(t, b, vcnt, h->voff, (int)(nv + 1), s);
    };
    CubTemp tmp;
    if (tmp.lay_out(L, scan_blocks, scan_vertices) != hipSuccess)
        return bail(1, "mqr_colormap_create: scan sizing failed");
    CachedBlock blk(device, L);
    if (!blk.p) return bail(scratch_failed("mqr_colormap_create", L.total()), nullptr);
    auto fail = [&](const char* msg) {
        (void)hipStreamSynchronize(s);  // the scratch block goes back to the cache
        return bail(1, msg);
    };
    const float* dT = hi ? d_t : t_hit;
    if (hi && copy_to_device(device, d_t, t_hit, sizeof(float) * NHW, s)) return fail("mqr_colormap_create: upload failed");
    const unsigned gi = blocks_of(NHW), gv = (unsigned)nvb;
    const Params P = h->P;
    cm_enqueue_masks(s, dT, NHW, H, W, P.depth_trunc, disc_threshold, half_dilation, hx, hy, m0, mask);
    // image -> vertex counts and offsets; vertex -> image counts and offsets
    if (hipMemsetAsync(bcnt + (nb - 1), 0, sizeof(int64_t), s) != hipSuccess ||
        hipMemsetAsync(vcnt + nv, 0, sizeof(int64_t), s) != hipSuccess)
        return fail("mqr_colormap_create: memset failed");
    hipLaunchKernelGGL(k_cmo_vis_block_count, dim3(gv, (unsigned)N), dim3(kThreads), 0, s, h->V, dT, mask, h->cams, P, bcnt);
    hipLaunchKernelGGL(k_cmo_vis_vertex_count, dim3(gv), dim3(kThreads), 0, s, h->V, dT, mask, h->cams, P, vcnt);
    if (tmp.run(scan_blocks) != hipSuccess || tmp.run(scan_vertices) != hipSuccess)
        return fail("mqr_colormap_create: scan failed");
    hipLaunchKernelGGL(k_cmo_kf_offsets, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, s, boff, N, nvb, h->kf_off);
    hipLaunchKernelGGL(k_cmo_chunk_starts, dim3(1), dim3(1), 0, s, h->kf_off, N, h->chunk_start);
    h->h_kf_off.assign(N + 1, 0);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h->h_kf_off.data(), h->kf_off, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail("mqr_colormap_create: visibility count failed");
    h->pairs = h->h_kf_off[N];
    h->n_chunks = 0;
    for (int c = 0; c < N; ++c) h->n_chunks += (h->h_kf_off[c + 1] - h->h_kf_off[c] + kThreads - 1) / kThreads;
    if (h->n_chunks >= (int64_t{1} << 31)) return fail("mqr_colormap_create: too many visibility pairs");
    ScratchLayout Lh;  // the handle's arrays whose sizes the read-back gave: one allocation of the handle's
    Lh.add_each(h->pairs, h->i2v, h->v2i);
    Lh.add(h->chunks, h->n_chunks);
    Lh.add(h->slabs, kSums * h->n_chunks);
    void* held = Lh.valid() ? h->dmalloc(Lh.total()) : nullptr;
    if (!held) {
        (void)hipStreamSynchronize(s);
        return bail(scratch_failed("mqr_colormap_create", Lh.total()), nullptr);
    }
    Lh.bind(held);
    if (h->pairs > 0) {
        hipLaunchKernelGGL(k_cmo_vis_block_emit, dim3(gv, (unsigned)N), dim3(kThreads), 0, s, h->V, dT, mask, h->cams, P,
                           boff, h->i2v);
        hipLaunchKernelGGL(k_cmo_vis_vertex_emit, dim3(gv), dim3(kThreads), 0, s, h->V, dT, mask, h->cams, P, h->voff,
                           h->v2i);
        hipLaunchKernelGGL(k_cmo_chunk_table, dim3((unsigned)N), dim3(256), 0, s, h->kf_off, h->chunk_start, h->chunks);
    }
    // utility images (hx, hy are free again: the masks are done with them on this stream)
    hipLaunchKernelGGL(k_cmo_gray_h, dim3(gi), dim3(256), 0, s, h->images, NHW, W, hx);
    hipLaunchKernelGGL(k_cmo_gray_v, dim3(gi), dim3(256), 0, s, hx, NHW, H, W, reinterpret_cast<float*>(h->util));
    hipLaunchKernelGGL(k_cmo_sobel_h, dim3(gi), dim3(256), 0, s, reinterpret_cast<const float*>(h->util), NHW, W, hx, hy);
    hipLaunchKernelGGL(k_cmo_sobel_v, dim3(gi), dim3(256), 0, s, hx, hy, NHW, H, W, reinterpret_cast<float*>(h->util));
    if (hipGetLastError() != hipSuccess) return fail("mqr_colormap_create: kernel launch failed");
    if (hipStreamSynchronize(s) != hipSuccess) return bail(1, "mqr_colormap_create: kernel failed");
    *out = h;
    return 0;
}

int mqr_colormap_destroy(mqr_colormap* h) {
    release(h);
    return 0;
}

int mqr_colormap_counts(mqr_colormap* h, int64_t* pairs_per_keyframe) {
    MQR_REQUIRE(h && (pairs_per_keyframe || h->P.N == 0), "null argument");
    for (int c = 0; c < h->P.N; ++c)
        pairs_per_keyframe[c] = h->empty ? 0 : h->h_kf_off[c + 1] - h->h_kf_off[c];
    return 0;
}

int mqr_colormap_get_poses(mqr_colormap* h, double* T_wc) {
    MQR_REQUIRE(h && (T_wc || h->P.N == 0), "null argument");
    if (h->empty) return 0;  // (nothing is held: the caller's poses are the poses)
    for (int c = 0; c < h->P.N; ++c) {
        std::memcpy(T_wc + 16 * (size_t)c, h->h_cams[c].E, sizeof(double) * 12);
        T_wc[16 * (size_t)c + 12] = T_wc[16 * (size_t)c + 13] = T_wc[16 * (size_t)c + 14] = 0.0;
        T_wc[16 * (size_t)c + 15] = 1.0;
    }
    return 0;
}

int mqr_colormap_set_poses(mqr_colormap* h, const double* T_wc) {
    MQR_REQUIRE(h && (T_wc || h->P.N == 0), "null argument");
    if (h->empty) return 0;
    MQR_REQUIRE(all_finite(T_wc, 16 * (size_t)h->P.N), "mqr_colormap_set_poses: non-finite extrinsic matrix");
    MQR_CHECK_HIP(hipSetDevice(h->device));
    for (int c = 0; c < h->P.N; ++c) std::memcpy(h->h_cams[c].E, T_wc + 16 * (size_t)c, sizeof(double) * 12);
    if (copy_to_device(h->device, h->cams, h->h_cams.data(), sizeof(ColorCam) * h->P.N, h->s)) return 1;
    h->proxy_stale = true;
    return 0;
}

int mqr_colormap_proxy(mqr_colormap* h, double* proxy) {
    MQR_REQUIRE(h, "null argument");
    if (h->empty) {
        if (proxy) std::memset(proxy, 0, sizeof(double) * (size_t)h->P.nv);
        return 0;
    }
    MQR_CHECK_HIP(hipSetDevice(h->device));
    enqueue_proxy(h);
    MQR_CHECK_HIP(hipGetLastError());
    if (proxy && copy_to_host(h->device, proxy, h->proxy, sizeof(double) * (size_t)h->P.nv, h->s)) return 1;
    MQR_CHECK_HIP(hipStreamSynchronize(h->s));
    return 0;
}

int mqr_colormap_systems(mqr_colormap* h, double* JTJ, double* JTr, double* r2, int64_t* count) {
    MQR_REQUIRE(h, "null argument");
    const int N = h->P.N;
    MQR_REQUIRE(N == 0 || (JTJ && JTr && r2 && count), "null argument");
    if (h->empty) {
        for (int c = 0; c < N; ++c) {
            std::memset(JTJ + 36 * (size_t)c, 0, sizeof(double) * 36);
            std::memset(JTr + 6 * (size_t)c, 0, sizeof(double) * 6);
            r2[c] = 0.0;
            count[c] = 0;
        }
        return 0;
    }
    MQR_CHECK_HIP(hipSetDevice(h->device));
    if (h->proxy_stale) enqueue_proxy(h);
    enqueue_systems(h, nullptr, 0);
    MQR_CHECK_HIP(hipGetLastError());
    std::vector<double> S((size_t)kSums * N);
    MQR_CHECK_HIP(hipMemcpyAsync(S.data(), h->sys, sizeof(double) * S.size(), hipMemcpyDeviceToHost, h->s));
    MQR_CHECK_HIP(hipStreamSynchronize(h->s));
    for (int c = 0; c < N; ++c) {
        const double* q = S.data() + (size_t)kSums * c;
        count[c] = (int64_t)q[0];
        r2[c] = q[1];
        for (int a = 0; a < 6; ++a) JTr[6 * (size_t)c + a] = q[2 + a];
        int k = 8;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b, ++k) JTJ[36 * (size_t)c + 6 * a + b] = JTJ[36 * (size_t)c + 6 * b + a] = q[k];
    }
    return 0;
}

int mqr_colormap_optimize(mqr_colormap* h, int max_iteration, double* residuals, int64_t* counts) {
    MQR_REQUIRE(h && max_iteration >= 0, "mqr_colormap_optimize: bad arguments");
    if (max_iteration == 0) return 0;
    MQR_REQUIRE(residuals && counts, "null argument");
    const int N = h->P.N;
    if (h->empty) {
        for (int it = 0; it < max_iteration; ++it) residuals[it] = 0.0, counts[it] = 0;
        return 0;
    }
    MQR_CHECK_HIP(hipSetDevice(h->device));
    const size_t nrec = (size_t)2 * N * max_iteration;
    double* rec = nullptr;
    MQR_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&rec), sizeof(double) * nrec));
    std::vector<double> hrec(nrec);
    int rc = 0;
    if (h->proxy_stale) enqueue_proxy(h);
    (void)hipEventRecord(h->ev0, h->s);
    for (int it = 0; it < max_iteration; ++it) {  // three launches per iteration, no host read in between
        enqueue_systems(h, rec + (size_t)2 * N * it, 1);
        enqueue_proxy(h);
    }
    (void)hipEventRecord(h->ev1, h->s);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(hrec.data(), rec, sizeof(double) * nrec, hipMemcpyDeviceToHost, h->s) != hipSuccess ||
        hipMemcpyAsync(h->h_cams.data(), h->cams, sizeof(ColorCam) * N, hipMemcpyDeviceToHost, h->s) != hipSuccess) {
        set_error("mqr_colormap_optimize: launch or copy failed");
        rc = 1;
    }
    if (hipStreamSynchronize(h->s) != hipSuccess && !rc) {
        set_error("mqr_colormap_optimize: kernel failed");
        rc = 1;
    }
    if (!rc && hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1) != hipSuccess) h->last_ms = 0.f;
    (void)hipFree(rec);
    if (rc) return rc;
    for (int it = 0; it < max_iteration; ++it) {  // the iteration's residual: the keyframes' r2 in keyframe order
        double r = 0.0, n = 0.0;
        for (int c = 0; c < N; ++c) {
            r += hrec[((size_t)it * N + c) * 2];
            n += hrec[((size_t)it * N + c) * 2 + 1];
        }
        residuals[it] = r;
        counts[it] = (int64_t)n;
    }
    return 0;
}

int mqr_colormap_optimize_ms(mqr_colormap* h, float* ms) {
    MQR_REQUIRE(h && ms, "null argument");
    *ms = h->last_ms;
    return 0;
}

#ifndef MQR_CMO_SRC_TAG
#define MQR_CMO_SRC_TAG "unknown"
#endif
int mqr_colormap_build_tag(char* buf, int n) {
    MQR_REQUIRE(buf && n > 0, "null argument");
    std::strncpy(buf, MQR_CMO_SRC_TAG, (size_t)n - 1);
    buf[n - 1] = 0;
    return 0;
}

int mqr_colormap_colors(mqr_colormap* h, int knn, float* colors, int32_t* counts, int loc) {
    MQR_REQUIRE(h && knn >= 0 && knn <= 8, "mqr_colormap_colors: bad arguments");
    MQR_REQUIRE(loc == MQR_HOST || loc == MQR_DEVICE, "mqr_colormap_colors: loc must be MQR_HOST or MQR_DEVICE");
    const int64_t nv = h->P.nv;
    if (nv == 0) return 0;
    MQR_REQUIRE(colors, "null argument");
    if (h->empty) {  // no keyframes: nothing is sampled
        if (loc == MQR_HOST) {
            std::memset(colors, 0, sizeof(float) * 3 * (size_t)nv);
            if (counts) std::memset(counts, 0, sizeof(int32_t) * (size_t)nv);
        } else {
            MQR_CHECK_HIP(hipSetDevice(h->device));
            MQR_CHECK_HIP(hipMemset(colors, 0, sizeof(float) * 3 * (size_t)nv));
            if (counts) MQR_CHECK_HIP(hipMemset(counts, 0, sizeof(int32_t) * (size_t)nv));
        }
        return 0;
    }
    MQR_CHECK_HIP(hipSetDevice(h->device));
    hipStream_t s = h->s;
    if (loc == MQR_DEVICE && order_after_caller(h->device, s)) return 2;
    ScratchLayout L;
    double* avg;
    int32_t* cnt;
    float* d_o;
    L.add(avg, 3 * nv);
    L.add(cnt, nv);
    L.add(d_o, 3 * nv, loc != MQR_DEVICE);
    CachedBlock blk(h->device, L);
    if (!blk.p) return scratch_failed("mqr_colormap_colors", L.total());
    float* dO = loc == MQR_DEVICE ? colors : d_o;
    int rc = 0;
    hipLaunchKernelGGL(k_cmo_color_avg, dim3(blocks_of(nv)), dim3(kThreads), 0, s, h->V, h->v2i, h->voff, h->cams,
                       h->images, h->P, avg, cnt);
    if (hipGetLastError() != hipSuccess) {
        set_error("mqr_colormap_colors: kernel launch failed");
        rc = 1;
    }
    if (!rc) rc = cm_finish_colors(h->device, s, h->V, nv, avg, cnt, knn, dO, "mqr_colormap_colors");
    if (!rc && loc != MQR_DEVICE &&
        (copy_to_host(h->device, colors, dO, sizeof(float) * 3 * nv, s) ||
         (counts && copy_to_host(h->device, counts, cnt, sizeof(int32_t) * nv, s)))) {
        set_error("mqr_colormap_colors: copy back failed");
        rc = 1;
    }
    if (!rc && loc == MQR_DEVICE && counts &&
        hipMemcpyAsync(counts, cnt, sizeof(int32_t) * nv, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("mqr_colormap_colors: copy failed");
        rc = 1;
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) {
        set_error("mqr_colormap_colors: kernel failed");
        rc = 1;
    }
    return rc;
}

}  // extern "C"
