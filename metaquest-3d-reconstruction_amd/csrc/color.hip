// color.hip -- per-vertex colour projection from keyframes.
//
// The reference colours its mesh with Open3D's colour-map pipeline: the extracted mesh, the colour
// keyframes and their colour-aligned depth (ray-cast from the mesh, raycast_in_color_view,
// o3d_utils.py:324-341) go to run_rigid_optimizer (optimize_color_pose.py:24-73).  Its colour
// assignment -- the part that is bandwidth work and runs on every iteration -- is the visibility
// test plus per-vertex averaging of upstream ColorMapUtils.cpp (CreateVertexAndImageVisibility,
// SetGeometryColorAverage; recalled, not vendored here -- VERIFY):
//   Vt = T_c [X 1] (float64), u = float(Vt.x fx / Vt.z + cx), v = float(Vt.y fy / Vt.z + cy),
//   d = float(Vt.z); ui = int(round(u)), vi = int(round(v));
//   visible in keyframe c iff d >= 0, (ui, vi) inside the image, depth_c(ui, vi) <= max_depth and
//   |d - depth_c(ui, vi)| < visibility_threshold (float difference, compared in float64);
//   sampled iff also margin <= u < W - margin and margin <= v < H - margin: the colour is the
//   average over the sampled keyframes of (float)image_c(ui, vi) / 255.0f, summed in float64 in
//   keyframe order.
// mqr_color_vertices is that visibility-and-average primitive; mqr_color_map (below) is the complete
// assignment -- RGBD depth truncation, depth-discontinuity masks, float64 averages and the
// k-nearest-neighbour fill of vertices no keyframe sees.  The pose optimisation is colormap.hip's; it shares
// the masks and the fill with this file through color_shared.hpp.
//
// One thread per vertex, keyframe loop in registers; the keyframe parameters sit in constant-
// cached global memory.  Colour images are RGB uint8 [N][H][W][3], depth float32 [N][H][W].
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <mutex>
#include <memory>
#include <vector>

#include "mqr_common.hpp"
#include "device_block.hpp"
#include "device_cub.hpp"
#include "bucket_tree.hpp"
#include "color_shared.hpp"

namespace mqr {

__global__ __launch_bounds__(256) void k_color_vertices(const float* __restrict__ V, int64_t nv,
                                                        const uint8_t* __restrict__ images,
                                                        const float* __restrict__ depths,
                                                        const ColorCam* __restrict__ cams, int N, int H, int W,
                                                        double max_depth, double vis_thr, int margin,
                                                        float* __restrict__ out, int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const double X = V[3 * i], Y = V[3 * i + 1], Z = V[3 * i + 2];
    double sr = 0.0, sg = 0.0, sb = 0.0;
    int cnt = 0;
    const int64_t HW = (int64_t)H * W;
    for (int c = 0; c < N; ++c) {
        const ColorCam& cm = cams[c];
        const double vx = cm.E[0] * X + cm.E[1] * Y + cm.E[2] * Z + cm.E[3];
        const double vy = cm.E[4] * X + cm.E[5] * Y + cm.E[6] * Z + cm.E[7];
        const double vz = cm.E[8] * X + cm.E[9] * Y + cm.E[10] * Z + cm.E[11];
        const float u = (float)((vx * cm.fx) / vz + cm.cx);
        const float v = (float)((vy * cm.fy) / vz + cm.cy);
        const float d = (float)vz;
        const int ui = (int)roundf(u), vi = (int)roundf(v);
        if (d < 0.0f || ui < 0 || ui >= W || vi < 0 || vi >= H) continue;
        const int64_t px = (int64_t)c * HW + (int64_t)vi * W + ui;
        const float ds = depths[px];
        if (ds > max_depth) continue;
        if (!((double)fabsf(d - ds) < vis_thr)) continue;
        if (!(u >= margin && u < W - margin && v >= margin && v < H - margin)) continue;
        const uint8_t* p = images + 3 * px;
        // upstream: float r = (float)r_temp / 255.0f, summed into a double vector
        sr += (double)((float)p[0] / 255.0f);
        sg += (double)((float)p[1] / 255.0f);
        sb += (double)((float)p[2] / 255.0f);
        ++cnt;
    }
    out[3 * i] = cnt ? (float)(sr / cnt) : 0.f;
    out[3 * i + 1] = cnt ? (float)(sg / cnt) : 0.f;
    out[3 * i + 2] = cnt ? (float)(sb / cnt) : 0.f;
    if (counts) counts[i] = cnt;
}

// ================================================================== complete colour map (mqr_color_map)
// run_rigid_optimizer's vertex colours with the keyframe poses as given (= maximum_iteration 0; the pose
// refinement is colormap.hip), upstream ColorMapUtils / Image.cpp as recalled -- VERIFY:
//   RGBD depth d = t_hit / 1.0, d >= depth_trunc (3.0, create_from_color_and_depth's default) -> 0;
//   depth-boundary mask: Sobel dx = (Sobel31 along x, then Sobel32 along y), dy = (Sobel32, Sobel31),
//     every pass a float32 image of double sums of float products over the clamped 3-tap window;
//     sqrt(dx^2 + dy^2) > 0.1 -> 255, dilated over the (2 half + 1)^2 window (half = 3);
//   visibility as k_color_vertices plus mask != 255; float64 averages; vertices no keyframe samples
//   take the float64 mean of their knn (3) nearest sampled vertices' colours (squared-distance ties
//   broken by the lower vertex index).

// horizontal pass of both filters from the truncated depth: hx = Sobel31 along x, hy = Sobel32 along x
__global__ void k_cm_filter_h(const float* __restrict__ t_hit, int64_t total, int H, int W, float depth_trunc,
                              float* __restrict__ hx, float* __restrict__ hy) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const int64_t row = i - x;
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int xs = min(max(x + k - 1, 0), W - 1);
        const float v = t_hit[row + xs] / 1.0f;
        d[k] = v >= depth_trunc ? 0.0f : v;
    }
    double a = 0, b = 0;
    a += (double)(d[0] * -1.0f);
    a += (double)(d[1] * 0.0f);
    a += (double)(d[2] * 1.0f);
    b += (double)(d[0] * 1.0f);
    b += (double)(d[1] * 2.0f);
    b += (double)(d[2] * 1.0f);
    hx[i] = (float)a;
    hy[i] = (float)b;
    (void)H;
}

// vertical passes (dx = Sobel32 along y of hx, dy = Sobel31 along y of hy) and the threshold
__global__ void k_cm_filter_v(const float* __restrict__ hx, const float* __restrict__ hy, int64_t total, int H, int W,
                              double disc_thr, uint8_t* __restrict__ m0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t HW = (int64_t)H * W;
    const int64_t f = i / HW;
    const int p = (int)(i - f * HW), y = p / W, x = p % W;
    double a = 0, b = 0;
    const float ka[3] = {1.0f, 2.0f, 1.0f}, kb[3] = {-1.0f, 0.0f, 1.0f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ys = min(max(y + k - 1, 0), H - 1);
        const int64_t q = f * HW + (int64_t)ys * W + x;
        a += (double)(hx[q] * ka[k]);
        b += (double)(hy[q] * kb[k]);
    }
    const double dx = (double)(float)a, dy = (double)(float)b;
    m0[i] = sqrt(dx * dx + dy * dy) > disc_thr ? 255 : 0;
}

__global__ void k_cm_dilate(const uint8_t* __restrict__ m0, int64_t total, int H, int W, int half,
                            uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t HW = (int64_t)H * W;
    const int64_t f = i / HW;
    const int p = (int)(i - f * HW), y = p / W, x = p % W;
    uint8_t o = 0;
    for (int yy = max(y - half, 0); yy <= min(y + half, H - 1) && !o; ++yy)
        for (int xx = max(x - half, 0); xx <= min(x + half, W - 1); ++xx)
            if (m0[f * HW + (int64_t)yy * W + xx] == 255) {
                o = 255;
                break;
            }
    mask[i] = o;
}

__global__ __launch_bounds__(256) void k_cm_vertices(const float* __restrict__ V, int64_t nv,
                                                     const uint8_t* __restrict__ images,
                                                     const float* __restrict__ t_hit, const uint8_t* __restrict__ mask,
                                                     const ColorCam* __restrict__ cams, int N, int H, int W,
                                                     double max_depth, double vis_thr, int margin, float depth_trunc,
                                                     double* __restrict__ avg, int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const double X = V[3 * i], Y = V[3 * i + 1], Z = V[3 * i + 2];
    double sr = 0.0, sg = 0.0, sb = 0.0;
    int cnt = 0;
    const int64_t HW = (int64_t)H * W;
    for (int c = 0; c < N; ++c) {
        const ColorCam& cm = cams[c];
        const double vx = cm.E[0] * X + cm.E[1] * Y + cm.E[2] * Z + cm.E[3];
        const double vy = cm.E[4] * X + cm.E[5] * Y + cm.E[6] * Z + cm.E[7];
        const double vz = cm.E[8] * X + cm.E[9] * Y + cm.E[10] * Z + cm.E[11];
        const float u = (float)((vx * cm.fx) / vz + cm.cx);
        const float v = (float)((vy * cm.fy) / vz + cm.cy);
        const float d = (float)vz;
        const int ui = (int)roundf(u), vi = (int)roundf(v);
        if (d < 0.0f || ui < 0 || ui >= W || vi < 0 || vi >= H) continue;
        const int64_t px = (int64_t)c * HW + (int64_t)vi * W + ui;
        const float th = t_hit[px] / 1.0f;
        const float ds = th >= depth_trunc ? 0.0f : th;
        if (ds > max_depth) continue;
        if (mask[px] == 255) continue;
        if (!((double)fabsf(d - ds) < vis_thr)) continue;
        if (!(u >= margin && u < W - margin && v >= margin && v < H - margin)) continue;
        const uint8_t* p = images + 3 * px;
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

// ---- knn over the sampled vertices: bucket_tree.hpp's Morton-bucket tree (built by bucket_tree.hip), exact
// search in float64.
//
// The knn (3) nearest sampled vertices of every unseen vertex (exact: float64 squared distances of the
// float32 positions, ties by vertex index, the oracle's k-d tree rule), then the mean of their colours.
// K = knn at compile time: the running best list lives in registers (static indices, an unrolled
// insertion).  Boxes are pruned and ordered in float32 on a proven lower bound (box_d2_lb); candidates are
// prefiltered on the same bound and compared exactly in float64.
// The traversal is shared by a wave: the wave's 64 queries -- neighbours in vertex order, so close in space --
// walk one stack of nodes together (node indices wave-uniform, read by scalar loads; 64 entries per wave in
// LDS, and a nearest-first DFS holds at most depth + 2), a node is skipped only when every lane's bound
// prunes it, and each lane keeps its own exact best list.  A lane may so test nodes it would have pruned
// alone: that only offers it candidates its own search would have rejected or met anyway, and the kept list
// is a total order on (d2, index), so the result is the same.  Inactive lanes (past the query count) prune
// everything.
// History, C5's 17.5 M unseen vertices: one traversal per lane with a 64 x int64 stack and a KMAX = 8 list
// with dynamic indices, both in scratch, 64 ms (round 4); float64 box tests and a 32-entry stack 44.5 ms,
// then float32 bounds, the list in registers and a stack-major LDS stack of depth + 2 entries 23.8 ms (round
// 5, profiles/r05_c5_kernel_stats.csv); this shared walk 12.7 ms (round 6, profiles/r06_ab_knn_wave.json: the
// A/B that decided against the per-lane kernel).  meshcompare.hip's k_nn1 is the per-lane form still in use.
template <int K>
__global__ __launch_bounds__(256) void k_cm_knn_fill_wave(const float* __restrict__ V, const int32_t* __restrict__ qids,
                                                          int64_t nq, const float4* __restrict__ pts, int64_t n,
                                                          int64_t P, const float4* __restrict__ lo,
                                                          const float4* __restrict__ hi,
                                                          const double* __restrict__ avg, float* __restrict__ out) {
    extern __shared__ int32_t stk_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t* stk = stk_lds + wave * 64;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = t < nq;
    const int32_t qv = active ? qids[t] : 0;
    float qf[3] = {0.f, 0.f, 0.f};
    if (active) {
        qf[0] = V[3 * (int64_t)qv];
        qf[1] = V[3 * (int64_t)qv + 1];
        qf[2] = V[3 * (int64_t)qv + 2];
    }
    const double q[3] = {qf[0], qf[1], qf[2]};
    double bd[K];
    int32_t bi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        bd[k] = active ? __builtin_inf() : -1.0;  // an inactive lane prunes every node
        bi[k] = 0x7fffffff;
    }
    if (__ballot(active) == 0) return;  // (wave-uniform)
    int sp = 0;
    if (lane == 0) stk[0] = 1;
    sp = 1;
    while (sp) {
        __builtin_amdgcn_wave_barrier();
        const int32_t node = __builtin_amdgcn_readfirstlane(stk[--sp]);
        const float4 nlo = lo[node], nhi = hi[node];
        if (!__ballot((double)box_d2_lb(qf, nlo, nhi) <= bd[K - 1])) continue;
        if (node >= P) {  // bucket
            const int64_t b = node - P;
            const int64_t e = min(n, (b + 1) * kBucket);
            for (int64_t j = b * kBucket; j < e; ++j) {
                const float4 pt = pts[j];
                const float fx = qf[0] - pt.x, fy = qf[1] - pt.y, fz = qf[2] - pt.z;
                if ((double)((fx * fx + fy * fy + fz * fz) * (1.0f - 0x1p-18f)) > bd[K - 1]) continue;
                const int32_t v = __float_as_int(pt.w);
                const double dx = q[0] - (double)pt.x, dy = q[1] - (double)pt.y, dz = q[2] - (double)pt.z;
                const double d2 = dx * dx + dy * dy + dz * dz;
                auto before = [&](int k) { return d2 < bd[k] || (d2 == bd[k] && v < bi[k]); };
                if (!before(K - 1)) continue;
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {
                    if (k > 0 && before(k - 1)) {
                        bd[k] = bd[k - 1];
                        bi[k] = bi[k - 1];
                    } else if (before(k)) {
                        bd[k] = d2;
                        bi[k] = v;
                    }
                }
            }
        } else {  // both children, the one nearer for most lanes popped first
            const int32_t a = 2 * node, c = a + 1;
            const float da = box_d2_lb(qf, lo[a], hi[a]), dc = box_d2_lb(qf, lo[c], hi[c]);
            const uint64_t m = __ballot(active && da <= dc), act = __ballot(active);
            const bool a_first = 2 * __popcll(m) >= __popcll(act);
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) {
                stk[sp] = a_first ? c : a;
                stk[sp + 1] = a_first ? a : c;
            }
            sp += 2;
        }
    }
    if (!active) return;
    int nb = 0;
    double cc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (bd[k] != __builtin_inf()) {
            ++nb;
#pragma unroll
            for (int a = 0; a < 3; ++a) cc[a] += avg[3 * (int64_t)bi[k] + a];
        }
    if (nb > 0)
#pragma unroll
        for (int a = 0; a < 3; ++a) cc[a] /= (double)nb;
#pragma unroll
    for (int a = 0; a < 3; ++a) out[3 * (int64_t)qv + a] = (float)cc[a];
}

__global__ void k_cm_out_seen(const double* __restrict__ avg, const int32_t* __restrict__ counts, int64_t nv,
                              float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv || counts[i] == 0) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) out[3 * i + a] = (float)avg[3 * i + a];
}

__global__ void k_cm_flags(const int32_t* __restrict__ counts, int64_t nv, uint8_t* __restrict__ seen,
                           uint8_t* __restrict__ unseen) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    seen[i] = counts[i] > 0;
    unseen[i] = counts[i] == 0;
}

void cm_enqueue_masks(hipStream_t s, const float* t_hit, int64_t NHW, int H, int W, float depth_trunc,
                      double disc_threshold, int half_dilation, float* hx, float* hy, uint8_t* m0, uint8_t* mask) {
    if (NHW <= 0) return;
    const unsigned gi = (unsigned)((NHW + 255) / 256);
    hipLaunchKernelGGL(k_cm_filter_h, dim3(gi), dim3(256), 0, s, t_hit, NHW, H, W, depth_trunc, hx, hy);
    hipLaunchKernelGGL(k_cm_filter_v, dim3(gi), dim3(256), 0, s, hx, hy, NHW, H, W, disc_threshold, m0);
    hipLaunchKernelGGL(k_cm_dilate, dim3(gi), dim3(256), 0, s, m0, NHW, H, W, half_dilation, mask);
}

int cm_finish_colors(int device, hipStream_t s, const float* dV, int64_t nv, const double* avg, const int32_t* cnt,
                     int knn, float* dO, const char* who) {
    int rc = 0;
    auto fail = [&](const char* msg) {
        set_error(std::string(who) + ": " + msg);
        rc = 1;
    };
    // device staging from the device-block cache (device_block.hpp): the flags and index lists in one block,
    // the knn pass's (sized once the seen vertices are counted) in a second; both returned after the final
    // synchronisation
    ScratchLayout L;
    uint8_t *fseen, *funseen;
    int32_t* ids;  // seen, then unseen
    int64_t* nsel;
    L.add_each(nv, fseen, funseen);
    L.add(ids, 2 * nv);
    L.add(nsel, 2);
    hipcub::CountingInputIterator<int32_t> it(0);
    auto select_seen = [&](void* t, size_t& b) {
        return hipcub::DeviceSelect::Flagged(t, b, it, fseen, ids, nsel, (int)nv, s);
    };
    auto select_unseen = [&](void* t, size_t& b) {
        return hipcub::DeviceSelect::Flagged(t, b, it, funseen, ids + nv, nsel + 1, (int)nv, s);
    };
    CubTemp tmp;
    if (tmp.lay_out(L, select_seen, select_unseen) != hipSuccess) {
        fail("select sizing failed");
        return rc;
    }
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed(who, L.total());
    std::unique_ptr<CachedBlock> blk_knn;
    int64_t nseen = 0, nunseen = 0;
    const unsigned gv = (unsigned)((nv + 255) / 256);
    hipLaunchKernelGGL(k_cm_flags, dim3(gv), dim3(256), 0, s, cnt, nv, fseen, funseen);
    if (tmp.run(select_seen) != hipSuccess || tmp.run(select_unseen) != hipSuccess) fail("select failed");
    int64_t h[2] = {0, 0};
    if (!rc && (hipMemcpyAsync(h, nsel, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess))
        fail("visibility pass failed");
    nseen = h[0];
    nunseen = h[1];
    if (!rc && hipMemsetAsync(dO, 0, sizeof(float) * 3 * nv, s) != hipSuccess) fail("memset failed");
    if (!rc && nseen > 0)
        hipLaunchKernelGGL(k_cm_out_seen, dim3(gv), dim3(256), 0, s, avg, cnt, nv, dO);
    if (!rc && knn > 0 && nseen > 0 && nunseen > 0) {
        // the tree's storage and its build scratch from a second block, sized by bucket_tree.hpp's rules
        const size_t b_scr = bucket_tree_scratch_bytes(nseen, false, s);
        ScratchLayout Lk;
        uint32_t* bb;
        float4 *blo, *bhi, *pts;
        void* scratch;
        Lk.add(bb, 6);
        Lk.add_each(2 * bucket_tree_leaves(nseen), blo, bhi);
        Lk.add(pts, nseen);
        Lk.add_bytes(scratch, b_scr);
        if (!b_scr) fail("knn allocation failed");
        if (!rc) blk_knn.reset(new CachedBlock(device, Lk));
        if (!rc && !blk_knn->p) rc = scratch_failed(who, Lk.total());
        BucketTree t{};
        if (!rc && bucket_tree_build(s, dV, ids, nseen, scratch, b_scr, blo, bhi, pts, bb, &t) != hipSuccess)
            fail("knn tree build failed");
        // the wave's stack holds 64 entries and a nearest-first DFS at most depth + 2 (depth <= 27 for
        // fewer than 2^31 points in buckets of 16)
        if (!rc && t.depth + 2 > 64) fail("the knn tree is too deep for the traversal stack");
        if (!rc) {
            auto fill = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3(nb(nunseen)), dim3(256), sizeof(int32_t) * 4 * 64, s, dV, ids + nv, nunseen,
                                   t.pts, t.n, t.P, t.lo, t.hi, avg, dO);
            };
            switch (knn) {  // knn in [1, 8] (checked on entry)
                case 1: fill(k_cm_knn_fill_wave<1>); break;
                case 2: fill(k_cm_knn_fill_wave<2>); break;
                case 3: fill(k_cm_knn_fill_wave<3>); break;
                case 4: fill(k_cm_knn_fill_wave<4>); break;
                case 5: fill(k_cm_knn_fill_wave<5>); break;
                case 6: fill(k_cm_knn_fill_wave<6>); break;
                case 7: fill(k_cm_knn_fill_wave<7>); break;
                default: fill(k_cm_knn_fill_wave<8>); break;
            }
        }
    }
    if (!rc && hipGetLastError() != hipSuccess) fail("kernel launch failed");
    // the staging blocks go back to the cache at scope exit: everything queued on them has to be done
    if (hipStreamSynchronize(s) != hipSuccess && !rc) fail("kernel failed");
    return rc;
}

}  // namespace mqr

using namespace mqr;

extern "C" {

int mqr_color_vertices(int device, const float* vertices, int64_t nv, int vloc, const uint8_t* images,
                       const float* depths, int img_loc, int N, int H, int W, const double* K, const double* T_wc,
                       double max_depth, double visibility_threshold, int margin, float* colors_out,
                       int32_t* counts_out, int out_loc) {
    MQR_REQUIRE(vertices && images && depths && K && T_wc && colors_out, "null argument");
    MQR_REQUIRE(nv >= 0 && N >= 0 && H > 0 && W > 0, "bad sizes");
    if (nv == 0) return 0;
    MQR_CHECK_HIP(hipSetDevice(device));
    std::vector<ColorCam> cams(N);
    for (int c = 0; c < N; ++c) {
        for (int k = 0; k < 12; ++k) cams[c].E[k] = T_wc[16 * c + k];
        cams[c].fx = K[9 * c + 0];
        cams[c].fy = K[9 * c + 4];
        cams[c].cx = K[9 * c + 2];
        cams[c].cy = K[9 * c + 5];
    }
    hipStream_t s = nullptr;
    MQR_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if ((vloc == MQR_DEVICE || img_loc == MQR_DEVICE || out_loc == MQR_DEVICE) && order_after_caller(device, s)) {
        (void)hipStreamDestroy(s);
        return 2;
    }
    int rc = 0;
    const int64_t HW = (int64_t)H * W;
    const bool hv = vloc != MQR_DEVICE, hi = img_loc != MQR_DEVICE, ho = out_loc != MQR_DEVICE;
    // device staging from the device-block cache (device_block.hpp), returned after the final synchronisation
    ScratchLayout L;
    float *d_v, *d_d, *d_o;
    uint8_t* d_i;
    ColorCam* dC;
    int32_t* d_n;
    L.add(d_v, 3 * nv, hv);
    L.add(d_i, 3 * HW * N, hi);
    L.add(d_d, HW * N, hi);
    L.add(dC, N);
    L.add(d_o, 3 * nv, ho);
    L.add(d_n, nv, ho);
    CachedBlock blk(device, L);
    const float *dV = hv ? d_v : vertices, *dD = hi ? d_d : depths;
    const uint8_t* dI = hi ? d_i : images;
    float* dO = ho ? d_o : colors_out;
    int32_t* dN = ho ? d_n : counts_out;
    if (!blk.p) {
        rc = scratch_failed("mqr_color_vertices", L.total());
    } else if ((hv && copy_to_device(device, d_v, vertices, sizeof(float) * 3 * nv, s)) ||
               (hi && (copy_to_device(device, d_i, images, (size_t)3 * HW * N, s) ||
                       copy_to_device(device, d_d, depths, sizeof(float) * HW * N, s))) ||
               copy_to_device(device, dC, cams.data(), sizeof(ColorCam) * N, s)) {
        rc = 1;
    } else {
        hipLaunchKernelGGL(k_color_vertices, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, dV, nv, dI, dD,
                           dC, N, H, W, max_depth, visibility_threshold, margin, dO, dN);
        if (hipGetLastError() != hipSuccess) {
            set_error("mqr_color_vertices: kernel launch failed");
            rc = 1;
        }
        if (!rc && out_loc != MQR_DEVICE &&
            (copy_to_host(device, colors_out, dO, sizeof(float) * 3 * nv, s) ||
             (counts_out && copy_to_host(device, counts_out, dN, sizeof(int32_t) * nv, s)))) {
            set_error("mqr_color_vertices: copy back failed");
            rc = 1;
        }
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) {
        set_error("mqr_color_vertices: kernel failed");
        rc = 1;
    }
    (void)hipStreamDestroy(s);
    return rc;
}

int mqr_color_map(int device, const float* vertices, int64_t nv, int vloc, const uint8_t* images, const float* t_hit,
                  int img_loc, int N, int H, int W, const double* K, const double* T_wc, double max_depth,
                  double visibility_threshold, int margin, double disc_threshold, int half_dilation, double depth_trunc,
                  int knn, float* colors_out, int32_t* counts_out, int out_loc) {
    MQR_REQUIRE(vertices && images && t_hit && K && T_wc && colors_out, "null argument");
    MQR_REQUIRE(nv >= 0 && N >= 0 && H > 0 && W > 0 && knn >= 0 && knn <= 8 && half_dilation >= 0, "bad sizes");
    MQR_REQUIRE(nv < (int64_t{1} << 31), "mqr_color_map: vertex ids are int32");
    if (nv == 0) return 0;
    MQR_CHECK_HIP(hipSetDevice(device));
    std::vector<ColorCam> cams(N);
    for (int c = 0; c < N; ++c) {
        for (int k = 0; k < 12; ++k) cams[c].E[k] = T_wc[16 * c + k];
        cams[c].fx = K[9 * c + 0];
        cams[c].fy = K[9 * c + 4];
        cams[c].cx = K[9 * c + 2];
        cams[c].cy = K[9 * c + 5];
    }
    hipStream_t s = nullptr;
    MQR_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if ((vloc == MQR_DEVICE || img_loc == MQR_DEVICE || out_loc == MQR_DEVICE) && order_after_caller(device, s)) {
        (void)hipStreamDestroy(s);
        return 2;
    }
    // device staging from the device-block cache (device_block.hpp): the visibility pass's arrays in one
    // block (the fill's are cm_finish_colors' own), returned after the final synchronisation
    const int64_t HW = (int64_t)H * W, NHW = HW * N;
    const bool hv = vloc != MQR_DEVICE, hi = img_loc != MQR_DEVICE, ho = out_loc != MQR_DEVICE;
    ScratchLayout L;
    float *d_v, *d_t, *hx, *hy, *d_o;
    uint8_t *d_i, *m0, *mask;
    ColorCam* dC;
    double* avg;
    int32_t* cnt;
    L.add(d_v, 3 * nv, hv);
    L.add(d_i, 3 * NHW, hi);
    L.add(d_t, NHW, hi);
    L.add(dC, N);
    L.add_each(NHW, hx, hy, m0, mask);
    L.add(avg, 3 * nv);
    L.add(cnt, nv);
    L.add(d_o, 3 * nv, ho);
    CachedBlock blk(device, L);
    const float *dV = hv ? d_v : vertices, *dT = hi ? d_t : t_hit;
    const uint8_t* dI = hi ? d_i : images;
    float* dO = ho ? d_o : colors_out;
    int rc = 0;
    auto fail = [&](const char* msg) {
        set_error(msg);
        rc = 1;
    };
    if (!blk.p)
        rc = scratch_failed("mqr_color_map", L.total());
    else if ((hv && copy_to_device(device, d_v, vertices, sizeof(float) * 3 * nv, s)) ||
             (hi && (copy_to_device(device, d_i, images, (size_t)3 * NHW, s) ||
                     copy_to_device(device, d_t, t_hit, sizeof(float) * NHW, s))) ||
             copy_to_device(device, dC, cams.data(), sizeof(ColorCam) * N, s))
        rc = 1;
    if (!rc) {
        const unsigned gv = (unsigned)((nv + 255) / 256);
        cm_enqueue_masks(s, dT, NHW, H, W, (float)depth_trunc, disc_threshold, half_dilation, hx, hy, m0, mask);
        hipLaunchKernelGGL(k_cm_vertices, dim3(gv), dim3(256), 0, s, dV, nv, dI, dT, mask, dC, N, H, W, max_depth,
                           visibility_threshold, margin, (float)depth_trunc, avg, cnt);
        if (hipGetLastError() != hipSuccess) fail("mqr_color_map: kernel launch failed");
        if (!rc) rc = cm_finish_colors(device, s, dV, nv, avg, cnt, knn, dO, "mqr_color_map");
        if (!rc && out_loc != MQR_DEVICE &&
            (copy_to_host(device, colors_out, dO, sizeof(float) * 3 * nv, s) ||
             (counts_out && copy_to_host(device, counts_out, cnt, sizeof(int32_t) * nv, s))))
            fail("mqr_color_map: copy back failed");
        if (!rc && out_loc == MQR_DEVICE && counts_out &&
            hipMemcpyAsync(counts_out, cnt, sizeof(int32_t) * nv, hipMemcpyDeviceToDevice, s) != hipSuccess)
            fail("mqr_color_map: copy failed");
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) fail("mqr_color_map: kernel failed");
    (void)hipStreamDestroy(s);
    return rc;
}

}  // extern "C"
