// colorframes.hip -- device-side colour-frame ingestion: Quest camera frames (Android YUV_420_888, as
// stored in <side>_camera_raw/<ts>.yuv) -> (N,H,W,3) uint8 RGB / BGR, the layout color.hip and colormap.hip
// read, plus the two per-frame statistics the reference's frame filter needs.  The colour twin of ingest.hip.
//
//   convert_yuv420_888_to_i420 / _to_bgr             scripts/utils/image_utils.py:6-71
//   is_blur_image / is_over_or_under_exposed         scripts/utils/image_utils.py:74-90
//   process_file / FilterFn                          scripts/processing/yuv_conversion/convert_yuv_dir.py:15-54
//
// The plane layout arrives resolved (mqr_yuv_layout; mqr/colorframes.py's resolve_layout turns the
// reference's three unpacking branches into it, quirks included), so the kernel only addresses bytes.  The
// colour arithmetic lives in color_convert.hpp (restated from OpenCV as recalled: parity unpinned).
//
// Two kernels:
//   k_decode_color   one thread per 4 horizontal pixels x 2 rows: two chroma pairs, eight Y, and per row four
//                    pixels = 12 bytes = three dwords.  WIDE: dword Y loads and 12-byte stores, CHROMA4: one
//                    dword for the two interleaved (U,V) pairs -- both only when every address involved is
//                    4-byte aligned (the host decides from the pointers and strides); otherwise byte accesses,
//                    which are correct for any base, stride and even width.
//   k_frame_stats    a second pass over the just-written image, launched only when statistics are asked for:
//                    a workgroup walks 64x16 tiles of one frame, each with its one-pixel reflect-101 halo of
//                    grey values in LDS; the blue histogram builds up in LDS and the Laplacian sums in
//                    registers, flushed once per workgroup: one global atomic per non-empty bin and two for
//                    the sums.  Integer atomics only: every output is independent of order.
#include <algorithm>
#include <mutex>

#include "color_convert.hpp"
#include "device_block.hpp"
#include "mqr_common.hpp"

namespace mqr {

struct alignas(4) Px4 {  // four packed 3-byte pixels
    uint32_t a, b, c;
};

// r | g << 8 | b << 16 of four pixels -> 12 bytes in RGB or BGR order
__device__ __forceinline__ Px4 pack4(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, bool bgr) {
    if (bgr) {
        auto sw = [](uint32_t p) { return (p & 0x00ff00u) | (p >> 16) | (p & 0xffu) << 16; };
        p0 = sw(p0), p1 = sw(p1), p2 = sw(p2), p3 = sw(p3);
    }
    return {p0 | p1 << 24, p1 >> 8 | p2 << 16, p2 >> 16 | p3 << 8};
}

template <bool WIDE, bool CHROMA4>
__global__ __launch_bounds__(256) void k_decode_color(const uint8_t* __restrict__ raw, int64_t frame_stride,
                                                      mqr_yuv_layout L, int W, int H, int bgr,
                                                      uint8_t* __restrict__ out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;   // 4-pixel group in the row
    const int rp = blockIdx.y * blockDim.y + threadIdx.y;  // row pair
    const int f = blockIdx.z;
    if (4 * g >= W || 2 * rp >= H) return;
    const uint8_t* fr = raw + (int64_t)f * frame_stride;
    const int npx = min(4, W - 4 * g);  // 4, or 2 in the last group of a width that is 2 mod 4
    // ---- the two chroma pairs of this group
    int U[2], V[2];
    if (CHROMA4) {  // U V U V (or V U V U) in one aligned dword
        const bool u_first = L.u_base < L.v_base;
        const uint32_t c =
            *reinterpret_cast<const uint32_t*>(fr + (u_first ? L.u_base : L.v_base) + (int64_t)rp * L.u_row_stride + 4 * g);
        const int a0 = c & 0xff, b0 = (c >> 8) & 0xff, a1 = (c >> 16) & 0xff, b1 = c >> 24;
        U[0] = u_first ? a0 : b0, V[0] = u_first ? b0 : a0;
        U[1] = u_first ? a1 : b1, V[1] = u_first ? b1 : a1;
    } else {
        const uint8_t* up = fr + L.u_base + (int64_t)rp * L.u_row_stride + (int64_t)(2 * g) * L.u_step;
        const uint8_t* vp = fr + L.v_base + (int64_t)rp * L.v_row_stride + (int64_t)(2 * g) * L.v_step;
        U[0] = up[0], V[0] = vp[0];
        U[1] = npx > 2 ? up[L.u_step] : 0, V[1] = npx > 2 ? vp[L.v_step] : 0;
    }
    const cc::Chroma c0 = cc::chroma_terms(U[0], V[0]), c1 = cc::chroma_terms(U[1], V[1]);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 2 * rp + r;
        const uint8_t* yp = fr + L.y_base + (int64_t)row * L.y_row_stride + (int64_t)(4 * g) * L.y_pixel_stride;
        uint8_t* op = out + (((int64_t)f * H + row) * W + 4 * g) * 3;
        if (WIDE) {
            const uint32_t y = *reinterpret_cast<const uint32_t*>(yp);
            *reinterpret_cast<Px4*>(op) =
                pack4(cc::yuv_to_rgb(y & 0xff, c0), cc::yuv_to_rgb((y >> 8) & 0xff, c0),
                      cc::yuv_to_rgb((y >> 16) & 0xff, c1), cc::yuv_to_rgb(y >> 24, c1), bgr != 0);
        } else {
            for (int k = 0; k < npx; ++k) {
                const uint32_t p = cc::yuv_to_rgb(yp[(int64_t)k * L.y_pixel_stride], k < 2 ? c0 : c1);
                const uint8_t cr = p & 0xff, cg = (p >> 8) & 0xff, cb = p >> 16;
                op[3 * k + 0] = bgr ? cb : cr;
                op[3 * k + 1] = cg;
                op[3 * k + 2] = bgr ? cr : cb;
            }
        }
    }
}

// ---- statistics pass
constexpr int kTileW = 64, kTileH = 16;  // pixels per tile: one wave per row, four rows per wave
// Workgroups per frame: about kStatsGroups in all, at most kStatsGroupsPerFrame of one frame.  Each walks its
// share of the frame's tiles and flushes ONCE: 258 device atomics per workgroup, which all land on the
// frame's 258 words.  (A workgroup per tile -- 1200 per 1280x960 frame -- made those words the bottleneck:
// the pass took nine times the decode.)
constexpr int kStatsGroups = 2048, kStatsGroupsPerFrame = 256;

__global__ __launch_bounds__(256) void k_frame_stats(const uint8_t* __restrict__ img, int W, int H, int bgr,
                                                     uint32_t* __restrict__ hist, unsigned long long* __restrict__ sums) {
    __shared__ int16_t grey[kTileH + 2][kTileW + 2];
    __shared__ uint32_t lhist[256];
    __shared__ unsigned long long wg_sum[2];
    const int tid = threadIdx.x, f = blockIdx.y;
    const uint8_t* im = img + (int64_t)f * H * W * 3;
    lhist[tid] = 0;
    if (tid < 2) wg_sum[tid] = 0;
    const bool want_hist = hist != nullptr;
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles = tiles_x * ((H + kTileH - 1) / kTileH);
    long long s1 = 0, s2 = 0;  // this thread's share of the Laplacian sums, over all its tiles
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int x0 = (t % tiles_x) * kTileW, y0 = (t / tiles_x) * kTileH;
        __syncthreads();  // the previous tile's grey values are read (and lhist is cleared)
        // the tile with its halo: grey of every position whose reflected pixel exists, blue counted for the interior
        for (int i = tid; i < (kTileH + 2) * (kTileW + 2); i += 256) {
            const int ly = i / (kTileW + 2), lx = i - ly * (kTileW + 2);
            const int gy = y0 + ly - 1, gx = x0 + lx - 1;
            if (gy > H || gx > W) continue;  // beyond the halo of the last row / column: never read back
            const int sy = cc::reflect101(gy, H), sx = cc::reflect101(gx, W);
            const uint8_t* p = im + ((int64_t)sy * W + sx) * 3;
            const int c0 = p[0], c1 = p[1], c2 = p[2];
            const int r = bgr ? c2 : c0, b = bgr ? c0 : c2;
            grey[ly][lx] = (int16_t)cc::grey_of(r, c1, b);
            if (want_hist && ly >= 1 && ly <= kTileH && lx >= 1 && lx <= kTileW && gy < H && gx < W)
                atomicAdd(&lhist[b], 1u);
        }
        __syncthreads();
        const int lx = (tid & 63) + 1;
        if (sums && x0 + lx - 1 < W) {
            for (int ly = (tid >> 6) + 1; ly <= kTileH && y0 + ly - 1 < H; ly += 4) {
                const int v = grey[ly - 1][lx] + grey[ly + 1][lx] + grey[ly][lx - 1] + grey[ly][lx + 1] - 4 * grey[ly][lx];
                s1 += v;
                s2 += v * v;
            }
        }
    }
    if (sums) {
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o, 64);
            s2 += __shfl_xor(s2, o, 64);
        }
        // two's complement: adding the sign-extended sum to the unsigned word is the signed addition
        if ((tid & 63) == 0) {
            atomicAdd(&wg_sum[0], (unsigned long long)s1);
            atomicAdd(&wg_sum[1], (unsigned long long)s2);
        }
    }
    __syncthreads();
    if (want_hist && lhist[tid]) atomicAdd(&hist[(int64_t)f * 256 + tid], lhist[tid]);
    if (sums && tid < 2 && wg_sum[tid]) atomicAdd(&sums[2 * (int64_t)f + tid], wg_sum[tid]);
}

// Per-device context, as ingest.hip's: a stream, grow-only scratch (staged input / output) and the
// statistics words.  Calls on one device serialise on the mutex.
struct ColorCtx {
    std::mutex mu;
    hipStream_t s = nullptr;
    GrowBuf scratch, stats;
    // events around the last call's two kernels (mqr_color_frames_last_ms); timed[1]: the statistics ran
    hipEvent_t ev[3] = {};
    bool timed[2] = {false, false};
};
static ColorCtx g_color[kMaxDevices];

// Every byte the kernels read lies in [0, valid_bytes) of its frame: checked here, from the sizes alone.
static bool plane_fits(int64_t base, int64_t row_stride, int64_t step, int rows, int cols, int64_t valid) {
    if (base < 0 || row_stride < 0 || step < 0) return false;
    // (operands bounded by 2^31 * 2^31 would overflow: the strides of a real frame are far smaller)
    if (row_stride > (int64_t(1) << 31) || step > (int64_t(1) << 31)) return false;
    const int64_t last = base + (int64_t)(rows - 1) * row_stride + (int64_t)(cols - 1) * step;
    return last < valid;
}

}  // namespace mqr

using namespace mqr;

extern "C" {

int mqr_color_constants(int32_t* out, int n) {
    MQR_REQUIRE(out && n == MQR_COLOR_CONSTANTS, "mqr_color_constants: out[MQR_COLOR_CONSTANTS]");
    const int32_t c[MQR_COLOR_CONSTANTS] = {cc::kCY,    cc::kCUB,   cc::kCUG,   cc::kCVG,      cc::kCVR, cc::kYuvShift,
                                            cc::kGreyB, cc::kGreyG, cc::kGreyR, cc::kGreyShift};
    std::copy(c, c + MQR_COLOR_CONSTANTS, out);
    return 0;
}

int mqr_decode_color_frames(int device, const uint8_t* raw, int raw_loc, int N, int64_t frame_stride, int W, int H,
                            const mqr_yuv_layout* layout, int bgr, uint8_t* rgb_out, int out_loc, uint32_t* hist,
                            int64_t* lap_sums) {
    MQR_REQUIRE(raw && layout && rgb_out, "null argument");
    MQR_REQUIRE(N >= 0 && N <= 65535, "frame count out of range (0..65535 per call)");
    MQR_REQUIRE(W > 0 && H > 0 && W % 2 == 0 && H % 2 == 0, "frame width and height must be even and positive");
    MQR_REQUIRE(W <= (1 << 20) && H <= (1 << 19), "frame too large");
    MQR_REQUIRE(device >= 0 && device < kMaxDevices, "device index out of range");
    const mqr_yuv_layout L = *layout;
    MQR_REQUIRE(L.valid_bytes > 0 && (N <= 1 || (frame_stride >= L.valid_bytes)),
                "frame stride smaller than the frame's valid bytes");
    MQR_REQUIRE(plane_fits(L.y_base, L.y_row_stride, L.y_pixel_stride, H, W, L.valid_bytes) &&
                    plane_fits(L.u_base, L.u_row_stride, L.u_step, H / 2, W / 2, L.valid_bytes) &&
                    plane_fits(L.v_base, L.v_row_stride, L.v_step, H / 2, W / 2, L.valid_bytes),
                "plane layout reads past the frame's valid bytes");
    if (N == 0) return 0;
    MQR_CHECK_HIP(hipSetDevice(device));
    ColorCtx& c = g_color[device];
    std::lock_guard<std::mutex> lock(c.mu);
    if (!c.s) {
        MQR_CHECK_HIP(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking));
        for (hipEvent_t& e : c.ev) MQR_CHECK_HIP(hipEventCreate(&e));
    }
    c.timed[0] = c.timed[1] = false;
    const bool stage_raw = raw_loc != MQR_DEVICE, stage_out = out_loc != MQR_DEVICE, stats = hist || lap_sums;
    const size_t in_bytes = (size_t)(N - 1) * (size_t)frame_stride + (size_t)L.valid_bytes;
    const size_t out_bytes = (size_t)N * H * W * 3;
    ScratchLayout scr, sts;
    uint8_t *s_raw, *s_out;
    uint32_t* d_hist;
    unsigned long long* d_sums;
    scr.add(s_raw, (int64_t)in_bytes, stage_raw);
    scr.add(s_out, (int64_t)out_bytes, stage_out);
    sts.add(d_hist, 256 * (int64_t)N, hist != nullptr);
    sts.add(d_sums, 2 * (int64_t)N, lap_sums != nullptr);
    MQR_REQUIRE(scr.valid() && sts.valid(), "bad frame shape");
    if (scr.total() > c.scratch.cap) {
        MQR_CHECK_HIP(hipStreamSynchronize(c.s));
        MQR_CHECK_HIP(c.scratch.reserve(scr.total(), scr.total()));
    }
    if (sts.total() > c.stats.cap) {
        MQR_CHECK_HIP(hipStreamSynchronize(c.s));
        MQR_CHECK_HIP(c.stats.reserve(sts.total(), sts.total()));
    }
    scr.bind(c.scratch.p);
    sts.bind(c.stats.p);
    if ((!stage_raw || !stage_out) && order_after_caller(device, c.s)) return 2;
    const uint8_t* d_raw = stage_raw ? s_raw : raw;
    if (stage_raw && copy_to_device(device, s_raw, raw, in_bytes, c.s)) return 1;
    uint8_t* d_out = stage_out ? s_out : rgb_out;

    auto al4 = [](int64_t v) { return (v & 3) == 0; };
    const bool frames4 = N == 1 || al4(frame_stride);
    const bool wide = W % 4 == 0 && frames4 && L.y_pixel_stride == 1 && al4(L.y_row_stride) &&
                      al4((int64_t)reinterpret_cast<uintptr_t>(d_raw) + L.y_base) &&
                      al4((int64_t)reinterpret_cast<uintptr_t>(d_out));
    const int64_t c_base = std::min(L.u_base, L.v_base);
    const bool chroma4 = W % 4 == 0 && frames4 && L.u_step == 2 && L.v_step == 2 &&
                         (L.u_base - L.v_base == 1 || L.v_base - L.u_base == 1) && L.u_row_stride == L.v_row_stride &&
                         al4(L.u_row_stride) && al4((int64_t)reinterpret_cast<uintptr_t>(d_raw) + c_base);
    MQR_CHECK_HIP(hipEventRecord(c.ev[0], c.s));
    const dim3 block(64, 4);
    const dim3 grid((unsigned)(((W + 3) / 4 + 63) / 64), (unsigned)((H / 2 + 3) / 4), (unsigned)N);
#define MQR_LAUNCH_DECODE(WD, C4)                                                                              \
    hipLaunchKernelGGL((k_decode_color<WD, C4>), grid, block, 0, c.s, d_raw, frame_stride, L, W, H, bgr, d_out)
    if (wide && chroma4)
        MQR_LAUNCH_DECODE(true, true);
    else if (wide)
        MQR_LAUNCH_DECODE(true, false);
    else if (chroma4)
        MQR_LAUNCH_DECODE(false, true);
    else
        MQR_LAUNCH_DECODE(false, false);
#undef MQR_LAUNCH_DECODE
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(hipEventRecord(c.ev[1], c.s));
    if (stats) {
        MQR_CHECK_HIP(hipMemsetAsync(c.stats.p, 0, sts.total(), c.s));
        const int tiles = ((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH);
        const int per_frame = std::min({tiles, kStatsGroupsPerFrame, std::max(1, (kStatsGroups + N - 1) / N)});
        const dim3 sgrid((unsigned)per_frame, (unsigned)N);
        hipLaunchKernelGGL(k_frame_stats, sgrid, dim3(256), 0, c.s, d_out, W, H, bgr, d_hist, d_sums);
        MQR_CHECK_HIP(hipGetLastError());
        MQR_CHECK_HIP(hipEventRecord(c.ev[2], c.s));
        if (hist && copy_to_host(device, hist, d_hist, sizeof(uint32_t) * 256 * N, c.s)) return 1;
        if (lap_sums && copy_to_host(device, lap_sums, d_sums, sizeof(int64_t) * 2 * N, c.s)) return 1;
    }
    if (stage_out && copy_to_host(device, rgb_out, d_out, out_bytes, c.s)) return 1;
    MQR_CHECK_HIP(hipStreamSynchronize(c.s));
    c.timed[0] = true;
    c.timed[1] = stats;
    return 0;
}

int mqr_color_frames_last_ms(int device, float* decode_ms, float* stats_ms) {
    MQR_REQUIRE(decode_ms && stats_ms, "null argument");
    MQR_REQUIRE(device >= 0 && device < kMaxDevices, "device index out of range");
    ColorCtx& c = g_color[device];
    std::lock_guard<std::mutex> lock(c.mu);
    MQR_REQUIRE(c.timed[0], "no completed mqr_decode_color_frames call on this device");
    *stats_ms = 0.0f;
    MQR_CHECK_HIP(hipEventElapsedTime(decode_ms, c.ev[0], c.ev[1]));
    if (c.timed[1]) MQR_CHECK_HIP(hipEventElapsedTime(stats_ms, c.ev[1], c.ev[2]));
    return 0;
}

}  // extern "C"
