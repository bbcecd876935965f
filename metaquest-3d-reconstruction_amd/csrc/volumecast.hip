// volumecast.hip -- depth, vertex and normal maps of the TSDF volume by marching rays through the block
// hash (VoxelBlockGrid.ray_cast; DESIGN.md §2.10 states the rule, restated from Open3D 0.19 RayCast /
// EstimateRange as recalled, unpinned against Open3D).  Two kernels per call:
//   k_cast_range   one thread per (block, frame): the block's 8 corners through the frame's extrinsic ->
//                  [zmin, zmax] into the coarse cells its projection covers (atomicMin / atomicMax on the
//                  floats' bit patterns: positive floats order as unsigned, so the map is order-independent)
//   k_volume_cast  one lane per pixel, an 8 x 8 pixel tile per wave, grid.z = frame: a dependent gather
//                  chain (hash probe, then one 8-byte voxel per step), bound by latency and divergence; the
//                  last (key -> buffer) pair stays in registers, so steps inside one block cost no probe.
// float32 throughout, uncontracted (-ffp-contract=off), every sum in a fixed order: tests/volumecast_ref.py
// restates the rule in numpy and matches bit for bit.
#include <cmath>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "device_block.hpp"
#include "mqr_common.hpp"

namespace mqr {
namespace {

constexpr int kMaxSteps = 2048;  // march steps per ray (compile-time: the loop ends whatever the volume holds)
constexpr uint32_t kInfBits = 0x7f800000u;

struct CastVol {
    Table tab;
    const float2* pool;
    int R;
    int64_t R3;
    float voxel, block_size;
};

// (vbg_kernels.hpp's table_find, which only vbg.hip can include: its kernels are defined there)
__device__ inline int32_t find_buf(const Table t, uint64_t k) {
    const uint64_t m = (uint64_t)t.cap - 1;
    uint64_t h = mix64(k) & m;
    for (int64_t p = 0; p < t.cap; ++p) {
        const uint64_t cur = t.keys[h];
        if (cur == k) return t.vals[h];
        if (cur == kEmpty) return -1;
        h = (h + 1) & m;
    }
    return -1;
}

// The last block looked up: its buffer (< 0: absent, out of the key range or without a pool buffer).
struct BlockCache {
    int x = INT32_MIN, y = 0, z = 0;
    int32_t buf = -1;
};
__device__ __forceinline__ int32_t block_buf(const CastVol& v, BlockCache& c, int x, int y, int z) {
    if (x != c.x || y != c.y || z != c.z) {
        c.x = x;
        c.y = y;
        c.z = z;
        c.buf = key_in_range(x, y, z) ? find_buf(v.tab, pack_key(x, y, z)) : -1;
    }
    return c.buf;
}

__device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((b - 1 - a) / b); }

// Trilinear tsdf at world point p over the 8 lattice corners around it (voxel X sits at
// X * voxel), across block seams, summed in corner order c = dx + 2 dy + 4 dz.  Usable only if all 8
// corners exist with w >= wthr.
__device__ bool trilinear(const CastVol& v, BlockCache& c, float px, float py, float pz, float wthr, float& out) {
    const float gx = px / v.voxel, gy = py / v.voxel, gz = pz / v.voxel;
    const float x0 = floorf(gx), y0 = floorf(gy), z0 = floorf(gz);
    if (!(fabsf(x0) < 0x1p24f && fabsf(y0) < 0x1p24f && fabsf(z0) < 0x1p24f)) return false;
    const float fx = gx - x0, fy = gy - y0, fz = gz - z0;
    const int ix = (int)x0, iy = (int)y0, iz = (int)z0;
    float sum = 0.0f;
    for (int k = 0; k < 8; ++k) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
        const int X = ix + dx, Y = iy + dy, Z = iz + dz;
        const int bx = floor_div(X, v.R), by = floor_div(Y, v.R), bz = floor_div(Z, v.R);
        const int32_t buf = block_buf(v, c, bx, by, bz);
        if (buf < 0) return false;
        const float2 tw = v.pool[(int64_t)buf * v.R3 + ((Z - bz * v.R) * v.R + (Y - by * v.R)) * v.R + (X - bx * v.R)];
        if (!(tw.y >= wthr)) return false;
        const float wx = dx ? fx : 1.0f - fx, wy = dy ? fy : 1.0f - fy, wz = dz ? fz : 1.0f - fz;
        sum = sum + ((wx * wy) * wz) * tw.x;
    }
    out = sum;
    return true;
}

// Colour at world point p: the 8 lattice corners of trilinear() with its fractions, corner order
// and seam handling; a corner contributes r c with r = (wx wy) wz when it exists and has w > 0, and the result
// is (sum r c / sum r) / 255 per channel, 0 when the sum of r is not greater than 0.  cpool: [buf][3][R^3].
__device__ void trilinear_color(const CastVol& v, const float* __restrict__ cpool, BlockCache& c, float px, float py,
                                float pz, float (&out)[3]) {
    out[0] = out[1] = out[2] = 0.0f;
    const float gx = px / v.voxel, gy = py / v.voxel, gz = pz / v.voxel;
    const float x0 = floorf(gx), y0 = floorf(gy), z0 = floorf(gz);
    if (!(fabsf(x0) < 0x1p24f && fabsf(y0) < 0x1p24f && fabsf(z0) < 0x1p24f)) return;
    const float fx = gx - x0, fy = gy - y0, fz = gz - z0;
    const int ix = (int)x0, iy = (int)y0, iz = (int)z0;
    float S = 0.0f, acc[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 8; ++k) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
        const int X = ix + dx, Y = iy + dy, Z = iz + dz;
        const int bx = floor_div(X, v.R), by = floor_div(Y, v.R), bz = floor_div(Z, v.R);
        const int32_t buf = block_buf(v, c, bx, by, bz);
        if (buf < 0) continue;
        const int64_t vi = ((Z - bz * v.R) * v.R + (Y - by * v.R)) * v.R + (X - bx * v.R);
        if (!(v.pool[(int64_t)buf * v.R3 + vi].y > 0.0f)) continue;
        const float wx = dx ? fx : 1.0f - fx, wy = dy ? fy : 1.0f - fy, wz = dz ? fz : 1.0f - fz;
        const float r = (wx * wy) * wz;
        const float* col = cpool + (int64_t)buf * 3 * v.R3 + vi;
        S = S + r;
        for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + r * col[ch * v.R3];
    }
    if (S > 0.0f)
        for (int ch = 0; ch < 3; ++ch) out[ch] = (acc[ch] / S) / 255.0f;
}

// Cell (0 .. cells - 1) ranges, then one whole-map range per frame at cells + f (the blocks with a corner
// behind the camera: they cover every cell, so they are kept once per frame and the march folds them in).
__global__ __launch_bounds__(256) void k_cast_range(const uint64_t* __restrict__ bkeys,
                                                    const int32_t* __restrict__ keys3, int64_t nblk, CastVol v,
                                                    const FrameParams* __restrict__ fps, int H, int W, int Hc, int Wc,
                                                    int df, float dmin, float dmax, int64_t cells,
                                                    uint32_t* __restrict__ rmin, uint32_t* __restrict__ rmax) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblk) return;
    const int f = blockIdx.y;
    int kx, ky, kz;
    if (keys3) {  // listed blocks: those the volume holds
        kx = keys3[3 * i];
        ky = keys3[3 * i + 1];
        kz = keys3[3 * i + 2];
        if (!key_in_range(kx, ky, kz) || find_buf(v.tab, pack_key(kx, ky, kz)) < 0) return;
    } else {
        unpack_key(bkeys[i], kx, ky, kz);
    }
    const FrameParams& fp = fps[f];
    float ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
    int behind = 0;
    for (int c = 0; c < 8; ++c) {
        const float xs = (float)((kx + (c & 1)) * v.R) * v.voxel;
        const float ys = (float)((ky + ((c >> 1) & 1)) * v.R) * v.voxel;
        const float zs = (float)((kz + (c >> 2)) * v.R) * v.voxel;
        const float xc = xs * fp.ext[0] + ys * fp.ext[1] + zs * fp.ext[2] + fp.ext[3];
        const float yc = xs * fp.ext[4] + ys * fp.ext[5] + zs * fp.ext[6] + fp.ext[7];
        const float zc = xs * fp.ext[8] + ys * fp.ext[9] + zs * fp.ext[10] + fp.ext[11];
        zlo = fminf(zlo, zc);
        zhi = fmaxf(zhi, zc);
        if (zc > 0) {
            const float pu = fp.fx * xc / zc + fp.cx;
            const float pv = fp.fy * yc / zc + fp.cy;
            ulo = fminf(ulo, pu);
            uhi = fmaxf(uhi, pu);
            vlo = fminf(vlo, pv);
            vhi = fmaxf(vhi, pv);
        } else {
            ++behind;
        }
    }
    if (behind == 8) return;
    zlo = fminf(fmaxf(zlo, dmin), dmax);
    zhi = fminf(fmaxf(zhi, dmin), dmax);
    if (behind) zlo = dmin;
    if (!(zlo < zhi)) return;
    const uint32_t lo = __float_as_uint(zlo), hi = __float_as_uint(zhi);
    if (behind) {
        atomicMin(&rmin[cells + f], lo);
        atomicMax(&rmax[cells + f], hi);
        return;
    }
    // pixel rectangle with one pixel of slack each way (the pixel offset shifts rays by up to half a pixel)
    const float x0 = fmaxf(floorf(ulo) - 1.0f, 0.0f), x1 = fminf(floorf(uhi) + 1.0f, (float)(W - 1));
    const float y0 = fmaxf(floorf(vlo) - 1.0f, 0.0f), y1 = fminf(floorf(vhi) + 1.0f, (float)(H - 1));
    if (!(x0 <= x1 && y0 <= y1)) return;
    const int cx0 = (int)x0 / df, cx1 = (int)x1 / df, cy0 = (int)y0 / df, cy1 = (int)y1 / df;
    uint32_t* mn = rmin + (int64_t)f * Hc * Wc;
    uint32_t* mx = rmax + (int64_t)f * Hc * Wc;
    for (int cy = cy0; cy <= cy1 && cy < Hc; ++cy)
        for (int cx = cx0; cx <= cx1 && cx < Wc; ++cx) {
            atomicMin(&mn[cy * Wc + cx], lo);
            atomicMax(&mx[cy * Wc + cx], hi);
        }
}

// 256 threads = four waves, wave w the 8 x 8 pixel tile (w % 2, w / 2) of a 16 x 16 pixel square.
// COLOR: a coloured volume asked for its colour map (cpool, color); the instantiation without compiles none of it.
template <bool COLOR>
__global__ __launch_bounds__(256) void k_volume_cast(CastVol v, const FrameParams* __restrict__ fps, int H, int W,
                                                     int Hc, int Wc, int df, int64_t cells,
                                                     const uint32_t* __restrict__ rmin,
                                                     const uint32_t* __restrict__ rmax, float off, float depth_scale,
                                                     float wthr, float sdf_trunc, int refine,
                                                     float* __restrict__ depth, float* __restrict__ vertex,
                                                     float* __restrict__ normal, const float* __restrict__ cpool,
                                                     float* __restrict__ color) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= W || y >= H) return;
    const int f = blockIdx.z;
    const FrameParams& fp = fps[f];
    const int64_t pix = ((int64_t)f * H + y) * W + x;

    const float xc = (((float)x + off) - fp.cx) / fp.fx;
    const float yc = (((float)y + off) - fp.cy) / fp.fy;
    const float ox = fp.pose[3], oy = fp.pose[7], oz = fp.pose[11];
    const float dx = (xc * fp.pose[0] + yc * fp.pose[1] + fp.pose[2] + fp.pose[3]) - ox;
    const float dy = (xc * fp.pose[4] + yc * fp.pose[5] + fp.pose[6] + fp.pose[7]) - oy;
    const float dz = (xc * fp.pose[8] + yc * fp.pose[9] + fp.pose[10] + fp.pose[11]) - oz;

    const int64_t cell = ((int64_t)f * Hc + y / df) * Wc + x / df;
    const float zmin = fminf(__uint_as_float(rmin[cell]), __uint_as_float(rmin[cells + f]));
    const float zmax = fmaxf(__uint_as_float(rmax[cell]), __uint_as_float(rmax[cells + f]));

    BlockCache bc;
    float t = zmin, t_prev = zmin, tsdf_prev = -1.0f, tsdf = 1.0f;
    float px = 0.f, py = 0.f, pz = 0.f;
    bool hit = false;
    if (zmin < zmax) {
        for (int s = 0; s < kMaxSteps && t < zmax; ++s) {
            px = ox + t * dx;
            py = oy + t * dy;
            pz = oz + t * dz;
            const float bxf = floorf(px / v.block_size), byf = floorf(py / v.block_size),
                        bzf = floorf(pz / v.block_size);
            const float lim = (float)kBias;
            int32_t buf = -1;
            int bx = 0, by = 0, bz = 0;
            if (bxf >= -lim && bxf < lim && byf >= -lim && byf < lim && bzf >= -lim && bzf < lim) {
                bx = (int)bxf;
                by = (int)byf;
                bz = (int)bzf;
                buf = block_buf(v, bc, bx, by, bz);
            }
            if (buf < 0) {
                t += v.block_size;
                tsdf_prev = tsdf;
                continue;
            }
            const float rm1 = (float)(v.R - 1);
            const int vx = (int)fminf(fmaxf(floorf((px - bxf * v.block_size) / v.voxel), 0.0f), rm1);
            const int vy = (int)fminf(fmaxf(floorf((py - byf * v.block_size) / v.voxel), 0.0f), rm1);
            const int vz = (int)fminf(fmaxf(floorf((pz - bzf * v.block_size) / v.voxel), 0.0f), rm1);
            const float2 tw = v.pool[(int64_t)buf * v.R3 + (vz * v.R + vy) * v.R + vx];
            tsdf = tw.x;
            if (tsdf_prev > 0 && tw.y >= wthr && tsdf <= 0) {
                hit = true;
                break;
            }
            tsdf_prev = tsdf;
            t_prev = t;
            t += fmaxf(tsdf * sdf_trunc, v.voxel);
        }
    }

    float ts = 0.f;
    if (hit) {
        ts = (t * tsdf_prev - t_prev * tsdf) / (tsdf_prev - tsdf);
        if (refine) {
            float a = 0.f, b = 0.f;
            const bool oka = trilinear(v, bc, ox + t_prev * dx, oy + t_prev * dy, oz + t_prev * dz, wthr, a);
            const bool okb = trilinear(v, bc, px, py, pz, wthr, b);
            if (oka && okb && a > 0 && b <= 0) ts = (t * a - t_prev * b) / (a - b);
        }
    }
    const float hx = ox + ts * dx, hy = oy + ts * dy, hz = oz + ts * dz;
    if (depth) depth[pix] = hit ? ts * depth_scale : 0.0f;
    if (vertex) {
        vertex[3 * pix + 0] = hit ? hx : 0.0f;
        vertex[3 * pix + 1] = hit ? hy : 0.0f;
        vertex[3 * pix + 2] = hit ? hz : 0.0f;
    }
    if (normal) {
        float n[3] = {0.f, 0.f, 0.f};
        if (hit) {
            float s[6];
            bool ok = true;
            for (int k = 0; k < 6 && ok; ++k) {
                const float e = (k & 1) ? -v.voxel : v.voxel;
                ok = trilinear(v, bc, k >> 1 == 0 ? hx + e : hx, k >> 1 == 1 ? hy + e : hy, k >> 1 == 2 ? hz + e : hz,
                               wthr, s[k]);
            }
            if (ok) {
                const float nx = s[0] - s[1], ny = s[2] - s[3], nz = s[4] - s[5];
                // (k_pt_emit's normalisation: extract.hip write_normal)
                const float norm = (float)((double)sqrtf(nx * nx + ny * ny + nz * nz) + 1e-5);
                n[0] = nx / norm;
                n[1] = ny / norm;
                n[2] = nz / norm;
            }
        }
        normal[3 * pix + 0] = n[0];
        normal[3 * pix + 1] = n[1];
        normal[3 * pix + 2] = n[2];
    }
    if constexpr (COLOR) {
        float c[3] = {0.f, 0.f, 0.f};
        if (hit) trilinear_color(v, cpool, bc, hx, hy, hz, c);
        color[3 * pix + 0] = c[0];
        color[3 * pix + 1] = c[1];
        color[3 * pix + 2] = c[2];
    }
}

// The last call's device times per device (as the other *_last_ms entry points keep them), and timing events
// lent to one call at a time: a call records its own three on its volume's stream, so casts of two volumes on
// one device never share an event.  Returned events are reused (creating one costs more than a small cast).
struct CastTimes {
    double range_ms = 0.0, march_ms = 0.0;
};
std::mutex g_times_mu;
CastTimes g_times[kMaxDevices];
std::vector<hipEvent_t> g_free_events[kMaxDevices];

struct CastEvents {
    int device;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    explicit CastEvents(int d) : device(d) {}
    bool take() {
        std::lock_guard<std::mutex> lk(g_times_mu);
        for (hipEvent_t& e : ev) {
            if (!g_free_events[device].empty()) {
                e = g_free_events[device].back();
                g_free_events[device].pop_back();
            } else if (hipEventCreate(&e) != hipSuccess) {
                e = nullptr;
                return false;
            }
        }
        return true;
    }
    ~CastEvents() {  // (the owner has drained its stream: the events are complete)
        std::lock_guard<std::mutex> lk(g_times_mu);
        for (hipEvent_t e : ev)
            if (e) g_free_events[device].push_back(e);
    }
};

struct CastScratch {
    uint32_t *rmin, *rmax;
    FrameParams* fp;
    int32_t* keys;
};

int cast_scratch(mqr_vbg* v, int64_t cells, int n, int64_t host_keys, CastScratch& s) {
    ScratchLayout L;
    L.add_each(cells + n, s.rmin, s.rmax);
    L.add(s.fp, n);
    L.add(s.keys, 3 * host_keys, host_keys > 0);
    MQR_REQUIRE(L.valid(), "ray_cast: scratch size out of range");
    const size_t need = L.total();
    if (v->ex_scratch_bytes < need) {  // the volume's grow-only scratch (shared with the extraction, same stream)
        MQR_CHECK_HIP(hipStreamSynchronize(v->stream));
        GrowBuf b{v->ex_scratch, v->ex_scratch_bytes};
        const hipError_t grown = b.reserve(need, need + need / 4);
        v->ex_scratch = b.p;
        v->ex_scratch_bytes = b.cap;
        if (grown != hipSuccess) return scratch_failed("ray_cast", need);
    }
    L.bind(v->ex_scratch);
    return 0;
}

bool finite_all(const double* a, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

}  // namespace
}  // namespace mqr

using namespace mqr;

extern "C" {

int mqr_vbg_ray_cast_color(mqr_vbg* v, const int32_t* block_keys, int64_t n_keys, int keys_loc, const double* K,
                           const double* T_wc, int n, int H, int W, float depth_scale, float depth_min,
                           float depth_max, float weight_threshold, float trunc_voxel_multiplier,
                           int range_map_down_factor, float pixel_offset, int flags, float* depth, float* vertex,
                           float* normal, float* color, int out_loc) {
    MQR_REQUIRE(v && K && T_wc, "ray_cast: null argument");
    MQR_REQUIRE(!color || v->has_color, "ray_cast: the volume carries no colour");
    MQR_REQUIRE(n > 0 && n <= 65535, "ray_cast: the frame count must be in [1, 65535], got " + std::to_string(n));
    MQR_REQUIRE(H > 0 && W > 0, "ray_cast: height and width must be positive");
    MQR_REQUIRE(range_map_down_factor > 0, "ray_cast: range_map_down_factor must be positive");
    MQR_REQUIRE(depth_min >= 0, "ray_cast: depth_min must be >= 0");  // (a NaN fails both tests)
    MQR_REQUIRE(depth_max > depth_min && std::isfinite(depth_max), "ray_cast: depth_max must be finite and > depth_min");
    MQR_REQUIRE(finite_all(K, (int64_t)n * 9) && finite_all(T_wc, (int64_t)n * 16), "ray_cast: non-finite K or T_wc");
    MQR_REQUIRE(depth || vertex || normal || color, "ray_cast: all outputs are null");
    MQR_REQUIRE(n_keys >= 0 && (n_keys == 0 || block_keys), "ray_cast: block keys missing");
    MQR_REQUIRE((keys_loc == MQR_HOST || keys_loc == MQR_DEVICE) && (out_loc == MQR_HOST || out_loc == MQR_DEVICE),
                "ray_cast: a location must be MQR_HOST or MQR_DEVICE");
    MQR_REQUIRE(std::isfinite(depth_scale) && std::isfinite(weight_threshold) && std::isfinite(pixel_offset) &&
                    std::isfinite(trunc_voxel_multiplier),
                "ray_cast: non-finite parameter");
    std::vector<FrameParams> fp((size_t)n);
    for (int f = 0; f < n; ++f) {
        make_frame_params(K + 9 * (int64_t)f, T_wc + 16 * (int64_t)f, &fp[f]);
        MQR_REQUIRE(fp[f].fx != 0.0f && fp[f].fy != 0.0f, "ray_cast: fx and fy must not be 0 (frame " + std::to_string(f) + ")");
    }
    const int df = range_map_down_factor;
    const int Hc = (H + df - 1) / df, Wc = (W + df - 1) / df;
    const int64_t cells = (int64_t)n * Hc * Wc, npix = (int64_t)n * H * W;
    const int64_t tiles_y = (H + 15) / 16;
    MQR_REQUIRE(tiles_y <= 65535, "ray_cast: height exceeds the launch grid");

    MQR_CHECK_HIP(hipSetDevice(v->device));
    MQR_REQUIRE(v->device >= 0 && v->device < kMaxDevices, "device index out of range");
    if (order_after_integrate(v)) return 1;  // an integrate may still be running on the second stream
    const bool dev_keys = block_keys && keys_loc == MQR_DEVICE;
    if ((dev_keys || out_loc == MQR_DEVICE) && order_after_caller(v->device, v->stream)) return 2;
    hipStream_t st = v->stream;

    CastScratch s{};
    if (cast_scratch(v, cells, n, block_keys && !dev_keys ? n_keys : 0, s)) return 1;
    // host outputs: staged in a block of the process's device-block cache, returned at the end of the call
    float *d_depth = depth, *d_vertex = vertex, *d_normal = normal, *d_color = color;
    ScratchLayout O;
    const bool stage = out_loc == MQR_HOST;
    O.add(d_depth, npix, stage && depth);
    O.add(d_vertex, 3 * npix, stage && vertex);
    O.add(d_normal, 3 * npix, stage && normal);
    O.add(d_color, 3 * npix, stage && color);
    if (!stage) {
        d_depth = depth;
        d_vertex = vertex;
        d_normal = normal;
        d_color = color;
    }
    CastEvents tm(v->device);  // (declared before `drain`: the events go back after the stream is drained)
    if (!tm.take()) {
        (void)hipGetLastError();
        set_error("ray_cast: cannot create timing events");
        return 1;
    }
    std::optional<CachedBlock> out_blk;
    if (stage) out_blk.emplace(v->device, O);
    StreamDrain drain{st};
    if (stage && !out_blk->p) return scratch_failed("ray_cast", O.total());

    if (copy_to_device(v->device, s.fp, fp.data(), sizeof(FrameParams) * (size_t)n, st)) return 1;
    const int32_t* d_keys = nullptr;
    if (block_keys) {
        if (dev_keys) {
            d_keys = block_keys;
        } else {
            if (copy_to_device(v->device, s.keys, block_keys, sizeof(int32_t) * 3 * (size_t)n_keys, st)) return 1;
            d_keys = s.keys;
        }
    }
    CastVol cv{v->tab, v->pool, v->R, v->R3, v->voxel_size, v->voxel_size * (float)v->R};
    const float sdf_trunc = v->voxel_size * trunc_voxel_multiplier;
    MQR_CHECK_HIP(hipEventRecord(tm.ev[0], st));
    MQR_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s.rmin), (int)kInfBits, (size_t)(cells + n), st));
    MQR_CHECK_HIP(hipMemsetAsync(s.rmax, 0, sizeof(uint32_t) * (size_t)(cells + n), st));
    const int64_t nblk = block_keys ? n_keys : v->pool_count;
    if (nblk > 0 && v->pool_count > 0) {
        hipLaunchKernelGGL(k_cast_range, dim3((unsigned)((nblk + 255) / 256), (unsigned)n), dim3(256), 0, st, v->bkeys,
                           d_keys, nblk, cv, s.fp, H, W, Hc, Wc, df, depth_min, depth_max, cells, s.rmin, s.rmax);
        MQR_CHECK_HIP(hipGetLastError());
    }
    MQR_CHECK_HIP(hipEventRecord(tm.ev[1], st));
    hipLaunchKernelGGL(color ? k_volume_cast<true> : k_volume_cast<false>,
                       dim3((unsigned)((W + 15) / 16), (unsigned)tiles_y, (unsigned)n), dim3(256), 0, st, cv, s.fp, H, W,
                       Hc, Wc, df, cells, s.rmin, s.rmax, pixel_offset, depth_scale, weight_threshold, sdf_trunc,
                       flags & MQR_CAST_REFINE, d_depth, d_vertex, d_normal, (const float*)v->cpool, d_color);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(hipEventRecord(tm.ev[2], st));
    if (stage) {
        if (depth && copy_to_host(v->device, depth, d_depth, sizeof(float) * (size_t)npix, st)) return 1;
        if (vertex && copy_to_host(v->device, vertex, d_vertex, sizeof(float) * 3 * (size_t)npix, st)) return 1;
        if (normal && copy_to_host(v->device, normal, d_normal, sizeof(float) * 3 * (size_t)npix, st)) return 1;
        if (color && copy_to_host(v->device, color, d_color, sizeof(float) * 3 * (size_t)npix, st)) return 1;
    }
    MQR_CHECK_HIP(hipStreamSynchronize(st));
    // the outputs are complete: a failed time query loses the times, not the call
    float r = 0.f, m = 0.f;
    if (hipEventElapsedTime(&r, tm.ev[0], tm.ev[1]) != hipSuccess || hipEventElapsedTime(&m, tm.ev[1], tm.ev[2]) != hipSuccess) {
        (void)hipGetLastError();
        r = m = 0.f;
    }
    std::lock_guard<std::mutex> lk(g_times_mu);
    g_times[v->device].range_ms = r;
    g_times[v->device].march_ms = m;
    return 0;
}

int mqr_vbg_ray_cast(mqr_vbg* v, const int32_t* block_keys, int64_t n_keys, int keys_loc, const double* K,
                     const double* T_wc, int n, int H, int W, float depth_scale, float depth_min, float depth_max,
                     float weight_threshold, float trunc_voxel_multiplier, int range_map_down_factor,
                     float pixel_offset, int flags, float* depth, float* vertex, float* normal, int out_loc) {
    return mqr_vbg_ray_cast_color(v, block_keys, n_keys, keys_loc, K, T_wc, n, H, W, depth_scale, depth_min, depth_max,
                                  weight_threshold, trunc_voxel_multiplier, range_map_down_factor, pixel_offset, flags,
                                  depth, vertex, normal, nullptr, out_loc);
}

int mqr_vbg_ray_cast_last_ms(mqr_vbg* v, double* range_ms, double* march_ms) {
    MQR_REQUIRE(v && v->device >= 0 && v->device < kMaxDevices, "ray_cast_last_ms: null volume");
    std::lock_guard<std::mutex> lk(g_times_mu);
    if (range_ms) *range_ms = g_times[v->device].range_ms;
    if (march_ms) *march_ms = g_times[v->device].march_ms;
    return 0;
}

}  // extern "C"
