// meshsimplify.hip -- vertex clustering of a triangle mesh (TriangleMesh.simplify_vertex_clustering, Average).
//
// Reference: scripts/downsample_fbx_mesh.py:129-283 reduces a coloured mesh with Open3D's
// simplify_vertex_clustering(voxel_size, Average).  The rule is restated from Open3D's SimplifyVertexClustering
// as recalled (unpinned); where Open3D's result depends on the iteration order of its hash
// containers, the order here is this package's own.  Everything is float64 on the widened float32 inputs:
//   origin    (double)min_bound - voxel_size * 0.5 per axis;
//   cell(i)   floor(((double)p_i - origin) / voxel_size) per axis;
//   vertex j  the j-th distinct cell in order of first appearance over i = 0 .. nv - 1, map[i] = j;
//   position  the members' values summed in ascending input index, divided by (double)count, rounded to
//             float32; normals and colours the same way (neither renormalised nor clamped);
//   triangle  (a, b, c) = map[corners]; dropped when two are equal; rotated so the smallest comes first; dropped
//             when the same rotated triple occurred at a lower input index; survivors keep input order.
// Passes: checks (device_prims.hpp, before anything gathers through an index), bounds, cell keys + iota, a
// stable radix sort of (key, index) over the bits in use, segment heads, the "first of its cell" flags scanned
// in input order, ONE THREAD PER CELL summing its members in ascending index (the sort is stable, so that is
// the order they lie in; a cell of 10^5 members is slow by construction -- the price of the bit-exact sum),
// then the triangle remap into packed triples, their stable sort, the heads test and the compaction.  With
// fewer than 2^21 output vertices a triple is one key of 3 ceil(log2 C) bits; otherwise the triples are sorted
// by c (32 bits) and then, stably, by (a, b) (64 bits).  The file is built with -ffp-contract=off.  Scratch is
// one block of the device-block cache per call; the result is a geometry of the block pool.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <memory>
#include <mutex>
#include <string>

#include "device_block.hpp"
#include "device_cub.hpp"
#include "device_prims.hpp"
#include "mqr_common.hpp"

namespace mqr {
namespace sv {

constexpr int kT = 256;
constexpr unsigned kGridCap = 2048;         // grid-stride kernels: 8 workgroups per CU
constexpr int64_t kAxisCells = 1 << 21;     // a grid of this many cells along an axis is an error

// Per-device timing events of the last call (mqr_mesh_simplify_last_ms, a measurement hook): call start (behind
// the input copies), vertices done, call end.  The mutex also makes the calls of a device take turns.
struct TimeCtx {
    std::mutex mu;
    hipEvent_t ev[3] = {};
    bool timed = false;
    int open() {
        for (hipEvent_t& e : ev)
            if (!e) MQR_CHECK_HIP(hipEventCreate(&e));
        timed = false;
        return 0;
    }
};
static TimeCtx g_time[kMaxDevices];

struct Ctrl {
    int32_t bad_coord;
    uint32_t box[6];               // ordered_u32 of the bounds: min xyz, max xyz
    unsigned long long n_cells;    // segment heads
    unsigned long long collapsed;  // triangles with two equal corners
    unsigned long long kept;       // surviving triangles
    unsigned int max_pop;          // the largest cell's population
};

// The grid of a call: origin and size as the rule states them, the bits of each axis' cell index.
struct Grid {
    double origin[3];
    double vs;
    int bits[3];
};

__host__ __device__ inline int64_t cell_of(float p, double origin, double vs) {
    return (int64_t)floor(((double)p - origin) / vs);
}

__device__ inline uint64_t cell_key(const float* __restrict__ pos, int64_t i, const Grid& g) {
    const uint64_t cx = (uint64_t)cell_of(pos[3 * i], g.origin[0], g.vs);
    const uint64_t cy = (uint64_t)cell_of(pos[3 * i + 1], g.origin[1], g.vs);
    const uint64_t cz = (uint64_t)cell_of(pos[3 * i + 2], g.origin[2], g.vs);
    return (cx << (g.bits[1] + g.bits[2])) | (cy << g.bits[2]) | cz;
}

// the workgroup's sum of v (every lane calls it) -> one atomicAdd
__device__ inline void block_count_atomic(unsigned v, unsigned long long* out) {
    __shared__ unsigned part[kT / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor((int)v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned s = part[0] + part[1] + part[2] + part[3];
        if (s) atomicAdd(out, (unsigned long long)s);
    }
}

__global__ void __launch_bounds__(kT) k_bounds(const float* __restrict__ pos, int64_t nv, uint32_t* box) {
    uint32_t lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * kT) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t u = ordered_u32(pos[3 * i + a]);
            lo[a] = min(lo[a], u);
            hi[a] = max(hi[a], u);
        }
    }
    block_bounds_atomic(lo, hi, box);
}

template <bool WITH_INDEX>
__global__ void __launch_bounds__(kT) k_keys(const float* __restrict__ pos, int64_t nv, Grid g,
                                             uint64_t* __restrict__ keys, int32_t* __restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * kT) {
        keys[i] = cell_key(pos, i, g);
        if (WITH_INDEX) idx[i] = (int32_t)i;
    }
}

// Segment heads of the sorted keys, counted.  WRITE: head[s], and flag[idx_s[s]] = head[s] -- the sort is
// stable, so a segment's head is its lowest input index, the cell's first appearance.
template <bool WRITE>
__global__ void __launch_bounds__(kT) k_heads(const uint64_t* __restrict__ keys_s, const int32_t* __restrict__ idx_s,
                                              int64_t nv, int32_t* __restrict__ head, int32_t* __restrict__ flag,
                                              unsigned long long* n_cells) {
    unsigned cnt = 0;
    for (int64_t s = (int64_t)blockIdx.x * kT + threadIdx.x; s < nv; s += (int64_t)gridDim.x * kT) {
        const int h = s == 0 || keys_s[s] != keys_s[s - 1];
        cnt += h;
        if (WRITE) {
            head[s] = h;
            flag[idx_s[s]] = h;
        }
    }
    block_count_atomic(cnt, n_cells);
}

// seg_start[k] = the sorted position where segment k begins (hscan: the exclusive sum of head)
__global__ void __launch_bounds__(kT) k_seg_starts(const int32_t* __restrict__ head, const int32_t* __restrict__ hscan,
                                                   int64_t nv, int32_t* __restrict__ seg_start) {
    const int64_t s = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (s < nv && head[s]) seg_start[hscan[s]] = (int32_t)s;
}

__device__ inline void add3(double (&acc)[3], const float* __restrict__ src, int64_t i) {
    acc[0] += (double)src[3 * i];
    acc[1] += (double)src[3 * i + 1];
    acc[2] += (double)src[3 * i + 2];
}
__device__ inline void mean3(float* __restrict__ out, int64_t j, const double (&acc)[3], double n) {
    out[3 * j] = (float)(acc[0] / n);
    out[3 * j + 1] = (float)(acc[1] / n);
    out[3 * j + 2] = (float)(acc[2] / n);
}

// ONE THREAD PER CELL: the members of segment k lie at sorted positions [seg_start[k], seg_start[k + 1]) in
// ascending input index.  Output vertex j = rank[first member] (rank: the exclusive sum of flag in input order).
__global__ void __launch_bounds__(kT) k_cells(const float* __restrict__ pos, const float* __restrict__ nrm,
                                              const float* __restrict__ col, const int32_t* __restrict__ idx_s,
                                              const int32_t* __restrict__ seg_start, const int32_t* __restrict__ rank,
                                              int64_t nv, int64_t n_cells, float* __restrict__ o_pos,
                                              float* __restrict__ o_nrm, float* __restrict__ o_col,
                                              int32_t* __restrict__ map, unsigned int* max_pop) {
    __shared__ unsigned part[kT / 64];
    unsigned pop_max = 0;
    for (int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x; k < n_cells; k += (int64_t)gridDim.x * kT) {
        const int64_t b = seg_start[k], e = k + 1 < n_cells ? (int64_t)seg_start[k + 1] : nv;
        const int32_t j = rank[idx_s[b]];
        double sp[3] = {0.0, 0.0, 0.0}, sn[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
        for (int64_t s = b; s < e; ++s) {
            const int64_t i = idx_s[s];
            add3(sp, pos, i);
            if (nrm) add3(sn, nrm, i);
            if (col) add3(sc, col, i);
            map[i] = j;
        }
        const double n = (double)(e - b);
        mean3(o_pos, j, sp, n);
        if (nrm) mean3(o_nrm, j, sn, n);
        if (col) mean3(o_col, j, sc, n);
        pop_max = max(pop_max, (unsigned)(e - b));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) pop_max = max(pop_max, (unsigned)__shfl_xor((int)pop_max, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = pop_max;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(max_pop, max(max(part[0], part[1]), max(part[2], part[3])));
}

// (a, b, c) = map[corners], rotated so the smallest comes first (the cyclic order, hence the orientation, stays)
struct Triple {
    uint32_t a, b, c;
};
__device__ inline Triple remap(const int32_t* __restrict__ tri, const int32_t* __restrict__ map, int64_t t) {
    const uint32_t a = (uint32_t)map[tri[3 * t]], b = (uint32_t)map[tri[3 * t + 1]], c = (uint32_t)map[tri[3 * t + 2]];
    if (a <= b && a <= c) return Triple{a, b, c};
    if (b <= a && b <= c) return Triple{b, c, a};
    return Triple{c, a, b};
}
__device__ inline bool collapsed(const Triple& r) { return r.a == r.b || r.b == r.c || r.a == r.c; }

// A triple as sort keys.  NARROW (fewer than 2^21 output vertices, bc = ceil(log2 C) <= 21): one key of 3 bc
// bits.  Otherwise key = (a, b) in 32 + bc bits and c32 = c.  A collapsed triple keeps its key: no triple with
// three distinct corners shares it, so it shadows no survivor, and k_keep drops it by unpacking.
template <bool NARROW>
__device__ inline uint64_t pack(const Triple& r, int bc) {
    return NARROW ? ((uint64_t)r.a << (2 * bc)) | ((uint64_t)r.b << bc) | r.c : ((uint64_t)r.a << 32) | r.b;
}
template <bool NARROW>
__device__ inline Triple unpack(uint64_t k, uint32_t c, int bc) {
    const uint64_t m = (1ull << bc) - 1;
    if (NARROW) return Triple{(uint32_t)((k >> (2 * bc)) & m), (uint32_t)((k >> bc) & m), (uint32_t)(k & m)};
    return Triple{(uint32_t)(k >> 32), (uint32_t)(k & 0xffffffffull), c};
}

// packed triples + iota, the collapsed ones counted
template <bool NARROW>
__global__ void __launch_bounds__(kT) k_triples(const int32_t* __restrict__ tri, const int32_t* __restrict__ map,
                                                int64_t nt, int bc, uint64_t* __restrict__ key,
                                                uint32_t* __restrict__ c32, int32_t* __restrict__ tidx,
                                                unsigned long long* n_collapsed) {
    unsigned cnt = 0;
    for (int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x; t < nt; t += (int64_t)gridDim.x * kT) {
        const Triple r = remap(tri, map, t);
        cnt += collapsed(r);
        key[t] = pack<NARROW>(r, bc);
        if (!NARROW) c32[t] = r.c;
        tidx[t] = (int32_t)t;
    }
    block_count_atomic(cnt, n_collapsed);
}

// the (a, b) keys in the order the sort by c left the triangles in
__global__ void __launch_bounds__(kT) k_gather_keys(const uint64_t* __restrict__ key, const int32_t* __restrict__ order,
                                                    int64_t nt, uint64_t* __restrict__ out) {
    for (int64_t s = (int64_t)blockIdx.x * kT + threadIdx.x; s < nt; s += (int64_t)gridDim.x * kT) out[s] = key[order[s]];
}

// keep[t]: not collapsed, and the first of its run of equal triples (the sorts are stable: the lowest input index)
template <bool NARROW>
__global__ void __launch_bounds__(kT) k_keep(const uint64_t* __restrict__ key_s, const int32_t* __restrict__ tidx_s,
                                             const uint32_t* __restrict__ c32, int64_t nt, int bc,
                                             int32_t* __restrict__ keep, unsigned long long* kept) {
    unsigned cnt = 0;
    for (int64_t s = (int64_t)blockIdx.x * kT + threadIdx.x; s < nt; s += (int64_t)gridDim.x * kT) {
        const uint64_t k = key_s[s];
        const int32_t t = tidx_s[s];
        const uint32_t c = NARROW ? 0u : c32[t];
        bool head = s == 0 || k != key_s[s - 1];
        if (!NARROW && !head) head = c != c32[tidx_s[s - 1]];
        const int kp = head && !collapsed(unpack<NARROW>(k, c, bc));
        keep[t] = kp;
        cnt += kp;
    }
    block_count_atomic(cnt, kept);
}

// the survivors, in input order (kscan: the exclusive sum of keep); the triple is unpacked from the unsorted key
template <bool NARROW>
__global__ void __launch_bounds__(kT) k_compact(const uint64_t* __restrict__ key, const uint32_t* __restrict__ c32,
                                                const int32_t* __restrict__ keep, const int32_t* __restrict__ kscan,
                                                int64_t nt, int bc, int32_t* __restrict__ o_tri) {
    for (int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x; t < nt; t += (int64_t)gridDim.x * kT) {
        if (!keep[t]) continue;
        const Triple r = unpack<NARROW>(key[t], NARROW ? 0u : c32[t], bc);
        const int64_t o = kscan[t];
        o_tri[3 * o] = (int32_t)r.a;
        o_tri[3 * o + 1] = (int32_t)r.b;
        o_tri[3 * o + 2] = (int32_t)r.c;
    }
}

// ---------------------------------------------------------------------------------------------- host side
static int check_common(const char* who, int device, const void* vertices, int64_t nv, int loc) {
    MQR_REQUIRE(vertices, "null argument");
    MQR_REQUIRE(nv > 0, std::string(who) + ": the mesh has no vertices");
    MQR_REQUIRE(nv < ((int64_t)1 << 31), std::string(who) + ": mesh too large (nt or nv >= 2^31)");
    MQR_REQUIRE(loc == MQR_HOST || loc == MQR_DEVICE, std::string(who) + ": loc must be MQR_HOST or MQR_DEVICE");
    MQR_REQUIRE(device >= 0 && device < kMaxDevices, "device index out of range");
    return 0;
}

static int check_voxel_size(const char* who, double vs) {
    MQR_REQUIRE(std::isfinite(vs) && vs > 0.0, std::string(who) + ": voxel_size must be finite and > 0");
    return 0;
}

// the caller's stream when it is this device's (then nothing needs ordering), else the null stream behind a
// host drain of the caller's (as meshsample.hip)
static int open_stream(int device, hipStream_t* s) {
    MQR_CHECK_HIP(hipSetDevice(device));
    *s = copy_stream(device);
    if (caller_stream() && *s != caller_stream()) MQR_CHECK_HIP(hipStreamSynchronize(caller_stream()));
    return 0;
}

// Finite check + bounds of `pos`, read back: lo / hi as the exact doubles of the float32 bounds (a -0 reads +0).
static int bounds_pass(const char* who, const float* pos, int64_t nv, Ctrl* ctrl, hipStream_t s, double (&lo)[3],
                       double (&hi)[3]) {
    Ctrl init = {};
    for (int a = 0; a < 3; ++a) init.box[a] = ~0u;
    MQR_CHECK_HIP(hipMemcpyAsync(ctrl, &init, sizeof init, hipMemcpyHostToDevice, s));
    const unsigned g = std::min<unsigned>(nb(nv), kGridCap);
    hipLaunchKernelGGL(k_check_finite, dim3(std::min<unsigned>(nb(3 * nv), 4096)), dim3(kT), 0, s, pos, 3 * nv, FLT_MAX,
                       &ctrl->bad_coord);
    hipLaunchKernelGGL(k_bounds, dim3(g), dim3(kT), 0, s, pos, nv, ctrl->box);
    MQR_CHECK_HIP(hipGetLastError());
    Ctrl hc;
    MQR_CHECK_HIP(hipMemcpyAsync(&hc, ctrl, sizeof hc, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    MQR_REQUIRE(!hc.bad_coord, std::string(who) + ": a vertex coordinate is not finite");
    for (int a = 0; a < 3; ++a) {
        lo[a] = (double)from_ordered(hc.box[a]) + 0.0;
        hi[a] = (double)from_ordered(hc.box[3 + a]) + 0.0;
    }
    return 0;
}

// The grid of (bounds, voxel size); *axis_cells = the largest cell count along an axis.  floor is monotone,
// so the largest cell index of an axis is the upper bound's.
static int make_grid(const char* who, const double (&lo)[3], const double (&hi)[3], double vs, Grid* g,
                     int64_t* axis_cells) {
    g->vs = vs;
    *axis_cells = 0;
    for (int a = 0; a < 3; ++a) {
        g->origin[a] = lo[a] - vs * 0.5;
        const double q = floor((hi[a] - g->origin[a]) / vs);
        MQR_REQUIRE(q + 1.0 < (double)kAxisCells,
                    std::string(who) + ": the grid is too fine (2^21 or more cells along an axis)");
        const int64_t n = (int64_t)q + 1;
        g->bits[a] = ceil_log2(n);
        *axis_cells = std::max(*axis_cells, n);
    }
    return 0;
}

static int key_bits(const Grid& g) { return std::max(1, g.bits[0] + g.bits[1] + g.bits[2]); }

}  // namespace sv
}  // namespace mqr

using namespace mqr;
using namespace mqr::sv;

extern "C" {

int mqr_vertex_bounds(int device, const float* vertices, int64_t nv, int loc, double* min3, double* max3) {
    MQR_REQUIRE(min3 && max3, "null argument");
    if (check_common("vertex bounds", device, vertices, nv, loc)) return 2;
    hipStream_t s;
    if (open_stream(device, &s)) return 1;
    ScratchLayout L;
    float* d_v;
    Ctrl* ctrl;
    L.add(d_v, 3 * nv, loc == MQR_HOST);
    L.add(ctrl, 1);
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed("vertex bounds", L.total());
    StreamDrain drain{s};
    const float* pos = vertices;
    if (loc == MQR_HOST) {
        if (copy_to_device(device, d_v, vertices, sizeof(float) * 3 * nv, s)) return 1;
        pos = d_v;
    }
    double lo[3], hi[3];
    if (int rc = bounds_pass("vertex bounds", pos, nv, ctrl, s, lo, hi)) return rc;
    for (int a = 0; a < 3; ++a) min3[a] = lo[a], max3[a] = hi[a];
    return 0;
}

int mqr_mesh_cluster_count(int device, const float* vertices, int64_t nv, int loc, double voxel_size,
                           int64_t* n_cells) {
    MQR_REQUIRE(n_cells, "null argument");
    if (check_voxel_size("cluster count", voxel_size)) return 2;
    if (check_common("cluster count", device, vertices, nv, loc)) return 2;
    hipStream_t s;
    if (open_stream(device, &s)) return 1;
    TimeCtx& tc = g_time[device];
    std::lock_guard<std::mutex> lock(tc.mu);
    if (tc.open()) return 1;
    ScratchLayout L;
    float* d_v;
    Ctrl* ctrl;
    uint64_t *keys, *keys_s;
    L.add(d_v, 3 * nv, loc == MQR_HOST);
    L.add(ctrl, 1);
    L.add_each(nv, keys, keys_s);
    int bits = 64;
    auto sort_keys = [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortKeys(t, b, (const uint64_t*)keys, keys_s, (int)nv, 0, bits, s);
    };
    CubTemp tmp;
    MQR_CHECK_HIP(tmp.lay_out(L, sort_keys));
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed("cluster count", L.total());
    StreamDrain drain{s};
    const float* pos = vertices;
    if (loc == MQR_HOST) {
        if (copy_to_device(device, d_v, vertices, sizeof(float) * 3 * nv, s)) return 1;
        pos = d_v;
    }
    MQR_CHECK_HIP(hipEventRecord(tc.ev[0], s));
    double lo[3], hi[3];
    if (int rc = bounds_pass("cluster count", pos, nv, ctrl, s, lo, hi)) return rc;
    Grid g;
    int64_t axis_cells;
    if (int rc = make_grid("cluster count", lo, hi, voxel_size, &g, &axis_cells)) return rc;
    bits = key_bits(g);
    const unsigned gv = std::min<unsigned>(nb(nv), kGridCap);
    hipLaunchKernelGGL(k_keys<false>, dim3(gv), dim3(kT), 0, s, pos, nv, g, keys, (int32_t*)nullptr);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(tmp.run(sort_keys));
    hipLaunchKernelGGL(k_heads<false>, dim3(gv), dim3(kT), 0, s, (const uint64_t*)keys_s, (const int32_t*)nullptr, nv,
                       (int32_t*)nullptr, (int32_t*)nullptr, &ctrl->n_cells);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(hipEventRecord(tc.ev[1], s));
    MQR_CHECK_HIP(hipEventRecord(tc.ev[2], s));
    unsigned long long n = 0;
    MQR_CHECK_HIP(hipMemcpyAsync(&n, &ctrl->n_cells, sizeof n, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    *n_cells = (int64_t)n;
    tc.timed = true;
    return 0;
}

int mqr_mesh_simplify_clustering(int device, const float* vertices, int64_t nv, const float* normals,
                                 const float* colors, const int32_t* triangles, int64_t nt, int loc, double voxel_size,
                                 mqr_geom** out, int64_t* stats) {
    MQR_REQUIRE(out && stats, "null argument");
    *out = nullptr;
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    if (check_voxel_size("mesh simplify", voxel_size)) return 2;
    MQR_REQUIRE(nt >= 0 && nt < ((int64_t)1 << 31), "mesh simplify: mesh too large (nt or nv >= 2^31)");
    MQR_REQUIRE(nt == 0 || triangles, "null argument");
    if (check_common("mesh simplify", device, vertices, nv, loc)) return 2;
    hipStream_t s;
    if (open_stream(device, &s)) return 1;
    TimeCtx& tc = g_time[device];
    std::lock_guard<std::mutex> lock(tc.mu);
    if (tc.open()) return 1;

    const bool host_in = loc == MQR_HOST, tris = nt > 0;
    const bool wide_possible = tris && nv >= kAxisCells;  // the output vertex count is at most nv
    ScratchLayout L;
    float *d_v, *d_n, *d_c;
    int32_t *d_t, *bad_index, *idx, *idx_s, *flag, *rank, *head, *hscan, *seg_start, *map;
    int32_t *tidx, *tidx_s, *tidx_c, *keep, *kscan;
    uint64_t *keys, *keys_s, *tkey, *tkey_s, *tkey_c;
    uint32_t *c32, *c32_s;
    Ctrl* ctrl;
    L.add(d_v, 3 * nv, host_in);
    L.add(d_t, 3 * nt, host_in && tris);
    L.add(d_n, 3 * nv, host_in && normals);
    L.add(d_c, 3 * nv, host_in && colors);
    L.add(ctrl, 1);
    L.add(bad_index, 1);
    L.add_each(nv, keys, keys_s);
    L.add_each(nv, idx, idx_s, flag, rank, head, hscan, seg_start, map);
    L.add(tkey, nt, tris);
    L.add(tkey_s, nt, tris);
    L.add(tidx, nt, tris);
    L.add(tidx_s, nt, tris);
    L.add(keep, nt, tris);
    L.add(kscan, nt, tris);
    L.add(c32, nt, wide_possible);    // the two-pass sort of the wide triples: c, then (a, b)
    L.add(c32_s, nt, wide_possible);
    L.add(tkey_c, nt, wide_possible);
    L.add(tidx_c, nt, wide_possible);
    // the size queries ask for every bit (the most passes); the runs sort the bits in use
    int vbits = 64, cbits = 32, tbits = 64;
    bool narrow = true;
    auto sort_cells = [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, (const uint64_t*)keys, keys_s, (const int32_t*)idx, idx_s,
                                                  (int)nv, 0, vbits, s);
    };
    auto scan_heads = [&](void* t, size_t& b) {
        return hipcub::DeviceScan::ExclusiveSum(t, b, (const int32_t*)head, hscan, (int)nv, s);
    };
    auto scan_flags = [&](void* t, size_t& b) {
        return hipcub::DeviceScan::ExclusiveSum(t, b, (const int32_t*)flag, rank, (int)nv, s);
    };
    auto sort_c = [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, (const uint32_t*)c32, c32_s, (const int32_t*)tidx, tidx_c,
                                                  (int)nt, 0, cbits, s);
    };
    auto sort_triples = [&](void* t, size_t& b) {  // narrow: the whole triple; wide: (a, b), behind the sort by c
        return hipcub::DeviceRadixSort::SortPairs(t, b, (const uint64_t*)(narrow ? tkey : tkey_c), tkey_s,
                                                  (const int32_t*)(narrow ? tidx : tidx_c), tidx_s, (int)nt, 0, tbits, s);
    };
    auto scan_keep = [&](void* t, size_t& b) {
        return hipcub::DeviceScan::ExclusiveSum(t, b, (const int32_t*)keep, kscan, (int)nt, s);
    };
    CubTemp tmp;
    MQR_CHECK_HIP(tmp.lay_out(L, sort_cells, scan_heads, scan_flags, sort_c, sort_triples, scan_keep));
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed("mesh simplify", L.total());
    StreamDrain drain{s};

    const size_t b_v = sizeof(float) * 3 * nv;
    const float *pos = vertices, *nrm = normals, *col = colors;
    const int32_t* tri = triangles;
    if (host_in) {
        if (copy_to_device(device, d_v, vertices, b_v, s) ||
            (tris && copy_to_device(device, d_t, triangles, sizeof(int32_t) * 3 * nt, s)) ||
            (d_n && copy_to_device(device, d_n, normals, b_v, s)) || (d_c && copy_to_device(device, d_c, colors, b_v, s)))
            return 1;
        pos = d_v, tri = d_t, nrm = d_n, col = d_c;
    }

    // ---- checks and bounds: nothing gathers through an index before the flags are read
    MQR_CHECK_HIP(hipEventRecord(tc.ev[0], s));
    MQR_CHECK_HIP(hipMemsetAsync(bad_index, 0, sizeof(int32_t), s));
    if (tris) {
        hipLaunchKernelGGL(k_check_indices, dim3(nb(3 * nt)), dim3(kT), 0, s, tri, 3 * nt, nv, bad_index);
        MQR_CHECK_HIP(hipGetLastError());
    }
    int32_t h_bad = 0;
    MQR_CHECK_HIP(hipMemcpyAsync(&h_bad, bad_index, sizeof h_bad, hipMemcpyDeviceToHost, s));
    double lo[3], hi[3];
    if (int rc = bounds_pass("mesh simplify", pos, nv, ctrl, s, lo, hi)) return rc;  // synchronises the stream
    MQR_REQUIRE(!h_bad, "mesh simplify: a triangle index is outside [0, nv)");
    Grid g;
    int64_t axis_cells;
    if (int rc = make_grid("mesh simplify", lo, hi, voxel_size, &g, &axis_cells)) return rc;

    // ---- cells: keys, stable sort, heads, first-of-its-cell flags, both scans, segment starts
    vbits = key_bits(g);
    const unsigned gv = std::min<unsigned>(nb(nv), kGridCap);
    hipLaunchKernelGGL(k_keys<true>, dim3(gv), dim3(kT), 0, s, pos, nv, g, keys, idx);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(tmp.run(sort_cells));
    hipLaunchKernelGGL(k_heads<true>, dim3(gv), dim3(kT), 0, s, (const uint64_t*)keys_s, (const int32_t*)idx_s, nv, head,
                       flag, &ctrl->n_cells);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(tmp.run(scan_heads));
    MQR_CHECK_HIP(tmp.run(scan_flags));
    hipLaunchKernelGGL(k_seg_starts, dim3(nb(nv)), dim3(kT), 0, s, (const int32_t*)head, (const int32_t*)hscan, nv,
                       seg_start);
    MQR_CHECK_HIP(hipGetLastError());
    unsigned long long n_cells_u = 0;
    MQR_CHECK_HIP(hipMemcpyAsync(&n_cells_u, &ctrl->n_cells, sizeof n_cells_u, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    const int64_t C = (int64_t)n_cells_u;
    MQR_REQUIRE(C >= 1 && C <= nv, "mesh simplify: internal error (cell count out of range)");

    // ---- the result: C vertices and room for every input triangle (held by a guard: every error exit below
    // frees it and returns its block to the cache)
    std::unique_ptr<mqr_geom, int (*)(mqr_geom*)> geom(new mqr_geom(), mqr_geom_free);
    geom->device = device;
    geom->nv = C;
    geom->nt = 0;
    if (geom_alloc(geom.get(), C, nt, colors != nullptr)) {
        set_error("mesh simplify: device allocation failed");
        return 1;
    }
    if (!nrm)  // zeros over the normals' whole piece of the block (it ends where the triangles begin)
        MQR_CHECK_HIP(hipMemsetAsync(geom->nrm, 0, (char*)geom->tri - (char*)geom->nrm, s));
    hipLaunchKernelGGL(k_cells, dim3(std::min<unsigned>(nb(C), kGridCap)), dim3(kT), 0, s, pos, nrm, col,
                       (const int32_t*)idx_s, (const int32_t*)seg_start, (const int32_t*)rank, nv, C, geom->pos,
                       nrm ? geom->nrm : (float*)nullptr, geom->col, map, &ctrl->max_pop);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(hipEventRecord(tc.ev[1], s));

    // ---- triangles: packed triples, stable sort, heads, compaction in input order
    if (tris) {
        narrow = C < kAxisCells;
        const int bc = std::max(1, ceil_log2(C));
        const unsigned gt = std::min<unsigned>(nb(nt), kGridCap);
        const uint32_t* cc = c32;
        if (narrow) {
            tbits = 3 * bc;
            hipLaunchKernelGGL(k_triples<true>, dim3(gt), dim3(kT), 0, s, tri, (const int32_t*)map, nt, bc, tkey,
                               (uint32_t*)nullptr, tidx, &ctrl->collapsed);
            MQR_CHECK_HIP(hipGetLastError());
            MQR_CHECK_HIP(tmp.run(sort_triples));
            hipLaunchKernelGGL(k_keep<true>, dim3(gt), dim3(kT), 0, s, (const uint64_t*)tkey_s, (const int32_t*)tidx_s, cc,
                               nt, bc, keep, &ctrl->kept);
        } else {
            cbits = bc, tbits = 32 + bc;
            hipLaunchKernelGGL(k_triples<false>, dim3(gt), dim3(kT), 0, s, tri, (const int32_t*)map, nt, bc, tkey, c32,
                               tidx, &ctrl->collapsed);
            MQR_CHECK_HIP(hipGetLastError());
            MQR_CHECK_HIP(tmp.run(sort_c));
            hipLaunchKernelGGL(k_gather_keys, dim3(gt), dim3(kT), 0, s, (const uint64_t*)tkey, (const int32_t*)tidx_c, nt,
                               tkey_c);
            MQR_CHECK_HIP(hipGetLastError());
            MQR_CHECK_HIP(tmp.run(sort_triples));
            hipLaunchKernelGGL(k_keep<false>, dim3(gt), dim3(kT), 0, s, (const uint64_t*)tkey_s, (const int32_t*)tidx_s,
                               cc, nt, bc, keep, &ctrl->kept);
        }
        MQR_CHECK_HIP(hipGetLastError());
        MQR_CHECK_HIP(tmp.run(scan_keep));
        if (narrow)
            hipLaunchKernelGGL(k_compact<true>, dim3(gt), dim3(kT), 0, s, (const uint64_t*)tkey, cc, (const int32_t*)keep,
                               (const int32_t*)kscan, nt, bc, geom->tri);
        else
            hipLaunchKernelGGL(k_compact<false>, dim3(gt), dim3(kT), 0, s, (const uint64_t*)tkey, cc, (const int32_t*)keep,
                               (const int32_t*)kscan, nt, bc, geom->tri);
        MQR_CHECK_HIP(hipGetLastError());
    }
    MQR_CHECK_HIP(hipEventRecord(tc.ev[2], s));
    Ctrl hc;
    MQR_CHECK_HIP(hipMemcpyAsync(&hc, ctrl, sizeof hc, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    tc.timed = true;
    geom->nt = (int64_t)hc.kept;
    stats[0] = nv;
    stats[1] = C;
    stats[2] = nt;
    stats[3] = (int64_t)hc.collapsed;
    stats[4] = nt - (int64_t)hc.collapsed - (int64_t)hc.kept;
    stats[5] = (int64_t)hc.kept;
    stats[6] = (int64_t)hc.max_pop;
    stats[7] = axis_cells;
    *out = geom.release();
    return 0;
}

int mqr_mesh_simplify_last_ms(int device, float* call_ms, float* vertex_ms, float* triangle_ms) {
    MQR_REQUIRE(call_ms && vertex_ms && triangle_ms, "null argument");
    MQR_REQUIRE(device >= 0 && device < kMaxDevices, "device index out of range");
    TimeCtx& tc = g_time[device];
    std::lock_guard<std::mutex> lock(tc.mu);
    MQR_REQUIRE(tc.timed, "no completed mqr_mesh_simplify_clustering or mqr_mesh_cluster_count call on this device");
    MQR_CHECK_HIP(hipEventElapsedTime(call_ms, tc.ev[0], tc.ev[2]));
    MQR_CHECK_HIP(hipEventElapsedTime(vertex_ms, tc.ev[0], tc.ev[1]));
    MQR_CHECK_HIP(hipEventElapsedTime(triangle_ms, tc.ev[1], tc.ev[2]));
    return 0;
}

}  // extern "C"
