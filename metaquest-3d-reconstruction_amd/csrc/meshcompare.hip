// meshcompare.hip -- the device side of the ground-truth comparison (mqr/compare_mesh_to_ground_truth.py).
//
// Reference: analysis/computation/compare_mesh_to_ground_truth.py.  Its Open3D calls come down to three
// primitives, each an entry point here (rules in DESIGN §2.6):
//   mqr_nn_*            compute_point_cloud_distance / KDTreeFlann knn 1: the exact nearest target of every
//                       query over bucket_tree.hpp's Morton-bucket tree (built by bucket_tree.hip), float64 on
//                       the widened float32 coordinates, d2 = (dx dx + dy dy) + dz dz, ties to the lowest
//                       target index;
//   mqr_distance_stats  np.mean / np.std / np.min / np.max / np.median / (x < t).sum() of a distance array:
//                       order-fixed float64 slab sums (device_prims.hpp), the median from a radix sort of
//                       the bit patterns;
//   mqr_mesh_measure    get_surface_area, get_axis_aligned_bounding_box, get_volume and the boundary edges of
//                       count_holes, on one edge sort (mesh_edges.hpp, loop edges kept).
// The file is built with -ffp-contract=off.  Scratch is one block of the device-block cache per call; a tree
// and a boundary list own a plain device allocation until they are destroyed.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>

#include "bucket_tree.hpp"
#include "device_block.hpp"
#include "device_cub.hpp"
#include "device_prims.hpp"
#include "mesh_edges.hpp"
#include "mqr_common.hpp"
#include "pair_reduce.hpp"

struct mqr_nn {
    int device = 0;
    void* mem = nullptr;     // one device allocation: the tree's boxes, points and bounds
    mqr::BucketTree t{};     // over the targets; pts carry the original target index
};

struct mqr_edge_list {
    int device = 0;
    int64_t n = 0;
    int32_t* pairs = nullptr;  // [n][2] (min, max)
};

namespace mqr {
namespace mc {
using namespace edges;

constexpr int kT = pairsum::kThreads;
constexpr int kPer = 4;
constexpr int kTile = kT * kPer;
constexpr int kNS = 2;          // sums of a slab
constexpr int kSlab = kNS + 2;  // ... then one min and one max

static StreamTable g_streams;

// ------------------------------------------------------------------ checks
// device_prims.hpp's k_check_finite with FLT_MAX asks for finite values; the search asks for kCoordLimit,
// inside which the float32 bounds of bucket_tree.hpp cannot overflow: a difference is at most 2e18, three
// squares of it 1.2e37 < FLT_MAX.  (An overflowed bound is +inf, which would prune a nearer point.)
constexpr float kCoordLimit = 1e18f;

// ------------------------------------------------------------------ nearest neighbour
// One query per lane, K = 1: the best (d2, index) pair in registers, the traversal stack in LDS (stack-major:
// lane t's entry e at stk[256 e + t], conflict-free), sized by the host to the tree's depth + 2 (a nearest-
// first DFS holds one pending sibling per level plus the current pair).  Boxes are pruned and ordered on
// box_d2_lb, candidates prefiltered on the same float32 bound and compared exactly in float64; (d2, index) is
// a total order, so neither the visiting order nor the order of the queries changes a result.  Lane t takes
// query order[t]: the host sorts the queries by their Morton key in the tree's frame, so a wave's 64 queries
// are neighbours and walk nearly the same nodes, and results scatter back to the caller's order.
__global__ __launch_bounds__(256) void k_nn1(const float* __restrict__ Q, const int32_t* __restrict__ order, int64_t nq,
                                             const float4* __restrict__ pts, int64_t n, int64_t P,
                                             const float4* __restrict__ lo, const float4* __restrict__ hi,
                                             double* __restrict__ dist, int32_t* __restrict__ idx) {
    extern __shared__ int32_t stk_lds[];
    int32_t* stk = stk_lds + threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq) return;
    const int64_t qi = order[t];
    const float qf[3] = {Q[3 * qi], Q[3 * qi + 1], Q[3 * qi + 2]};
    const double q[3] = {qf[0], qf[1], qf[2]};
    double bd = __builtin_inf();
    int32_t bi = 0x7fffffff;
    int sp = 0;
    stk[256 * sp++] = 1;
    while (sp) {
        const int32_t node = stk[256 * --sp];
        if ((double)box_d2_lb(qf, lo[node], hi[node]) > bd) continue;
        if (node >= P) {  // bucket
            const int64_t b = node - P;
            const int64_t e = min(n, (b + 1) * kBucket);
            for (int64_t j = b * kBucket; j < e; ++j) {
                const float4 pt = pts[j];
                const float fx = qf[0] - pt.x, fy = qf[1] - pt.y, fz = qf[2] - pt.z;
                if ((double)((fx * fx + fy * fy + fz * fz) * (1.0f - 0x1p-18f)) > bd) continue;
                const int32_t v = __float_as_int(pt.w);
                const double dx = q[0] - (double)pt.x, dy = q[1] - (double)pt.y, dz = q[2] - (double)pt.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < bd || (d2 == bd && v < bi)) bd = d2, bi = v;
            }
        } else {  // nearer child popped first
            const int32_t a = 2 * node, c = a + 1;
            const float da = box_d2_lb(qf, lo[a], hi[a]), dc = box_d2_lb(qf, lo[c], hi[c]);
            stk[256 * sp++] = da <= dc ? c : a;
            stk[256 * sp++] = da <= dc ? a : c;
        }
    }
    dist[qi] = sqrt(bd);
    if (idx) idx[qi] = bi;
}

// ------------------------------------------------------------------ distance statistics
struct StatsRes {
    double r0[kSlab];  // sum, count below the threshold, min, max
    double r1[kSlab];  // sum of squared deviations from the mean
    double median;
};

// PASS 0: [sum x, count of x < thr], min, max.  PASS 1: [sum (x - mean)^2] with the mean from PASS 0.
template <int PASS>
__global__ void __launch_bounds__(kT) k_stats(const double* __restrict__ x, int64_t n, double thr,
                                              const double* __restrict__ r0, double* __restrict__ slabs) {
    double acc[kNS] = {0.0, 0.0};
    double mn = INFINITY, mx = -INFINITY;
    const double mean = PASS == 1 ? r0[0] / (double)n : 0.0;
    for (int k = 0; k < kPer; ++k) {
        const int64_t i = (int64_t)blockIdx.x * kTile + k * kT + threadIdx.x;
        if (i >= n) continue;
        const double v = x[i];
        if (PASS == 0) {
            acc[0] += v;
            if (v < thr) acc[1] += 1.0;
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        } else {
            acc[0] += (v - mean) * (v - mean);
        }
    }
    block_sums_minmax_to_slab(acc, mn, mx, slabs + (int64_t)blockIdx.x * kSlab);
}

// numpy's median of the ascending array: the middle value, or the mean of the two middle ones
__global__ void k_median(const uint64_t* __restrict__ sorted, int64_t n, StatsRes* res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double a = __longlong_as_double((long long)sorted[(n - 1) / 2]);
    const double b = __longlong_as_double((long long)sorted[n / 2]);
    res->median = (n & 1) ? a : (a + b) / 2.0;
}

// ------------------------------------------------------------------ mesh measure
struct MeasureCtrl {
    uint32_t bb[8];     // bounds as ordered keys: min x y z, max x y z
    int32_t bad_index;
    int32_t bad_coord;
    int32_t open;       // an edge run that is not two opposite traversals
    int32_t pad;
    int64_t nboundary;  // DeviceSelect's count
    double sums[kSlab];  // area, signed volume
};

// Per triangle: 0.5 |(p1 - p0) x (p2 - p0)| and p0 . (p1 x p2) / 6, one slab per workgroup.
__global__ void __launch_bounds__(kT) k_tri_measure(const float* __restrict__ pos, const int32_t* __restrict__ tri,
                                                    int64_t nt, double* __restrict__ slabs) {
    double acc[kNS] = {0.0, 0.0};
    for (int k = 0; k < kPer; ++k) {
        const int64_t t = (int64_t)blockIdx.x * kTile + k * kT + threadIdx.x;
        if (t >= nt) continue;
        const int32_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
        double p0[3], p1[3], p2[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p0[a] = (double)pos[3 * (int64_t)i0 + a];
            p1[a] = (double)pos[3 * (int64_t)i1 + a];
            p2[a] = (double)pos[3 * (int64_t)i2 + a];
        }
        const double ea[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const double eb[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        const double n0 = ea[1] * eb[2] - ea[2] * eb[1], n1 = ea[2] * eb[0] - ea[0] * eb[2],
                     n2 = ea[0] * eb[1] - ea[1] * eb[0];
        acc[0] += 0.5 * sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        const double c0 = p1[1] * p2[2] - p1[2] * p2[1], c1 = p1[2] * p2[0] - p1[0] * p2[2],
                     c2 = p1[0] * p2[1] - p1[1] * p2[0];
        acc[1] += ((p0[0] * c0 + p0[1] * c1) + p0[2] * c2) / 6.0;
    }
    block_sums_minmax_to_slab(acc, INFINITY, -INFINITY, slabs + (int64_t)blockIdx.x * kSlab);
}

// slot 3 t + e runs from corner e to corner e + 1 of triangle t: does it go from the lower index to the higher?
__device__ inline bool ascending(const int32_t* __restrict__ tri, int32_t s) {
    const int32_t t = s / 3, e = s % 3;
    return tri[3 * (int64_t)t + e] < tri[3 * (int64_t)t + (e + 1) % 3];
}

// Run heads of the sorted edge entries: a run of one marks its slot as boundary; any run that is not exactly
// two traversals in opposite directions clears the closed-and-oriented property.
__global__ void k_edge_runs(const uint64_t* __restrict__ keys, const int32_t* __restrict__ slot, int64_t m,
                            const int32_t* __restrict__ tri, uint8_t* __restrict__ bflag, MeasureCtrl* c) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = keys[i];
    if (!run_head(keys, i, k)) return;
    const int mult = run_length3(keys, m, i);
    if (mult == 1) bflag[slot[i]] = 1;
    if (mult != 2 || ascending(tri, slot[i]) == ascending(tri, slot[i + 1])) c->open = 1;
}

__global__ void k_boundary_pairs(const int32_t* __restrict__ slots, int64_t nb, const int32_t* __restrict__ tri,
                                 int32_t* __restrict__ pairs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const int32_t s = slots[i], t = s / 3, e = s % 3;
    const int32_t a = tri[3 * (int64_t)t + e], b = tri[3 * (int64_t)t + (e + 1) % 3];
    pairs[2 * i] = min(a, b);
    pairs[2 * i + 1] = max(a, b);
}

}  // namespace mc
}  // namespace mqr

using namespace mqr;
using namespace mqr::mc;

extern "C" {

int mqr_nn_create(int device, const float* targets, int64_t n, int loc, mqr_nn** out) {
    MQR_REQUIRE(out, "null argument");
    *out = nullptr;
    MQR_REQUIRE(n > 0, "nn: the target set is empty");
    MQR_REQUIRE(targets, "null argument");
    MQR_REQUIRE(loc == MQR_HOST || loc == MQR_DEVICE, "nn: loc must be MQR_HOST or MQR_DEVICE");
    MQR_REQUIRE(n < ((int64_t)1 << 31), "nn: too many targets (n >= 2^31)");
    MQR_CHECK_HIP(hipSetDevice(device));
    hipStream_t s = g_streams.get(device);
    MQR_REQUIRE(s, "nn: no stream for the device");

    const size_t b_scr = bucket_tree_scratch_bytes(n, true, s);
    MQR_REQUIRE(b_scr, "nn: the tree build's sort could not be sized");
    const bool host_in = loc == MQR_HOST;
    const size_t b_pos = sizeof(float) * 3 * n;
    ScratchLayout L;
    float* d_pos;
    int32_t* flag;
    void* scratch;
    L.add(d_pos, 3 * n, host_in);
    L.add(flag, 1);
    L.add_bytes(scratch, b_scr);
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed("nn", L.total());

    const float* pos = targets;
    if (host_in) {
        if (copy_to_device(device, d_pos, targets, b_pos, s)) return 1;
        pos = d_pos;
    } else if (order_after_caller(device, s)) {
        return 2;
    }
    StreamDrain drain{s};

    MQR_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_check_finite, dim3(std::min<unsigned>(nb(3 * n), 4096)), dim3(kT), 0, s, pos, 3 * n,
                       kCoordLimit, flag);
    MQR_CHECK_HIP(hipGetLastError());
    int32_t bad = 0;
    MQR_CHECK_HIP(hipMemcpyAsync(&bad, flag, sizeof bad, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    MQR_REQUIRE(!bad, "nn: a target coordinate is not finite or beyond 1e18 in magnitude");

    // the tree keeps a plain allocation of its own: boxes, points, bounds
    mqr_nn* h = new mqr_nn();
    h->device = device;
    const size_t b_box = al256(bucket_tree_node_bytes(n)), b_pts = al256(sizeof(float4) * n);
    if (hipMalloc(&h->mem, 2 * b_box + b_pts + 256) != hipSuccess) {
        delete h;
        return scratch_failed("nn", 2 * b_box + b_pts + 256);
    }
    char* base = (char*)h->mem;
    hipError_t e = bucket_tree_build(s, pos, nullptr, n, scratch, b_scr, (float4*)base, (float4*)(base + b_box),
                                     (float4*)(base + 2 * b_box), (uint32_t*)(base + 2 * b_box + b_pts), &h->t);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error(std::string("nn: tree build: ") + hipGetErrorString(e));
        (void)hipFree(h->mem);
        delete h;
        return 1;
    }
    *out = h;
    return 0;
}

int mqr_nn_destroy(mqr_nn* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->mem);  // waits for the device: nothing still reads the tree
    delete h;
    return 0;
}

int mqr_nn_query(mqr_nn* h, const float* queries, int64_t nq, int loc, double* dist, int32_t* idx, int out_loc) {
    MQR_REQUIRE(h, "null argument");
    MQR_REQUIRE(nq >= 0 && nq < ((int64_t)1 << 31), "nn: too many queries (nq >= 2^31)");
    if (nq == 0) return 0;
    MQR_REQUIRE(queries && dist, "null argument");
    MQR_REQUIRE((loc == MQR_HOST || loc == MQR_DEVICE) && (out_loc == MQR_HOST || out_loc == MQR_DEVICE),
                "nn: loc and out_loc must be MQR_HOST or MQR_DEVICE");
    const int device = h->device;
    MQR_CHECK_HIP(hipSetDevice(device));
    hipStream_t s = g_streams.get(device);
    MQR_REQUIRE(s, "nn: no stream for the device");
    const size_t lds = sizeof(int32_t) * 256 * (size_t)(h->t.depth + 2);
    MQR_REQUIRE(lds <= 64 * 1024, "nn: the tree is too deep for the traversal stack");

    const bool host_in = loc == MQR_HOST, host_out = out_loc == MQR_HOST;
    const size_t b_q = sizeof(float) * 3 * nq, b_d = sizeof(double) * nq, b_i = sizeof(int32_t) * nq;
    ScratchLayout L;
    float* d_q;
    double* d_d;
    int32_t *d_i, *flag, *ids, *order;
    uint64_t *keys, *keys_s;
    L.add(d_q, 3 * nq, host_in);
    L.add(d_d, nq, host_out);
    L.add(d_i, nq, host_out && idx);
    L.add(flag, 1);
    L.add_each(nq, keys, keys_s, ids, order);
    auto sort_queries = [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, (const uint64_t*)keys, keys_s, (const int32_t*)ids, order,
                                                  (int)nq, 0, 63, s);
    };
    CubTemp tmp;
    MQR_CHECK_HIP(tmp.lay_out(L, sort_queries));
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed("nn", L.total());

    const float* Q = queries;
    if (host_in) {
        if (copy_to_device(device, d_q, queries, b_q, s)) return 1;
        Q = d_q;
    }
    if ((!host_in || !host_out) && order_after_caller(device, s)) return 2;
    StreamDrain drain{s};

    MQR_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_check_finite, dim3(std::min<unsigned>(nb(3 * nq), 4096)), dim3(kT), 0, s, Q, 3 * nq,
                       kCoordLimit, flag);
    MQR_CHECK_HIP(hipGetLastError());
    int32_t bad = 0;
    MQR_CHECK_HIP(hipMemcpyAsync(&bad, flag, sizeof bad, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    MQR_REQUIRE(!bad, "nn: a query coordinate is not finite or beyond 1e18 in magnitude");

    // queries in the Morton order of the tree's frame (a query outside the targets' box clamps to its faces)
    const unsigned gq = nb(nq);
    hipLaunchKernelGGL(k_iota, dim3(gq), dim3(kT), 0, s, ids, nq);
    bucket_tree_enqueue_keys(s, Q, ids, nq, h->t.bb, keys);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(tmp.run(sort_queries));
    double* o_d = host_out ? d_d : dist;
    int32_t* o_i = host_out ? d_i : idx;
    hipLaunchKernelGGL(k_nn1, dim3(gq), dim3(256), lds, s, Q, (const int32_t*)order, nq, h->t.pts, h->t.n, h->t.P,
                       h->t.lo, h->t.hi, o_d, o_i);
    MQR_CHECK_HIP(hipGetLastError());
    if (host_out) {
        if (copy_to_host(device, dist, d_d, b_d, s)) return 1;
        if (idx && copy_to_host(device, idx, d_i, b_i, s)) return 1;
    }
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int mqr_distance_stats(int device, const double* dist, int64_t n, int loc, double threshold,
                       mqr_distance_stats_result* out) {
    MQR_REQUIRE(out && dist, "null argument");
    MQR_REQUIRE(n > 0, "distance stats: the array is empty");
    MQR_REQUIRE(n < ((int64_t)1 << 31), "distance stats: too many values (n >= 2^31)");
    MQR_REQUIRE(loc == MQR_HOST || loc == MQR_DEVICE, "distance stats: loc must be MQR_HOST or MQR_DEVICE");
    MQR_CHECK_HIP(hipSetDevice(device));
    hipStream_t s = g_streams.get(device);
    MQR_REQUIRE(s, "distance stats: no stream for the device");

    const bool host_in = loc == MQR_HOST;
    const size_t b_x = sizeof(double) * n;
    const int64_t nblk = nb(n, kTile);
    const double* x = dist;
    ScratchLayout L;
    double *d_x, *slabs;
    StatsRes* res;
    uint64_t* sorted;
    L.add(d_x, n, host_in);
    L.add(res, 1);
    L.add(sorted, n);
    L.add(slabs, kSlab * nblk);
    // non-negative doubles order as their bit patterns (the sign bit is clear: 63 key bits)
    auto sort_values = [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortKeys(t, b, (const uint64_t*)x, sorted, (int)n, 0, 63, s);
    };
    CubTemp tmp;
    MQR_CHECK_HIP(tmp.lay_out(L, sort_values));
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed("distance stats", L.total());

    if (host_in) {
        if (copy_to_device(device, d_x, dist, b_x, s)) return 1;
        x = d_x;
    } else if (order_after_caller(device, s)) {
        return 2;
    }
    StreamDrain drain{s};

    hipLaunchKernelGGL(k_stats<0>, dim3((unsigned)nblk), dim3(kT), 0, s, x, n, threshold, (const double*)nullptr, slabs);
    hipLaunchKernelGGL(k_reduce_slabs<kNS>, dim3(1), dim3(kT), 0, s, slabs, nblk, res->r0);
    hipLaunchKernelGGL(k_stats<1>, dim3((unsigned)nblk), dim3(kT), 0, s, x, n, threshold, (const double*)res->r0, slabs);
    hipLaunchKernelGGL(k_reduce_slabs<kNS>, dim3(1), dim3(kT), 0, s, slabs, nblk, res->r1);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(tmp.run(sort_values));
    hipLaunchKernelGGL(k_median, dim3(1), dim3(64), 0, s, (const uint64_t*)sorted, n, res);
    MQR_CHECK_HIP(hipGetLastError());
    StatsRes r;
    MQR_CHECK_HIP(hipMemcpyAsync(&r, res, sizeof r, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));

    mqr_distance_stats_result o{};
    o.mean = r.r0[0] / (double)n;
    o.std = std::sqrt(r.r1[0] / (double)n);
    o.min = r.r0[kNS];
    o.max = r.r0[kNS + 1];
    o.median = r.median;
    o.count_below = (int64_t)r.r0[1];  // exact in float64: < 2^31
    o.count = n;
    *out = o;
    return 0;
}

int mqr_mesh_measure(int device, const float* vertices, int64_t nv, const int32_t* triangles, int64_t nt, int loc,
                     mqr_mesh_measure_result* out, mqr_edge_list** boundary) {
    MQR_REQUIRE(out, "null argument");
    if (boundary) *boundary = nullptr;
    MQR_REQUIRE(nv > 0, "mesh measure: the mesh has no vertices");
    MQR_REQUIRE(nt >= 0 && vertices && (triangles || nt == 0), "null argument");
    MQR_REQUIRE(loc == MQR_HOST || loc == MQR_DEVICE, "mesh measure: loc must be MQR_HOST or MQR_DEVICE");
    MQR_REQUIRE(nt < ((int64_t)1 << 31) / 3 && nv < ((int64_t)1 << 31), "mesh measure: mesh too large (3 nt >= 2^31)");
    MQR_CHECK_HIP(hipSetDevice(device));
    hipStream_t s = g_streams.get(device);
    MQR_REQUIRE(s, "mesh measure: no stream for the device");

    const int64_t m = 3 * nt;
    const int vbits = ceil_log2(nv + 1);
    const int64_t nblk_t = nb(nt, kTile);
    const bool host_in = loc == MQR_HOST;
    const size_t b_pos = sizeof(float) * 3 * nv, b_tri = sizeof(int32_t) * m;
    ScratchLayout L;
    float* d_pos;
    int32_t *d_tri, *vid, *slot, *slot_s;
    MeasureCtrl* ctrl;
    uint64_t *keys, *keys_s;
    uint8_t* bflag;
    double* slabs;
    L.add(d_pos, 3 * nv, host_in);
    L.add(d_tri, m, host_in && nt > 0);
    L.add(ctrl, 1);
    L.add(vid, nv);
    L.add(keys, m);  // (a point cloud's empty edge arrays still take a slot each)
    L.add_each(m, keys_s, slot, slot_s, bflag);
    L.add(slabs, kSlab * nblk_t);
    hipcub::CountingInputIterator<int32_t> it(0);
    auto sort_edges = [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, (const uint64_t*)keys, keys_s, (const int32_t*)slot, slot_s,
                                                  (int)m, 0, 32 + vbits, s);
    };
    // boundary slots ascending (the unsorted slot array is free again: the compacted list goes there)
    auto select_boundary = [&](void* t, size_t& b) {
        return hipcub::DeviceSelect::Flagged(t, b, it, (const uint8_t*)bflag, slot, &ctrl->nboundary, (int)m, s);
    };
    CubTemp tmp;
    MQR_CHECK_HIP(nt > 0 ? tmp.lay_out(L, sort_edges, select_boundary) : tmp.lay_out(L));
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed("mesh measure", L.total());

    const float* pos = vertices;
    const int32_t* tri = triangles;
    if (host_in) {
        if (copy_to_device(device, d_pos, vertices, b_pos, s) ||
            (nt > 0 && copy_to_device(device, d_tri, triangles, b_tri, s)))
            return 1;
        pos = d_pos, tri = d_tri;
    } else if (order_after_caller(device, s)) {
        return 2;
    }
    StreamDrain drain{s};

    // ---- checks and bounds (no kernel gathers through an index before the flags are read)
    MQR_CHECK_HIP(hipMemsetAsync(ctrl, 0, sizeof(MeasureCtrl), s));
    MQR_CHECK_HIP(hipMemsetAsync(ctrl->bb, 0xff, 3 * sizeof(uint32_t), s));
    if (nt > 0) hipLaunchKernelGGL(k_check_indices, dim3(nb(m)), dim3(kT), 0, s, tri, m, nv, &ctrl->bad_index);
    hipLaunchKernelGGL(k_check_finite, dim3(std::min<unsigned>(nb(3 * nv), 4096)), dim3(kT), 0, s, pos, 3 * nv,
                       FLT_MAX, &ctrl->bad_coord);
    hipLaunchKernelGGL(k_iota, dim3(nb(nv)), dim3(kT), 0, s, vid, nv);
    bucket_tree_enqueue_bounds(s, pos, vid, nv, ctrl->bb);
    MQR_CHECK_HIP(hipGetLastError());
    MeasureCtrl hc;
    MQR_CHECK_HIP(hipMemcpyAsync(&hc, ctrl, sizeof hc, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    MQR_REQUIRE(!hc.bad_index, "mesh measure: a triangle index is outside [0, nv)");
    MQR_REQUIRE(!hc.bad_coord, "mesh measure: a vertex coordinate is not finite");

    mqr_mesh_measure_result r{};
    for (int a = 0; a < 3; ++a) {
        r.min_bound[a] = (double)from_ordered(hc.bb[a]);
        r.max_bound[a] = (double)from_ordered(hc.bb[3 + a]);
    }
    r.num_vertices = nv;
    r.num_triangles = nt;
    if (nt == 0) {
        *out = r;
        return 0;
    }

    // ---- area and signed volume
    hipLaunchKernelGGL(k_tri_measure, dim3((unsigned)nblk_t), dim3(kT), 0, s, pos, tri, nt, slabs);
    hipLaunchKernelGGL(k_reduce_slabs<kNS>, dim3(1), dim3(kT), 0, s, slabs, nblk_t, ctrl->sums);
    // ---- the edge runs: boundary slots, closed and oriented
    hipLaunchKernelGGL(k_edge_keys<false>, dim3(nb(m)), dim3(kT), 0, s, tri, nt, (uint64_t)0, keys, slot);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(tmp.run(sort_edges));
    MQR_CHECK_HIP(hipMemsetAsync(bflag, 0, m, s));
    hipLaunchKernelGGL(k_edge_runs, dim3(nb(m)), dim3(kT), 0, s, (const uint64_t*)keys_s, (const int32_t*)slot_s, m, tri,
                       bflag, ctrl);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(tmp.run(select_boundary));
    MQR_CHECK_HIP(hipMemcpyAsync(&hc, ctrl, sizeof hc, hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));

    r.surface_area = hc.sums[0];
    r.is_closed_oriented = hc.open ? 0 : 1;
    r.volume = hc.open ? 0.0 : std::fabs(hc.sums[1]);
    r.boundary_edges = hc.nboundary;
    if (boundary && hc.nboundary > 0) {
        mqr_edge_list* e = new mqr_edge_list();
        e->device = device;
        e->n = hc.nboundary;
        if (hipMalloc((void**)&e->pairs, sizeof(int32_t) * 2 * e->n) != hipSuccess) {
            delete e;
            return scratch_failed("mesh measure", sizeof(int32_t) * 2 * (size_t)hc.nboundary);
        }
        hipLaunchKernelGGL(k_boundary_pairs, dim3(nb(e->n)), dim3(kT), 0, s, (const int32_t*)slot, e->n, tri, e->pairs);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            (void)hipFree(e->pairs);
            delete e;
            set_error("mesh measure: the boundary list kernel failed");
            return 1;
        }
        *boundary = e;
    }
    *out = r;
    return 0;
}

int mqr_edge_list_count(mqr_edge_list* list, int64_t* n) {
    MQR_REQUIRE(n, "null argument");
    *n = list ? list->n : 0;
    return 0;
}

int mqr_edge_list_copy(mqr_edge_list* list, int32_t* pairs, int loc) {
    if (!list || list->n == 0) return 0;
    MQR_REQUIRE(pairs, "null argument");
    MQR_REQUIRE(loc == MQR_HOST || loc == MQR_DEVICE, "edge list: loc must be MQR_HOST or MQR_DEVICE");
    MQR_CHECK_HIP(hipSetDevice(list->device));
    hipStream_t s = g_streams.get(list->device);
    MQR_REQUIRE(s, "edge list: no stream for the device");
    const size_t bytes = sizeof(int32_t) * 2 * list->n;
    if (loc == MQR_HOST) return copy_to_host(list->device, pairs, list->pairs, bytes, s);
    if (order_after_caller(list->device, s)) return 2;
    MQR_CHECK_HIP(hipMemcpyAsync(pairs, list->pairs, bytes, hipMemcpyDeviceToDevice, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int mqr_edge_list_free(mqr_edge_list* list) {
    if (!list) return 0;
    (void)hipSetDevice(list->device);
    (void)hipFree(list->pairs);
    delete list;
    return 0;
}

}  // extern "C"
