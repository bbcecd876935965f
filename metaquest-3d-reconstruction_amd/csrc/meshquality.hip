// meshquality.hip -- the reference's intrinsic mesh quality metrics on the device.
//
// Reference: scripts/evaluation/evaluate_fbx_quality.py, compute_raw_metrics_for_mesh: pure-Python loops
// over every triangle and every edge (shape, topology, smoothness, completeness, colour).  The rules are
// restated in DESIGN §2.5; all arithmetic is float64 on the float32 inputs, a sum of squares is
// (x^2 + y^2) + z^2, and the file is built with -ffp-contract=off.
//
// Device work: an index check and a vertex pass (finite check, bounding box by integer atomics on
// order-preserving keys) -> host reads two flags -> density histogram (LDS, integer atomics) ->
// per-triangle shape terms and unnormalised normals -> stable radix sort of the corner list by vertex id
// and one walk per vertex (vertex normals in Open3D's accumulation order, no float atomics) -> the sorted
// edge list of mesh_edges.hpp (loop edges dropped) -> its union-find over vertices by run heads -> two
// passes over run heads (sums, then squared deviations from the means).  Every mean and std is an
// order-fixed float64 reduction (device_prims.hpp's slab per workgroup, the slabs summed by one workgroup
// in a fixed order), so a repeated call is bit-identical.  Scratch is one block of the device-block cache.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <string>

#include "device_block.hpp"
#include "device_cub.hpp"
#include "device_prims.hpp"
#include "mesh_edges.hpp"
#include "mqr_common.hpp"
#include "pair_reduce.hpp"

namespace mqr {
namespace mq {
using namespace edges;

constexpr int kT = pairsum::kThreads;         // lanes of every workgroup here
constexpr int kPer = 4;                       // items per lane of the reducing kernels
constexpr int kTile = kT * kPer;              // items per workgroup (and per slab)
constexpr int kNS = 7;                        // sums of a slab
constexpr int kSlab = kNS + 2;                // ... then one min and one max
constexpr int kCells = 1000;                  // 10 x 10 x 10 density grid
constexpr double kEps = 1e-12;
constexpr double kTheta = 1.0471975511965976;   // radians(60)
constexpr double kRadToDeg = 57.29577951308232;  // 180 / pi, numpy's degrees() factor

// control words (one small device region; the box minimum is set to all ones, the rest to zero)
struct Ctrl {
    uint32_t bb[8];     // bounding box as order-preserving keys: min x y z, max x y z (two words unused)
    int32_t bad_index;  // a triangle index outside [0, nv)
    int32_t bad_coord;  // a non-finite coordinate
    int32_t roots;      // components of the vertex graph
    int32_t pad;
    int32_t hist[kCells];
};

struct Res {  // reduced slabs, read back by the host
    double shape[kSlab];
    double e0[kSlab];
    double e1[kSlab];
    double density_std;
};

// ------------------------------------------------------------------ checks, bounding box, density
// The finite check and the box in one pass over the positions (the reduction is block_bounds_atomic's).
__global__ void k_vertex_box(const float* __restrict__ pos, int64_t nv, Ctrl* c) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    uint32_t mn[3] = {~0u, ~0u, ~0u}, mx[3] = {0u, 0u, 0u};
    bool bad = false;
    for (int64_t i = i0; i < nv; i += step) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float f = pos[3 * i + a];
            bad |= !isfinite(f);
            const uint32_t k = ordered_u32(f);
            mn[a] = min(mn[a], k);
            mx[a] = max(mx[a], k);
        }
    }
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) c->bad_coord = 1;
    block_bounds_atomic(mn, mx, c->bb);
}

// The reference's voxel index per axis: clip(floor((p - min) / (extent / 10)), 0, 9), a true division.
__global__ void __launch_bounds__(kT) k_density_hist(const float* __restrict__ pos, int64_t nv, Ctrl* c) {
    __shared__ int32_t h[kCells];
    for (int j = threadIdx.x; j < kCells; j += kT) h[j] = 0;
    double lo[3], vox[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = (double)from_ordered(c->bb[a]);
        double ext = (double)from_ordered(c->bb[3 + a]) - lo[a];
        if (ext == 0.0) ext = 1e-6;
        vox[a] = ext / 10.0;
    }
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * kT;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < nv; i += step) {
        int cell = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double r = floor(((double)pos[3 * i + a] - lo[a]) / vox[a]);
            const int q = r < 0.0 ? 0 : r > 9.0 ? 9 : (int)r;
            cell = cell * 10 + q;
        }
        atomicAdd(&h[cell], 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < kCells; j += kT)
        if (h[j]) atomicAdd(&c->hist[j], h[j]);
}

// the workgroup's sum of v in a fixed order, returned to every lane
__device__ inline double block_sum(double v, double (&sh)[kT / 64]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();  // the previous call's readers are done with sh
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// population std of count / voxel volume over the non-empty cells (mean first, then squared deviations)
__global__ void __launch_bounds__(kT) k_density_std(const Ctrl* __restrict__ c, Res* res) {
    __shared__ double sh[kT / 64];
    double vox[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double ext = (double)from_ordered(c->bb[3 + a]) - (double)from_ordered(c->bb[a]);
        if (ext == 0.0) ext = 1e-6;
        vox[a] = ext / 10.0;
    }
    double vol = (vox[0] * vox[1]) * vox[2];
    if (vol <= 0.0) vol = 1.0;
    double x[(kCells + kT - 1) / kT];
    double s = 0.0, n = 0.0;
#pragma unroll
    for (int k = 0; k < (kCells + kT - 1) / kT; ++k) {
        const int j = k * kT + threadIdx.x;
        const int32_t cnt = j < kCells ? c->hist[j] : 0;
        x[k] = cnt > 0 ? (double)cnt / vol : -1.0;
        if (cnt > 0) s += x[k], n += 1.0;
    }
    s = block_sum(s, sh);
    n = block_sum(n, sh);
    const double mean = s / n;  // n >= 1: the mesh has a vertex
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < (kCells + kT - 1) / kT; ++k)
        if (x[k] >= 0.0) d2 += (x[k] - mean) * (x[k] - mean);
    d2 = block_sum(d2, sh);
    if (threadIdx.x == 0) res->density_std = sqrt(d2 / n);
}

// ------------------------------------------------------------------ triangles
__device__ inline double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }
__device__ inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ inline double clip1(double c) { return c < -1.0 ? -1.0 : c > 1.0 ? 1.0 : c; }

// a / |a| as Eigen's normalize() leaves it: a zero vector stays zero
__device__ inline void unit3(const double* a, double* o) {
    const double z = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    if (z > 0.0) {
        const double l = sqrt(z);
        o[0] = a[0] / l, o[1] = a[1] / l, o[2] = a[2] / l;
    } else {
        o[0] = a[0], o[1] = a[1], o[2] = a[2];
    }
}

// degrees(acos(clip(a^ . b^))) with a^ = a / (|a| + 1e-12): the reference's dihedral_angle
__device__ inline double angle_deg_eps(const double* a, const double* b) {
    const double la = norm3(a[0], a[1], a[2]) + kEps, lb = norm3(b[0], b[1], b[2]) + kEps;
    const double an[3] = {a[0] / la, a[1] / la, a[2] / la}, bn[3] = {b[0] / lb, b[1] / lb, b[2] / lb};
    return acos(clip1(dot3(an, bn))) * kRadToDeg;
}

// Per triangle: the unnormalised normal (p1 - p0) x (p2 - p0) into tn; for the non-degenerate ones the
// aspect ratio and the equiangle skewness, reduced into one slab per workgroup (count, sum, sum).
__global__ void __launch_bounds__(kT) k_shape(const float* __restrict__ pos, const int32_t* __restrict__ tri, int64_t nt,
                                              double* __restrict__ tn, double* __restrict__ slabs) {
    double acc[kNS];
#pragma unroll
    for (int j = 0; j < kNS; ++j) acc[j] = 0.0;
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
        const double ea[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};  // v1 - v0
        const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};  // v2 - v0
        const double n0 = ea[1] * e2[2] - ea[2] * e2[1], n1 = ea[2] * e2[0] - ea[0] * e2[2],
                     n2 = ea[0] * e2[1] - ea[1] * e2[0];
        tn[3 * t] = n0, tn[3 * t + 1] = n1, tn[3 * t + 2] = n2;
        if (i0 == i1 || i1 == i2 || i2 == i0) continue;
        if (0.5 * norm3(n0, n1, n2) < 1e-10) continue;
        const double eb[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};  // v2 - v1
        const double ec[3] = {p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2]};  // v0 - v2
        const double la = norm3(ea[0], ea[1], ea[2]), lb = norm3(eb[0], eb[1], eb[2]), lc = norm3(ec[0], ec[1], ec[2]);
        const double emin = fmax(fmin(la, fmin(lb, lc)), 1e-12), emax = fmax(la, fmax(lb, lc));
        // the corner angles: at v0 between (v1 - v0, v2 - v0), at v1 (v2 - v1, v0 - v1), at v2 (v0 - v2, v1 - v2),
        // each vector divided by (its length + 1e-12); v0 - v1 = -(v1 - v0) exactly, and so are its quotients
        const double da = la + kEps, db = lb + kEps, d2 = norm3(e2[0], e2[1], e2[2]) + kEps, dc = lc + kEps;
        const double ua[3] = {ea[0] / da, ea[1] / da, ea[2] / da}, ub[3] = {eb[0] / db, eb[1] / db, eb[2] / db};
        const double u2[3] = {e2[0] / d2, e2[1] / d2, e2[2] / d2}, uc[3] = {ec[0] / dc, ec[1] / dc, ec[2] / dc};
        const double ma[3] = {-ua[0], -ua[1], -ua[2]}, mb[3] = {-ub[0], -ub[1], -ub[2]};
        const double a0 = acos(clip1(dot3(ua, u2))), a1 = acos(clip1(dot3(ub, ma))), a2 = acos(clip1(dot3(uc, mb)));
        const double amin = fmin(a0, fmin(a1, a2)), amax = fmax(a0, fmax(a1, a2));
        double sk = fmax((kTheta - amin) / kTheta, (amax - kTheta) / kTheta);
        sk = sk < 0.0 ? 0.0 : sk > 1.0 ? 1.0 : sk;
        acc[0] += 1.0;
        acc[1] += emax / emin;
        acc[2] += sk;
    }
    block_sums_minmax_to_slab(acc, INFINITY, -INFINITY, slabs + (int64_t)blockIdx.x * kSlab);
}

// ------------------------------------------------------------------ vertex normals
__global__ void k_corner_keys(const int32_t* __restrict__ tri, int64_t m, uint32_t* key, int32_t* corner) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    key[i] = (uint32_t)tri[i];
    corner[i] = (int32_t)i;
}

// The corner list sorted (stably) by vertex id: the head of a vertex's run adds the unnormalised triangle
// normals of its corners in list order -- ascending triangle, corners 0, 1, 2 within one, which is the order
// Open3D's loop adds them in -- and writes the normalised sum.  Unreferenced vertices keep zero.
__global__ void k_vertex_normals(const uint32_t* __restrict__ key, const int32_t* __restrict__ corner, int64_t m,
                                 const double* __restrict__ tn, double* __restrict__ vn) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t v = key[i];
    if (i > 0 && key[i - 1] == v) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t j = i; j < m && key[j] == v; ++j) {
        const double* n = tn + 3 * (int64_t)(corner[j] / 3);
        s[0] += n[0], s[1] += n[1], s[2] += n[2];
    }
    double u[3];
    unit3(s, u);
    vn[3 * (int64_t)v] = u[0], vn[3 * (int64_t)v + 1] = u[1], vn[3 * (int64_t)v + 2] = u[2];
}

// ------------------------------------------------------------------ edges
// union-find over vertices, hooked by each distinct edge
__global__ void k_union_vertices(const uint64_t* __restrict__ keys, int64_t m, uint64_t none, int32_t* parent) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = keys[i];
    if (k == none || !run_head(keys, i, k)) return;
    uf_union(parent, (int32_t)(k >> 32), (int32_t)(uint32_t)k);
}

// Hooks only ever re-parent a root and halving only writes non-roots, so after the unions the roots are
// exactly the vertices that are their own parent (unreferenced vertices included).
__global__ void k_count_roots(const int32_t* __restrict__ parent, int64_t nv, Ctrl* c) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = i < nv && parent[i] == (int32_t)i;
    const uint64_t b = __ballot(root);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(&c->roots, __popcll(b));
}

// Run heads of the sorted edge entries.  PASS 0: slab sums [distinct, boundary, non-manifold, 2-runs, sum of
// the vertex-normal deviation, sum of the colour difference, sum of the dihedral] and the dihedral min / max.
// PASS 1: [sum (colour - mean)^2, sum (dihedral - mean)^2] with the means from PASS 0's reduced slab `e0`.
template <int PASS>
__global__ void __launch_bounds__(kT) k_edge_pass(const uint64_t* __restrict__ keys, const int32_t* __restrict__ slot,
                                                  int64_t m, uint64_t none, const double* __restrict__ vn,
                                                  const double* __restrict__ tn, const float* __restrict__ col,
                                                  const double* __restrict__ e0, double* __restrict__ slabs) {
    double acc[kNS];
#pragma unroll
    for (int j = 0; j < kNS; ++j) acc[j] = 0.0;
    double mn = INFINITY, mx = -INFINITY;
    double col_mean = 0.0, dih_mean = 0.0;
    if (PASS == 1) {
        col_mean = e0[5] / e0[0];  // used only where an edge exists (e0[0] > 0)
        dih_mean = e0[6] / e0[3];  // ... where a 2-run exists (e0[3] > 0)
    }
    for (int kk = 0; kk < kPer; ++kk) {
        const int64_t i = (int64_t)blockIdx.x * kTile + kk * kT + threadIdx.x;
        if (i >= m) continue;
        const uint64_t k = keys[i];
        if (k == none || !run_head(keys, i, k)) continue;
        const int mult = run_length3(keys, m, i);
        const int64_t u = (int64_t)(k >> 32), v = (int64_t)(uint32_t)k;
        if (PASS == 0) {
            acc[0] += 1.0;
            if (mult == 1) acc[1] += 1.0;
            if (mult > 2) acc[2] += 1.0;
            const double* n1 = vn + 3 * u;
            const double* n2 = vn + 3 * v;
            const double den = (norm3(n1[0], n1[1], n1[2]) + kEps) * (norm3(n2[0], n2[1], n2[2]) + kEps);
            acc[4] += acos(clip1(dot3(n1, n2) / den)) * kRadToDeg;
        }
        if (col) {
            const double d0 = (double)col[3 * u] - (double)col[3 * v], d1 = (double)col[3 * u + 1] - (double)col[3 * v + 1],
                         d2 = (double)col[3 * u + 2] - (double)col[3 * v + 2];
            const double g = norm3(d0, d1, d2);
            if (PASS == 0) acc[5] += g;
            else acc[0] += (g - col_mean) * (g - col_mean);
        }
        if (mult == 2) {
            double a[3], b[3];
            unit3(tn + 3 * (int64_t)(slot[i] / 3), a);  // compute_triangle_normals normalises ...
            unit3(tn + 3 * (int64_t)(slot[i + 1] / 3), b);
            const double d = angle_deg_eps(a, b);  // ... and dihedral_angle divides by (|n| + 1e-12) again
            if (PASS == 0) {
                acc[3] += 1.0;
                acc[6] += d;
                mn = fmin(mn, d);
                mx = fmax(mx, d);
            } else {
                acc[1] += (d - dih_mean) * (d - dih_mean);
            }
        }
    }
    block_sums_minmax_to_slab(acc, mn, mx, slabs + (int64_t)blockIdx.x * kSlab);
}

// ------------------------------------------------------------------ host
static StreamTable g_streams;

}  // namespace mq
}  // namespace mqr

using namespace mqr;
using namespace mqr::mq;

extern "C" {

int mqr_mesh_quality(int device, const float* vertices, int64_t nv, const float* colors, const int32_t* triangles,
                     int64_t nt, int loc, mqr_quality_metrics* out) {
    MQR_REQUIRE(out, "null argument");
    MQR_REQUIRE(nv > 0 && nt > 0, "mesh quality: the mesh has no geometry (no vertices or no triangles)");
    MQR_REQUIRE(vertices && triangles, "null argument");
    MQR_REQUIRE(loc == MQR_HOST || loc == MQR_DEVICE, "mesh quality: loc must be MQR_HOST or MQR_DEVICE");
    MQR_REQUIRE(nt < ((int64_t)1 << 31) / 3 && nv < ((int64_t)1 << 31), "mesh quality: mesh too large (3 nt >= 2^31)");
    MQR_CHECK_HIP(hipSetDevice(device));
    hipStream_t s = g_streams.get(device);
    MQR_REQUIRE(s, "mesh quality: no stream for the device");

    const int64_t m = 3 * nt;
    const int vbits = ceil_log2(nv + 1);  // bits of a vertex id, and of `nv` itself (the dropped-edge key)
    const uint64_t none = (uint64_t)nv << 32 | (uint64_t)nv;
    const int64_t nblk_t = nb(nt, kTile), nblk_e = nb(m, kTile);

    const bool host_in = loc == MQR_HOST;
    const size_t b_pos = sizeof(float) * 3 * nv, b_tri = sizeof(int32_t) * m;
    ScratchLayout L;
    float *d_pos, *d_col;
    int32_t *d_tri, *parent, *slot, *slot_s;
    Ctrl* ctrl;
    Res* res;
    double *tn, *vn, *slabs;
    uint64_t *keys, *keys_s;
    L.add(d_pos, 3 * nv, host_in);
    L.add(d_col, 3 * nv, host_in && colors);
    L.add(d_tri, m, host_in);
    L.add_each(1, ctrl, res);
    L.add(tn, 3 * nt);
    L.add(vn, 3 * nv);
    L.add(parent, nv);
    L.add_each(m, keys, keys_s, slot, slot_s);
    L.add(slabs, kSlab * nblk_e);
    // the two radix sorts; the corner sort borrows the edge sort's buffers
    auto sort_corners = [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, (const uint32_t*)keys, (uint32_t*)keys_s, (const int32_t*)slot,
                                                  slot_s, (int)m, 0, vbits, s);
    };
    auto sort_edges = [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, (const uint64_t*)keys, keys_s, (const int32_t*)slot, slot_s,
                                                  (int)m, 0, 32 + vbits, s);
    };
    CubTemp tmp;
    MQR_CHECK_HIP(tmp.lay_out(L, sort_corners, sort_edges));
    CachedBlock blk(device, L);
    if (!blk.p) return scratch_failed("mesh quality", L.total());

    const float* pos = vertices;
    const float* col = colors;
    const int32_t* tri = triangles;
    if (host_in) {
        if (copy_to_device(device, d_pos, vertices, b_pos, s) || copy_to_device(device, d_tri, triangles, b_tri, s) ||
            (colors && copy_to_device(device, d_col, colors, b_pos, s)))
            return 1;
        pos = d_pos, col = d_col, tri = d_tri;
    } else if (order_after_caller(device, s)) {
        return 2;
    }
    StreamDrain drain{s};

    // ---- checks (no kernel gathers through an index before the flags are read)
    MQR_CHECK_HIP(hipMemsetAsync(ctrl, 0, sizeof(Ctrl), s));
    MQR_CHECK_HIP(hipMemsetAsync(ctrl->bb, 0xff, 3 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_check_indices, dim3(nb(m)), dim3(kT), 0, s, tri, m, nv, &ctrl->bad_index);
    hipLaunchKernelGGL(k_vertex_box, dim3(std::min<unsigned>(nb(nv), 4096)), dim3(kT), 0, s, pos, nv, ctrl);
    MQR_CHECK_HIP(hipGetLastError());
    int32_t flags[2] = {0, 0};
    MQR_CHECK_HIP(hipMemcpyAsync(flags, &ctrl->bad_index, sizeof(flags), hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));
    MQR_REQUIRE(!flags[0], "mesh quality: a triangle index is outside [0, nv)");
    MQR_REQUIRE(!flags[1], "mesh quality: a vertex coordinate is not finite");

    // ---- completeness
    hipLaunchKernelGGL(k_density_hist, dim3(std::min<unsigned>(nb(nv, kTile), 1024)), dim3(kT), 0, s, pos, nv, ctrl);
    hipLaunchKernelGGL(k_density_std, dim3(1), dim3(kT), 0, s, ctrl, res);
    // ---- shape, triangle normals
    hipLaunchKernelGGL(k_shape, dim3((unsigned)nblk_t), dim3(kT), 0, s, pos, tri, nt, tn, slabs);
    hipLaunchKernelGGL(k_reduce_slabs<kNS>, dim3(1), dim3(kT), 0, s, slabs, nblk_t, res->shape);
    MQR_CHECK_HIP(hipGetLastError());
    // ---- vertex normals: the corner sort borrows the edge sort's buffers
    {
        uint32_t* ck = (uint32_t*)keys;
        const uint32_t* ck_s = (const uint32_t*)keys_s;
        hipLaunchKernelGGL(k_corner_keys, dim3(nb(m)), dim3(kT), 0, s, tri, m, ck, slot);
        MQR_CHECK_HIP(hipGetLastError());
        MQR_CHECK_HIP(tmp.run(sort_corners));
        MQR_CHECK_HIP(hipMemsetAsync(vn, 0, sizeof(double) * 3 * nv, s));
        hipLaunchKernelGGL(k_vertex_normals, dim3(nb(m)), dim3(kT), 0, s, ck_s, slot_s, m, tn, vn);
        MQR_CHECK_HIP(hipGetLastError());
    }
    // ---- topology
    hipLaunchKernelGGL(k_edge_keys<true>, dim3(nb(m)), dim3(kT), 0, s, tri, nt, none, keys, slot);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(tmp.run(sort_edges));
    hipLaunchKernelGGL(k_iota, dim3(nb(nv)), dim3(kT), 0, s, parent, nv);
    hipLaunchKernelGGL(k_union_vertices, dim3(nb(m)), dim3(kT), 0, s, keys_s, m, none, parent);
    hipLaunchKernelGGL(k_count_roots, dim3(nb(nv)), dim3(kT), 0, s, parent, nv, ctrl);
    MQR_CHECK_HIP(hipGetLastError());
    // ---- smoothness and colour over run heads: sums, then squared deviations
    hipLaunchKernelGGL(k_edge_pass<0>, dim3((unsigned)nblk_e), dim3(kT), 0, s, keys_s, slot_s, m, none, vn, tn, col,
                       (const double*)nullptr, slabs);
    hipLaunchKernelGGL(k_reduce_slabs<kNS>, dim3(1), dim3(kT), 0, s, slabs, nblk_e, res->e0);
    hipLaunchKernelGGL(k_edge_pass<1>, dim3((unsigned)nblk_e), dim3(kT), 0, s, keys_s, slot_s, m, none, vn, tn, col,
                       (const double*)res->e0, slabs);
    hipLaunchKernelGGL(k_reduce_slabs<kNS>, dim3(1), dim3(kT), 0, s, slabs, nblk_e, res->e1);
    MQR_CHECK_HIP(hipGetLastError());

    Res h;
    int32_t roots = 0;
    MQR_CHECK_HIP(hipMemcpyAsync(&h, res, sizeof(Res), hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipMemcpyAsync(&roots, &ctrl->roots, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MQR_CHECK_HIP(hipStreamSynchronize(s));

    // ---- the reference's closing arithmetic (counts are exact in float64: all < 2^31)
    mqr_quality_metrics q{};
    const double valid = h.shape[0];
    q.mean_aspect_ratio = valid > 0 ? h.shape[1] / valid : 1.0;
    q.mean_skewness = valid > 0 ? h.shape[2] / valid : 0.0;
    q.degenerate_triangles = nt - (int64_t)valid;
    const double total = h.e0[0], boundary = h.e0[1], n2 = h.e0[3];
    q.non_manifold_edges = (int64_t)h.e0[2];
    q.boundary_edge_ratio = total > 0 ? boundary / total : 0.0;
    q.component_count = roots;
    q.total_edges = (int64_t)total;
    q.normal_deviation_avg_deg = total > 0 ? h.e0[4] / total : 0.0;
    if (n2 > 0) {
        q.dihedral_min_deg = h.e0[kNS];
        q.dihedral_max_deg = h.e0[kNS + 1];
        q.dihedral_penalty = std::max(0.0, 30.0 - q.dihedral_min_deg) + std::max(0.0, q.dihedral_max_deg - 170.0);
        q.surface_roughness = std::sqrt(h.e1[1] / n2);
    } else {
        q.dihedral_min_deg = 180.0;
        q.dihedral_max_deg = 0.0;
        q.dihedral_penalty = 0.0;
        q.surface_roughness = 0.0;
    }
    q.is_single_component = roots == 1;
    q.vertex_density_stddev = h.density_std;
    q.has_color = colors != nullptr;
    q.uncolored_vertex_ratio = colors ? 0.0 : 1.0;
    q.color_gradient_stddev = colors && total > 0 ? std::sqrt(h.e1[0] / total) : 0.0;
    q.is_manifold = q.non_manifold_edges == 0;
    q.is_watertight = q.is_manifold && boundary == 0 && roots == 1;
    q.num_vertices = nv;
    q.num_triangles = nt;
    *out = q;
    return 0;
}

}  // extern "C"
