// registration.hip -- batched fragment registration (DESIGN §2 row `registration`).
//
// Reference: refine_fragment_poses.py:122-271 registers every pair of fragment clouds with Open3D's
// evaluate_registration, multi_scale_icp (point to point) and get_information_matrix, one pair at a
// time.  Here a CLOUD SET keeps N clouds in HBM and caches, per cloud, the point selections
// (full / every k-th / voxel down-sample) and a uniform-grid index per (selection, cell edge); the
// three pair operations run over a whole batch of pairs in one launch, grid = (blocks, pairs).
//
// Everything that decides a result is float64 and order-fixed (DESIGN "registration rules"):
//   voxel key     floor((double)p / v) per axis; stable radix sort of the packed (kx, ky, kz) key;
//                 one thread per voxel sums its members in ascending original index
//   query         q = R p + t in float64 from the ORIGINAL float32 point and the pair's float64 T
//   search        the 27 cells around q (cell edge = radius): 9 runs of 3 z-adjacent cells, each a
//                 contiguous range of the sorted keys found by binary search; d^2 in float64;
//                 accept d^2 <= r^2; ties go to the lower view index
//   reduction     per workgroup a fixed butterfly over lanes, then the four waves in order through
//                 LDS; one slab of float64 partials per (pair, workgroup); a per-pair kernel sums
//                 the slabs in workgroup order.  No float atomics: a repeated call is bit-identical.
//   Kabsch        Horn's quaternion: cyclic Jacobi on the symmetric 4x4 in float64 (always a proper
//                 rotation, which is what the SVD form gives after its determinant fix)
// A level's iterations are enqueued back to back; a pair that has finished sets a flag its later
// launches return on, and the host reads the per-pair state once per level.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "device_block.hpp"
#include "device_cub.hpp"
#include "device_prims.hpp"
#include "mqr_common.hpp"
#include "pair_reduce.hpp"

namespace mqr {
namespace reg {

using pairsum::kInfoSums;  // count, 21 unique entries of sum G^T G
using pairsum::kThreads;
using pairsum::kWaves;
constexpr int kIcpSums = 17;   // count, sum q (3), sum t (3), sum q t^T (9), sum d^2
constexpr double kCellLimit = 1048575.0;  // |cell index| < 2^20 per axis (pack_key)
constexpr float kCoordLimit = 3.0e38f;    // a cloud's coordinates pass k_check_finite within it

struct PairDesc {
    const float* src;       // source selection, view order
    const float* tpts;      // target selection in grid (sorted) order
    const uint64_t* tkeys;  // sorted cell keys of the target grid
    const int32_t* torder;  // grid position -> view index
    int32_t ns, nt, nblk, slab_off;
};

struct PairState {
    double T[16];
    double prev_fit, prev_rmse, fit, rmse, count;
    int32_t iters, done;
};

// ------------------------------------------------------------------ kernels
__global__ void k_every_k(const float* __restrict__ p, int64_t m, int64_t k, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    for (int a = 0; a < 3; ++a) out[3 * i + a] = p[3 * i * k + a];
}

// packed cell key of every point (cell edge e), idx = iota; a cell index beyond 2^20 raises bit 1
__global__ void k_cell_keys(const float* __restrict__ p, int64_t n, double e, uint64_t* keys, int32_t* idx, int* bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double kx = floor((double)p[3 * i] / e), ky = floor((double)p[3 * i + 1] / e),
                 kz = floor((double)p[3 * i + 2] / e);
    const bool ok = fabs(kx) <= kCellLimit - 1 && fabs(ky) <= kCellLimit - 1 && fabs(kz) <= kCellLimit - 1;
    if (!ok) atomicOr(bad, 2);
    keys[i] = ok ? pack_key((int)kx, (int)ky, (int)kz) : 0;
    idx[i] = (int32_t)i;
}

__global__ void k_heads(const uint64_t* __restrict__ keys, int64_t n, uint8_t* head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) head[i] = i == 0 || keys[i] != keys[i - 1];
}

// one thread per voxel: members [start[v], start[v + 1]) of the stably sorted list, i.e. in
// ascending original index, summed in float64, divided by the count, rounded to float32
__global__ void k_voxel_mean(const float* __restrict__ p, const int32_t* __restrict__ idx,
                             const int32_t* __restrict__ start, int64_t m, int64_t n, float* out) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m) return;
    const int64_t a = start[v], b = v + 1 < m ? start[v + 1] : n;
    double sx = 0, sy = 0, sz = 0;
    for (int64_t j = a; j < b; ++j) {
        const float* q = p + 3 * (int64_t)idx[j];
        sx += (double)q[0];
        sy += (double)q[1];
        sz += (double)q[2];
    }
    const double c = (double)(b - a);
    out[3 * v] = (float)(sx / c);
    out[3 * v + 1] = (float)(sy / c);
    out[3 * v + 2] = (float)(sz / c);
}

__global__ void k_gather_points(const float* __restrict__ p, const int32_t* __restrict__ idx, int64_t n, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = p + 3 * (int64_t)idx[i];
    out[3 * i] = q[0];
    out[3 * i + 1] = q[1];
    out[3 * i + 2] = q[2];
}

__global__ void k_level_init(PairState* st, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st[i].prev_fit = st[i].prev_rmse = st[i].fit = st[i].rmse = st[i].count = 0.0;
    st[i].iters = 0;
    st[i].done = 0;
}

__device__ inline int32_t lower_bound(const uint64_t* __restrict__ keys, int32_t n, uint64_t k) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// nearest target within the radius (squared r2) of q; returns its grid position or -1
__device__ inline int32_t nearest(const PairDesc& d, double qx, double qy, double qz, double cell, double r2,
                                  double& best_d2) {
    // clamped so that the three neighbours stay inside the key range; a NaN query clamps too
    const double lim = kCellLimit - 2;
    const int cx = (int)fmin(fmax(floor(qx / cell), -lim), lim);
    const int cy = (int)fmin(fmax(floor(qy / cell), -lim), lim);
    const int cz = (int)fmin(fmax(floor(qz / cell), -lim), lim);
    int32_t best = -1, best_view = 0x7fffffff;
    best_d2 = r2;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy) {
            const uint64_t klo = pack_key(cx + dx, cy + dy, cz - 1), khi = pack_key(cx + dx, cy + dy, cz + 1);
            for (int32_t j = lower_bound(d.tkeys, d.nt, klo); j < d.nt && d.tkeys[j] <= khi; ++j) {
                const double ex = qx - (double)d.tpts[3 * (int64_t)j], ey = qy - (double)d.tpts[3 * (int64_t)j + 1],
                             ez = qz - (double)d.tpts[3 * (int64_t)j + 2];
                const double d2 = (ex * ex + ey * ey) + ez * ez;
                if (d2 > best_d2) continue;
                const int32_t view = d.torder[j];
                if (d2 < best_d2 || best < 0 || view < best_view) {
                    best = j;
                    best_view = view;
                    best_d2 = d2;
                }
            }
        }
    return best;
}

// Correspondence + accumulate.  MODE 0: the ICP sums (kIcpSums), MODE 1: the information sums
// (kInfoSums).  One lane per source point; slab (slab_off + blockIdx.x) receives the workgroup's sums.
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_corr(const PairDesc* __restrict__ pd, const PairState* __restrict__ st,
                                                   double radius, double* __restrict__ slabs) {
    constexpr int NS = MODE == 0 ? kIcpSums : kInfoSums;
    __shared__ double sh[kWaves][NS];
    const int pair = blockIdx.y;
    const PairDesc d = pd[pair];
    if ((int)blockIdx.x >= d.nblk || st[pair].done) return;  // uniform over the workgroup
    const double* T = st[pair].T;
    double acc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.0;
    const int32_t i = (int32_t)blockIdx.x * kThreads + (int32_t)threadIdx.x;
    if (i < d.ns) {
        const double px = (double)d.src[3 * (int64_t)i], py = (double)d.src[3 * (int64_t)i + 1],
                     pz = (double)d.src[3 * (int64_t)i + 2];
        const double qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
        const double qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
        const double qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
        double d2;
        const int32_t j = nearest(d, qx, qy, qz, radius, radius * radius, d2);
        if (j >= 0) {
            const double tx = (double)d.tpts[3 * (int64_t)j], ty = (double)d.tpts[3 * (int64_t)j + 1],
                         tz = (double)d.tpts[3 * (int64_t)j + 2];
            acc[0] = 1.0;
            if constexpr (MODE == 0) {
                acc[1] = qx, acc[2] = qy, acc[3] = qz;
                acc[4] = tx, acc[5] = ty, acc[6] = tz;
                acc[7] = qx * tx, acc[8] = qx * ty, acc[9] = qx * tz;
                acc[10] = qy * tx, acc[11] = qy * ty, acc[12] = qy * tz;
                acc[13] = qz * tx, acc[14] = qz * ty, acc[15] = qz * tz;
                acc[16] = d2;
            } else {
                pairsum::info_sums(1.0, tx, ty, tz, tx * tx, ty * ty, tz * tz, tx * ty, tx * tz, ty * tz, acc);
            }
        }
    }
    pairsum::block_sums_to_slab<NS>(acc, sh, slabs + ((int64_t)d.slab_off + blockIdx.x) * NS);
}

// largest eigenvector of the symmetric 4x4 N (cyclic Jacobi), as a unit quaternion (w, x, y, z)
__device__ inline void horn_quaternion(double A[4][4], double q[4]) {
    double V[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) V[a][b] = a == b ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) (a == b ? diag : off) += A[a][b] * A[a][b];
        if (off <= 1e-40 * diag || off == 0.0) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int r = p + 1; r < 4; ++r) {
                const double apq = A[p][r];
                if (apq == 0.0) continue;
                const double theta = (A[r][r] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {  // A <- A J, V <- V J
                    const double akp = A[k][p], akq = A[k][r];
                    A[k][p] = c * akp - s * akq;
                    A[k][r] = s * akp + c * akq;
                    const double vkp = V[k][p], vkq = V[k][r];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][r] = s * vkp + c * vkq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {  // A <- J^T A
                    const double apk = A[p][k], aqk = A[r][k];
                    A[p][k] = c * apk - s * aqk;
                    A[r][k] = s * apk + c * aqk;
                }
            }
    }
    int best = 0;
#pragma unroll
    for (int a = 1; a < 4; ++a)
        if (A[a][a] > A[best][best]) best = a;
    double nrm = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        q[a] = best == 0 ? V[a][0] : best == 1 ? V[a][1] : best == 2 ? V[a][2] : V[a][3];
        nrm += q[a] * q[a];
    }
    nrm = sqrt(nrm);
#pragma unroll
    for (int a = 0; a < 4; ++a) q[a] /= nrm;
}

// One workgroup (one wave) per pair: sum the slabs in workgroup order, fitness / rmse of the current
// T, then (update != 0) the Kabsch step T <- dT T and the convergence test of the level.
__global__ __launch_bounds__(64) void k_finalize(const PairDesc* __restrict__ pd, PairState* st,
                                                 const double* __restrict__ slabs, int update, double rel_fit,
                                                 double rel_rmse) {
    __shared__ double S[kIcpSums];
    const int pair = blockIdx.x;
    const PairDesc d = pd[pair];
    PairState& s = st[pair];
    if (s.done) return;
    if (threadIdx.x < kIcpSums) {
        double v = 0.0;
        for (int b = 0; b < d.nblk; ++b) v += slabs[((int64_t)d.slab_off + b) * kIcpSums + threadIdx.x];
        S[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = S[0];
    const double fit = n / (double)d.ns, rmse = n > 0.0 ? sqrt(S[16] / n) : 0.0;
    s.fit = fit;
    s.rmse = rmse;
    s.count = n;
    s.iters += 1;
    if (!update || n < 3.0) {
        s.done = 1;
        return;
    }
    double mq[3], mt[3], H[3][3];
    for (int a = 0; a < 3; ++a) mq[a] = S[1 + a] / n, mt[a] = S[4 + a] / n;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) H[a][b] = S[7 + 3 * a + b] / n - mq[a] * mt[b];
    double N[4][4];
    N[0][0] = H[0][0] + H[1][1] + H[2][2];
    N[1][1] = H[0][0] - H[1][1] - H[2][2];
    N[2][2] = -H[0][0] + H[1][1] - H[2][2];
    N[3][3] = -H[0][0] - H[1][1] + H[2][2];
    N[0][1] = N[1][0] = H[1][2] - H[2][1];
    N[0][2] = N[2][0] = H[2][0] - H[0][2];
    N[0][3] = N[3][0] = H[0][1] - H[1][0];
    N[1][2] = N[2][1] = H[0][1] + H[1][0];
    N[1][3] = N[3][1] = H[2][0] + H[0][2];
    N[2][3] = N[3][2] = H[1][2] + H[2][1];
    double q[4];
    horn_quaternion(N, q);
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z), R[0][1] = 2.0 * (x * y - w * z), R[0][2] = 2.0 * (x * z + w * y);
    R[1][0] = 2.0 * (x * y + w * z), R[1][1] = 1.0 - 2.0 * (x * x + z * z), R[1][2] = 2.0 * (y * z - w * x);
    R[2][0] = 2.0 * (x * z - w * y), R[2][1] = 2.0 * (y * z + w * x), R[2][2] = 1.0 - 2.0 * (x * x + y * y);
    double D[3][4], Tn[3][4];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) D[a][b] = R[a][b];
        D[a][3] = mt[a] - ((R[a][0] * mq[0] + R[a][1] * mq[1]) + R[a][2] * mq[2]);
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b)
            Tn[a][b] = ((D[a][0] * s.T[b] + D[a][1] * s.T[4 + b]) + D[a][2] * s.T[8 + b]) + (b == 3 ? D[a][3] : 0.0);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b) s.T[4 * a + b] = Tn[a][b];
    if (fabs(s.prev_fit - fit) < rel_fit && fabs(s.prev_rmse - rmse) < rel_rmse) {
        s.done = 1;
        return;
    }
    s.prev_fit = fit;
    s.prev_rmse = rmse;
}

// information: sum the slabs in workgroup order and spread the 21 sums over the symmetric 6x6
__global__ __launch_bounds__(64) void k_finalize_info(const PairDesc* __restrict__ pd, const double* __restrict__ slabs,
                                                      double* info) {
    __shared__ double S[kInfoSums];
    const int pair = blockIdx.x;
    const PairDesc d = pd[pair];
    pairsum::info_from_slabs(slabs, d.slab_off, d.nblk, S, info + 36 * (int64_t)pair);
}

// ------------------------------------------------------------------ host side
struct Selection {  // points of one (cloud, kind, parameter)
    const float* pts = nullptr;
    int64_t n = 0;
    float* owned = nullptr;
};
struct Grid {  // uniform-grid index of one selection at one cell edge
    uint64_t* keys = nullptr;
    int32_t* order = nullptr;
    float* pts = nullptr;
};
enum Kind : int { kFull = 0, kEveryK = 1, kVoxel = 2 };
typedef std::tuple<int, int, uint64_t> SelKey;             // cloud, kind, parameter bits
typedef std::tuple<int, int, uint64_t, uint64_t> GridKey;  // + cell edge bits

inline uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}

}  // namespace reg
}  // namespace mqr

using namespace mqr;
using namespace mqr::reg;

struct mqr_cloudset {
    int device = 0;
    hipStream_t s = nullptr;
    std::vector<const float*> pts;  // device pointers (caller's, or into `owned`)
    std::vector<int64_t> counts;
    std::vector<void*> owned;
    std::map<SelKey, Selection> sels;
    std::map<GridKey, Grid> grids;
    int* d_flag = nullptr;
    // grow-only scratch of the pair calls: 0 descriptors, 1 state, 2 slabs, 3 information
    GrowBuf scratch[4];

    void* get_scratch(int slot, size_t bytes) {  // nullptr when the device is out of memory
        (void)scratch[slot].reserve(bytes, std::max<size_t>(bytes + bytes / 2, 4096));
        return scratch[slot].p;
    }
};

namespace {

template <class T>
struct Tmp {  // device temporary of a view build
    T* p = nullptr;
    ~Tmp() {
        if (p) (void)hipFree(p);
    }
    int alloc(int64_t n) { return hipMalloc(&p, sizeof(T) * (size_t)std::max<int64_t>(n, 1)) != hipSuccess; }
};

// sorted (keys, idx) of the points at cell edge e; fails on a cell index beyond the key range
int sorted_keys(mqr_cloudset* cs, const float* pts, int64_t n, double e, uint64_t* keys_s, int32_t* idx_s) {
    Tmp<uint64_t> keys;
    Tmp<int32_t> idx;
    Tmp<char> tmp;
    if (keys.alloc(n) || idx.alloc(n)) {
        set_error("registration: device allocation failed");
        return 1;
    }
    MQR_CHECK_HIP(hipMemsetAsync(cs->d_flag, 0, sizeof(int), cs->s));
    hipLaunchKernelGGL(k_cell_keys, dim3(nb(n)), dim3(256), 0, cs->s, pts, n, e, keys.p, idx.p, cs->d_flag);
    MQR_CHECK_HIP(hipGetLastError());
    auto sort_cells = [&](void* t, size_t& b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, keys.p, keys_s, idx.p, idx_s, (int)n, 0, 63, cs->s);
    };
    CubTemp ct;
    MQR_CHECK_HIP(ct.size(sort_cells));
    if (tmp.alloc((int64_t)ct.bytes)) {
        set_error("registration: device allocation failed");
        return 1;
    }
    ct.p = tmp.p;
    MQR_CHECK_HIP(ct.run(sort_cells));
    int flag = 0;
    MQR_CHECK_HIP(hipMemcpyAsync(&flag, cs->d_flag, sizeof(int), hipMemcpyDeviceToHost, cs->s));
    MQR_CHECK_HIP(hipStreamSynchronize(cs->s));
    if (flag) {
        set_error("registration: a coordinate divided by the cell size " + std::to_string(e) +
                  " gives a cell index beyond 2^20, which the 63-bit key cannot hold");
        return 2;
    }
    return 0;
}

int get_selection(mqr_cloudset* cs, int cloud, int kind, double param, const Selection** out) {
    if (kind == kEveryK && param <= 1.0) kind = kFull;
    if (kind == kVoxel && !(param > 0.0)) kind = kFull;
    if (kind == kFull) param = 0.0;
    const SelKey key(cloud, kind, bits(param));
    auto it = cs->sels.find(key);
    if (it != cs->sels.end()) {
        *out = &it->second;
        return 0;
    }
    Selection sel;
    const float* src = cs->pts[cloud];
    const int64_t n = cs->counts[cloud];
    if (kind == kFull) {
        sel.pts = src;
        sel.n = n;
    } else if (kind == kEveryK) {
        const int64_t k = (int64_t)param, m = (n + k - 1) / k;
        MQR_CHECK_HIP(hipMalloc(&sel.owned, sizeof(float) * 3 * (size_t)m));
        hipLaunchKernelGGL(k_every_k, dim3(nb(m)), dim3(256), 0, cs->s, src, m, k, sel.owned);
        MQR_CHECK_HIP(hipGetLastError());
        sel.pts = sel.owned;
        sel.n = m;
    } else {
        Tmp<uint64_t> keys_s;
        Tmp<int32_t> idx_s, start, d_num;
        Tmp<uint8_t> head;
        Tmp<char> tmp;
        if (keys_s.alloc(n) || idx_s.alloc(n) || start.alloc(n) || d_num.alloc(1) || head.alloc(n)) {
            set_error("registration: device allocation failed");
            return 1;
        }
        if (int rc = sorted_keys(cs, src, n, param, keys_s.p, idx_s.p)) return rc;
        hipLaunchKernelGGL(k_heads, dim3(nb(n)), dim3(256), 0, cs->s, keys_s.p, n, head.p);
        MQR_CHECK_HIP(hipGetLastError());
        hipcub::CountingInputIterator<int32_t> iota(0);
        auto select_heads = [&](void* t, size_t& b) {
            return hipcub::DeviceSelect::Flagged(t, b, iota, head.p, start.p, d_num.p, (int)n, cs->s);
        };
        CubTemp ct;
        MQR_CHECK_HIP(ct.size(select_heads));
        if (tmp.alloc((int64_t)ct.bytes)) {
            set_error("registration: device allocation failed");
            return 1;
        }
        ct.p = tmp.p;
        MQR_CHECK_HIP(ct.run(select_heads));
        int32_t m = 0;
        MQR_CHECK_HIP(hipMemcpyAsync(&m, d_num.p, sizeof(int32_t), hipMemcpyDeviceToHost, cs->s));
        MQR_CHECK_HIP(hipStreamSynchronize(cs->s));
        if (m < 1 || m > n) {
            set_error("registration: voxel count out of range");
            return 1;
        }
        MQR_CHECK_HIP(hipMalloc(&sel.owned, sizeof(float) * 3 * (size_t)m));
        hipLaunchKernelGGL(k_voxel_mean, dim3(nb(m)), dim3(256), 0, cs->s, src, idx_s.p, start.p, (int64_t)m, n,
                           sel.owned);
        MQR_CHECK_HIP(hipGetLastError());
        MQR_CHECK_HIP(hipStreamSynchronize(cs->s));  // the temporaries go out of scope
        sel.pts = sel.owned;
        sel.n = m;
    }
    *out = &(cs->sels[key] = sel);
    return 0;
}

int get_grid(mqr_cloudset* cs, int cloud, int kind, double param, double cell, const Selection** sel_out,
             const Grid** out) {
    const Selection* sel = nullptr;
    if (int rc = get_selection(cs, cloud, kind, param, &sel)) return rc;
    *sel_out = sel;
    // the selection's normalised key (get_selection folds k <= 1 and v <= 0 into the full cloud)
    int nk = kind;
    double np_ = param;
    if (sel->pts == cs->pts[cloud]) nk = kFull, np_ = 0.0;
    const GridKey key(cloud, nk, bits(np_), bits(cell));
    auto it = cs->grids.find(key);
    if (it != cs->grids.end()) {
        *out = &it->second;
        return 0;
    }
    Grid g;
    const int64_t n = sel->n;
    MQR_CHECK_HIP(hipMalloc(&g.keys, sizeof(uint64_t) * (size_t)n));
    MQR_CHECK_HIP(hipMalloc(&g.order, sizeof(int32_t) * (size_t)n));
    MQR_CHECK_HIP(hipMalloc(&g.pts, sizeof(float) * 3 * (size_t)n));
    int rc = sorted_keys(cs, sel->pts, n, cell, g.keys, g.order);
    if (!rc) {
        hipLaunchKernelGGL(k_gather_points, dim3(nb(n)), dim3(256), 0, cs->s, sel->pts, g.order, n, g.pts);
        if (hipGetLastError() != hipSuccess) {
            set_error("registration: gather launch failed");
            rc = 1;
        }
    }
    if (rc) {
        (void)hipFree(g.keys);
        (void)hipFree(g.order);
        (void)hipFree(g.pts);
        return rc;
    }
    *out = &(cs->grids[key] = g);
    return 0;
}

struct Batch {
    PairDesc* d_desc = nullptr;
    PairState* d_state = nullptr;
    double* d_slabs = nullptr;
    int max_blk = 0;
};

// descriptors of one batch at one (selection, radius): builds the views it needs and uploads them
int make_batch(mqr_cloudset* cs, int n_pairs, const int32_t* src, const int32_t* tgt, int kind, double param,
               double radius, int n_sums, Batch* b) {
    std::vector<PairDesc> h((size_t)n_pairs);
    int64_t off = 0;
    b->max_blk = 1;
    for (int p = 0; p < n_pairs; ++p) {
        const Selection *ss = nullptr, *ts = nullptr;
        const Grid* g = nullptr;
        if (int rc = get_selection(cs, src[p], kind, param, &ss)) return rc;
        if (int rc = get_grid(cs, tgt[p], kind, param, radius, &ts, &g)) return rc;
        PairDesc& d = h[(size_t)p];
        d.src = ss->pts;
        d.ns = (int32_t)ss->n;
        d.tpts = g->pts;
        d.tkeys = g->keys;
        d.torder = g->order;
        d.nt = (int32_t)ts->n;
        d.nblk = (int32_t)((ss->n + kThreads - 1) / kThreads);
        d.slab_off = (int32_t)off;
        off += d.nblk;
        b->max_blk = std::max(b->max_blk, (int)d.nblk);
    }
    if (off >= ((int64_t)1 << 31) / kInfoSums) {
        set_error("registration: batch too large");
        return 2;
    }
    b->d_desc = static_cast<PairDesc*>(cs->get_scratch(0, sizeof(PairDesc) * (size_t)n_pairs));
    b->d_slabs = static_cast<double*>(cs->get_scratch(2, sizeof(double) * (size_t)n_sums * (size_t)off));
    if (!b->d_desc || !b->d_slabs) {
        set_error("registration: device allocation failed");
        return 1;
    }
    MQR_CHECK_HIP(hipMemcpyAsync(b->d_desc, h.data(), sizeof(PairDesc) * (size_t)n_pairs,
                                 hipMemcpyHostToDevice, cs->s));
    MQR_CHECK_HIP(hipStreamSynchronize(cs->s));  // `h` is pageable host memory
    return 0;
}

int check_pairs(mqr_cloudset* cs, int n_pairs, const int32_t* src, const int32_t* tgt) {
    MQR_REQUIRE(cs && src && tgt, "null argument");
    MQR_REQUIRE(n_pairs >= 1 && n_pairs <= 65535, "n_pairs must be in [1, 65535]");
    const int n = (int)cs->counts.size();
    for (int p = 0; p < n_pairs; ++p)
        MQR_REQUIRE(src[p] >= 0 && src[p] < n && tgt[p] >= 0 && tgt[p] < n, "cloud index out of range");
    return 0;
}

int upload_state(mqr_cloudset* cs, int n_pairs, const double* T, PairState** d_state) {
    std::vector<PairState> h((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        std::memset(&h[(size_t)p], 0, sizeof(PairState));
        for (int a = 0; a < 16; ++a) {
            MQR_REQUIRE(std::isfinite(T[16 * (size_t)p + a]), "non-finite transformation");
            h[(size_t)p].T[a] = T[16 * (size_t)p + a];
        }
    }
    *d_state = static_cast<PairState*>(cs->get_scratch(1, sizeof(PairState) * (size_t)n_pairs));
    MQR_REQUIRE(*d_state, "registration: device allocation failed");
    MQR_CHECK_HIP(hipMemcpyAsync(*d_state, h.data(), sizeof(PairState) * (size_t)n_pairs,
                                 hipMemcpyHostToDevice, cs->s));
    MQR_CHECK_HIP(hipStreamSynchronize(cs->s));
    return 0;
}

int download_state(mqr_cloudset* cs, int n_pairs, const PairState* d_state, std::vector<PairState>* h) {
    h->resize((size_t)n_pairs);
    MQR_CHECK_HIP(hipMemcpyAsync(h->data(), d_state, sizeof(PairState) * (size_t)n_pairs,
                                 hipMemcpyDeviceToHost, cs->s));
    MQR_CHECK_HIP(hipStreamSynchronize(cs->s));
    return 0;
}

}  // namespace

extern "C" {

int mqr_cloudset_create(int device, int n_clouds, const float* const* points, const int64_t* counts, int loc,
                        mqr_cloudset** out) {
    MQR_REQUIRE(out && points && counts, "null argument");
    MQR_REQUIRE(n_clouds >= 1, "a cloud set needs at least one cloud");
    MQR_REQUIRE(loc == MQR_HOST || loc == MQR_DEVICE, "loc must be MQR_HOST or MQR_DEVICE");
    for (int i = 0; i < n_clouds; ++i) {
        MQR_REQUIRE(counts[i] > 0 && points[i], "cloud " + std::to_string(i) + " is empty");
        MQR_REQUIRE(counts[i] < ((int64_t)1 << 31) / 3, "cloud too large");
    }
    MQR_CHECK_HIP(hipSetDevice(device));
    mqr_cloudset* cs = new mqr_cloudset();
    cs->device = device;
    int rc = 0;
    auto fail = [&](int code) {
        mqr_cloudset_destroy(cs);
        return code;
    };
    if (hipStreamCreateWithFlags(&cs->s, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&cs->d_flag, sizeof(int)) != hipSuccess) {
        set_error("registration: stream or flag allocation failed");
        return fail(1);
    }
    if (loc == MQR_DEVICE && order_after_caller(device, cs->s)) return fail(2);
    if (hipMemsetAsync(cs->d_flag, 0, sizeof(int), cs->s) != hipSuccess) {
        set_error("registration: memset failed");
        return fail(1);
    }
    for (int i = 0; i < n_clouds && !rc; ++i) {
        const float* p = points[i];
        if (loc == MQR_HOST) {
            void* d = nullptr;
            if (hipMalloc(&d, sizeof(float) * 3 * (size_t)counts[i]) != hipSuccess) {
                set_error("registration: device allocation failed");
                rc = 1;
                break;
            }
            cs->owned.push_back(d);
            if (copy_to_device(device, d, points[i], sizeof(float) * 3 * (size_t)counts[i], cs->s)) {
                rc = 1;
                break;
            }
            p = static_cast<const float*>(d);
        }
        cs->pts.push_back(p);
        cs->counts.push_back(counts[i]);
        hipLaunchKernelGGL(k_check_finite, dim3(std::min(nb(3 * counts[i]), 4096u)), dim3(256), 0, cs->s, p,
                           3 * counts[i], kCoordLimit, cs->d_flag);
    }
    if (rc) return fail(rc);
    int flag = 0;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&flag, cs->d_flag, sizeof(int), hipMemcpyDeviceToHost, cs->s) != hipSuccess ||
        hipStreamSynchronize(cs->s) != hipSuccess) {
        set_error("registration: the coordinate check failed to run");
        return fail(1);
    }
    if (flag) {
        set_error("registration: a cloud holds a non-finite coordinate");
        return fail(2);
    }
    *out = cs;
    return 0;
}

int mqr_cloudset_destroy(mqr_cloudset* cs) {
    if (!cs) return 0;
    (void)hipSetDevice(cs->device);
    if (cs->s) (void)hipStreamSynchronize(cs->s);
    for (auto& kv : cs->sels)
        if (kv.second.owned) (void)hipFree(kv.second.owned);
    for (auto& kv : cs->grids) {
        (void)hipFree(kv.second.keys);
        (void)hipFree(kv.second.order);
        (void)hipFree(kv.second.pts);
    }
    for (void* p : cs->owned) (void)hipFree(p);
    for (GrowBuf& b : cs->scratch)
        if (b.p) (void)hipFree(b.p);
    if (cs->d_flag) (void)hipFree(cs->d_flag);
    if (cs->s) (void)hipStreamDestroy(cs->s);
    delete cs;
    return 0;
}

int mqr_cloudset_voxel_down(mqr_cloudset* cs, int cloud, double voxel_size, int64_t* n, float* out, int loc) {
    MQR_REQUIRE(cs && n, "null argument");
    MQR_REQUIRE(cloud >= 0 && cloud < (int)cs->counts.size(), "cloud index out of range");
    MQR_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "voxel_size must be positive");
    MQR_CHECK_HIP(hipSetDevice(cs->device));
    if (order_after_caller(cs->device, cs->s)) return 2;
    const Selection* sel = nullptr;
    if (int rc = get_selection(cs, cloud, kVoxel, voxel_size, &sel)) return rc;
    *n = sel->n;
    if (!out) return 0;
    const size_t bytes = sizeof(float) * 3 * (size_t)sel->n;
    if (loc == MQR_DEVICE) {
        MQR_CHECK_HIP(hipMemcpyAsync(out, sel->pts, bytes, hipMemcpyDeviceToDevice, cs->s));
        MQR_CHECK_HIP(hipStreamSynchronize(cs->s));
        return 0;
    }
    return copy_to_host(cs->device, out, sel->pts, bytes, cs->s);
}

int mqr_evaluate_pairs(mqr_cloudset* cs, int n_pairs, const int32_t* src, const int32_t* tgt, int every_k,
                       double max_dist, const double* T, double* fitness, double* rmse, int64_t* ncorr) {
    if (int rc = check_pairs(cs, n_pairs, src, tgt)) return rc;
    MQR_REQUIRE(T && fitness && rmse && ncorr, "null argument");
    MQR_REQUIRE(max_dist > 0.0 && std::isfinite(max_dist), "max_dist must be positive");
    MQR_CHECK_HIP(hipSetDevice(cs->device));
    if (order_after_caller(cs->device, cs->s)) return 2;
    Batch b;
    if (int rc = make_batch(cs, n_pairs, src, tgt, kEveryK, (double)every_k, max_dist, kIcpSums, &b)) return rc;
    if (int rc = upload_state(cs, n_pairs, T, &b.d_state)) return rc;
    hipLaunchKernelGGL(k_corr<0>, dim3(b.max_blk, n_pairs), dim3(kThreads), 0, cs->s, b.d_desc, b.d_state, max_dist,
                       b.d_slabs);
    hipLaunchKernelGGL(k_finalize, dim3(n_pairs), dim3(64), 0, cs->s, b.d_desc, b.d_state, b.d_slabs, 0, 0.0, 0.0);
    MQR_CHECK_HIP(hipGetLastError());
    std::vector<PairState> h;
    if (download_state(cs, n_pairs, b.d_state, &h)) return 1;
    for (int p = 0; p < n_pairs; ++p) {
        fitness[p] = h[(size_t)p].fit;
        rmse[p] = h[(size_t)p].rmse;
        ncorr[p] = (int64_t)h[(size_t)p].count;
    }
    return 0;
}

int mqr_icp_pairs(mqr_cloudset* cs, int n_pairs, const int32_t* src, const int32_t* tgt, int n_levels,
                  const double* voxel_sizes, const double* max_dists, const int32_t* max_iters,
                  const double* rel_fitness, const double* rel_rmse, const double* T_init, double* T_out,
                  double* fitness, double* rmse, int32_t* iterations) {
    if (int rc = check_pairs(cs, n_pairs, src, tgt)) return rc;
    MQR_REQUIRE(voxel_sizes && max_dists && max_iters && rel_fitness && rel_rmse && T_init && T_out && fitness &&
                    rmse && iterations,
                "null argument");
    MQR_REQUIRE(n_levels >= 1 && n_levels <= 16, "n_levels must be in [1, 16]");
    for (int l = 0; l < n_levels; ++l) {
        MQR_REQUIRE(max_dists[l] > 0.0 && std::isfinite(max_dists[l]), "max_dists must be positive");
        MQR_REQUIRE(max_iters[l] >= 1 && max_iters[l] <= 10000, "max_iters must be in [1, 10000]");
        MQR_REQUIRE(std::isfinite(voxel_sizes[l]), "non-finite voxel size");
    }
    MQR_CHECK_HIP(hipSetDevice(cs->device));
    if (order_after_caller(cs->device, cs->s)) return 2;
    PairState* d_state = nullptr;
    if (int rc = upload_state(cs, n_pairs, T_init, &d_state)) return rc;
    std::vector<PairState> h;
    for (int l = 0; l < n_levels; ++l) {
        Batch b;
        if (int rc = make_batch(cs, n_pairs, src, tgt, kVoxel, voxel_sizes[l], max_dists[l], kIcpSums, &b)) return rc;
        hipLaunchKernelGGL(k_level_init, dim3(nb(n_pairs)), dim3(256), 0, cs->s, d_state, n_pairs);
        for (int it = 0; it < max_iters[l]; ++it) {
            hipLaunchKernelGGL(k_corr<0>, dim3(b.max_blk, n_pairs), dim3(kThreads), 0, cs->s, b.d_desc, d_state,
                               max_dists[l], b.d_slabs);
            hipLaunchKernelGGL(k_finalize, dim3(n_pairs), dim3(64), 0, cs->s, b.d_desc, d_state, b.d_slabs, 1,
                               rel_fitness[l], rel_rmse[l]);
        }
        MQR_CHECK_HIP(hipGetLastError());
        if (download_state(cs, n_pairs, d_state, &h)) return 1;  // the one host read of the level
        for (int p = 0; p < n_pairs; ++p) iterations[(size_t)p * n_levels + l] = h[(size_t)p].iters;
    }
    for (int p = 0; p < n_pairs; ++p) {
        const PairState& s = h[(size_t)p];
        for (int a = 0; a < 12; ++a) T_out[16 * (size_t)p + a] = s.T[a];
        T_out[16 * (size_t)p + 12] = T_out[16 * (size_t)p + 13] = T_out[16 * (size_t)p + 14] = 0.0;
        T_out[16 * (size_t)p + 15] = 1.0;
        fitness[p] = s.fit;
        rmse[p] = s.rmse;
    }
    return 0;
}

int mqr_information_pairs(mqr_cloudset* cs, int n_pairs, const int32_t* src, const int32_t* tgt, double max_dist,
                          const double* T, double* info) {
    if (int rc = check_pairs(cs, n_pairs, src, tgt)) return rc;
    MQR_REQUIRE(T && info, "null argument");
    MQR_REQUIRE(max_dist > 0.0 && std::isfinite(max_dist), "max_dist must be positive");
    MQR_CHECK_HIP(hipSetDevice(cs->device));
    if (order_after_caller(cs->device, cs->s)) return 2;
    Batch b;
    if (int rc = make_batch(cs, n_pairs, src, tgt, kFull, 0.0, max_dist, kInfoSums, &b)) return rc;
    if (int rc = upload_state(cs, n_pairs, T, &b.d_state)) return rc;
    double* d_info = static_cast<double*>(cs->get_scratch(3, sizeof(double) * 36 * (size_t)n_pairs));
    MQR_REQUIRE(d_info, "registration: device allocation failed");
    hipLaunchKernelGGL(k_corr<1>, dim3(b.max_blk, n_pairs), dim3(kThreads), 0, cs->s, b.d_desc, b.d_state, max_dist,
                       b.d_slabs);
    hipLaunchKernelGGL(k_finalize_info, dim3(n_pairs), dim3(64), 0, cs->s, b.d_desc, b.d_slabs, d_info);
    MQR_CHECK_HIP(hipGetLastError());
    MQR_CHECK_HIP(hipMemcpyAsync(info, d_info, sizeof(double) * 36 * (size_t)n_pairs, hipMemcpyDeviceToHost, cs->s));
    MQR_CHECK_HIP(hipStreamSynchronize(cs->s));
    return 0;
}

}  // extern "C"
