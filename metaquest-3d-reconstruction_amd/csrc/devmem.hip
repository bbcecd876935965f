// devmem.hip -- device memory and host <-> device copies shared by every module (device_block.hpp,
// mqr_common.hpp): the grow-only buffer, the process's device-block cache, the geometry result handle and
// the copy path with its pinned download ring.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "device_block.hpp"
#include "mqr_common.hpp"

namespace mqr {

hipError_t GrowBuf::reserve(size_t need, size_t alloc_bytes) {
    if (cap >= need) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = std::max(need, alloc_bytes);
    const hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        return e;
    }
    cap = want;
    return hipSuccess;
}

int scratch_failed(const char* who, size_t bytes) {
    (void)hipGetLastError();
    set_error(std::string(who) + ": device allocation failed (needed " + std::to_string(bytes) + " bytes)");
    return 1;
}

static std::mutex g_geom_mu;
static std::vector<std::tuple<int, void*, size_t>> g_geom_cache;  // (device, block, capacity)
constexpr size_t kGeomCacheBlocks = 4;

void* geom_block_alloc(int device, size_t bytes, size_t* cap) {
    {
        std::lock_guard<std::mutex> lk(g_geom_mu);
        int best = -1;
        for (size_t i = 0; i < g_geom_cache.size(); ++i) {
            const auto& e = g_geom_cache[i];
            if (std::get<0>(e) == device && std::get<2>(e) >= bytes &&
                (best < 0 || std::get<2>(e) < std::get<2>(g_geom_cache[best])))
                best = (int)i;
        }
        if (best >= 0) {
            void* p = std::get<1>(g_geom_cache[best]);
            *cap = std::get<2>(g_geom_cache[best]);
            g_geom_cache.erase(g_geom_cache.begin() + best);
            return p;
        }
    }
    const size_t want = (bytes + (size_t(1) << 20) - 1) & ~((size_t(1) << 20) - 1);
    void* p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) return nullptr;
    *cap = want;
    return p;
}

void geom_block_release(int device, void* p, size_t cap) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_geom_mu);
        if (cap && g_geom_cache.size() < kGeomCacheBlocks) {
            g_geom_cache.emplace_back(device, p, cap);
            return;
        }
    }
    (void)hipFree(p);
}

int geom_alloc(mqr_geom* g, int64_t nv, int64_t nt, bool colors) {
    const size_t sv = al256(sizeof(float) * 3 * std::max<int64_t>(nv, 1));
    const size_t st = al256(sizeof(int32_t) * 3 * std::max<int64_t>(nt, 1));
    g->blk = geom_block_alloc(g->device, (colors ? 3 : 2) * sv + st, &g->blk_cap);
    MQR_REQUIRE(g->blk, "geometry: device allocation failed");
    char* p = static_cast<char*>(g->blk);
    g->pos = reinterpret_cast<float*>(p);
    g->nrm = reinterpret_cast<float*>(p + sv);
    g->tri = reinterpret_cast<int32_t*>(p + 2 * sv);
    g->col = colors ? reinterpret_cast<float*>(p + 2 * sv + st) : nullptr;
    return 0;
}

// Device -> pageable host copies of large results (mqr_geom_copy, mqr_memcpy).  hipMemcpy into pageable
// memory stages through the runtime's pinned buffers on the calling thread: ~10 GB/s for the 1 GB C5 mesh
// (BENCH_r04 c5.extract_ms 102.9 ms).  Here a copy kernel moves the range chunk by chunk into a ring of
// pinned slots (GPU stores over the fabric: 54.7 GB/s into pinned memory, SDMA 57.1, tools/d2h_modes.hip)
// on a stream the process already runs, and kD2HThreads host threads copy each slot out as its event
// completes (first-touching the destination pages in parallel).  Round 5's first version gave every host
// thread its own stream and DMA: the same ~41 GB/s once set up, but its set-up cost the process's first
// large copy 46.6 ms (first 48 MB copy, vs 1.6 ms for the second, tools/d2h_probe.py) -- four stream
// creations 50 ms and the copy engine's first use 16-19 ms on an MI355X box (tools/d2h_setup_probe.hip,
// profiles/r05_d2h_setup_probe.json).  The ring (one pinned allocation per device) is kept and the calls
// are serialised by a mutex: one large copy at a time per process.
constexpr int kD2HThreads = 8;  // 1 GiB into a fresh array: 44.4 GB/s with 4, 51.1 with 8 (profiles/r05_d2h_probe.jsonl)
constexpr int kD2HSlots = 8;
constexpr size_t kD2HChunk = size_t(8) << 20;
struct D2HRing {
    char* buf = nullptr;
    hipEvent_t ev[kD2HSlots] = {};
};
static std::mutex g_d2h_mu;
static D2HRing g_d2h[kMaxDevices];

__global__ __launch_bounds__(256) void k_copy_out16(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_copy_out1(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

hipStream_t copy_stream(int device) {
    if (caller_stream()) {
        hipDevice_t sd = -1;
        const bool same = hipStreamGetDevice(caller_stream(), &sd) == hipSuccess && sd == device;
        (void)hipGetLastError();
        if (same) return caller_stream();
    }
    return nullptr;
}

static void launch_copy(char* to, const char* from, size_t len, hipStream_t s) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(to) | reinterpret_cast<uintptr_t>(from)) & 15) == 0;
    const size_t n16 = aligned ? len / 16 : 0, tail = len - 16 * n16;
    if (n16) k_copy_out16<<<1024, 256, 0, s>>>(reinterpret_cast<uint4*>(to), reinterpret_cast<const uint4*>(from), n16);
    if (tail)
        k_copy_out1<<<(unsigned)std::min<size_t>(1024, (tail + 255) / 256), 256, 0, s>>>(
            reinterpret_cast<uint8_t*>(to) + 16 * n16, reinterpret_cast<const uint8_t*>(from) + 16 * n16, tail);
}

// One ring transfer: the GPU fills slot k % S with chunk k, host thread k % T copies it out once its
// event completes; this thread queues the GPU copies in chunk order, each into a slot whose previous
// chunk has been copied out.
static int ring_copy(int device, char* dst, const char* src, size_t bytes, hipStream_t s) {
    MQR_REQUIRE(device >= 0 && device < kMaxDevices, "device index out of range");
    std::lock_guard<std::mutex> lk(g_d2h_mu);
    D2HRing& r = g_d2h[device];
    if (!r.buf) {
        MQR_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&r.buf), kD2HSlots * kD2HChunk, hipHostMallocDefault));
        for (auto& e : r.ev) MQR_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const size_t nchunks = (bytes + kD2HChunk - 1) / kD2HChunk;
    // MQR_D2H_THREADS (1..8): another thread count, for tools/d2h_probe.py
    static const int env_threads =
        getenv("MQR_D2H_THREADS") ? std::max(1, std::min(8, atoi(getenv("MQR_D2H_THREADS")))) : kD2HThreads;
    const int T = (int)std::min<size_t>(env_threads, nchunks);
    auto len_of = [&](size_t k) { return std::min(kD2HChunk, bytes - k * kD2HChunk); };
    std::atomic<int64_t> issued{0};            // chunks whose GPU copy and event are queued
    std::atomic<int64_t> host_done[kD2HSlots];  // the last chunk copied out of each slot
    for (auto& d : host_done) d.store(-1);
    std::atomic<int> failed{0};
    std::vector<std::string> errs(T + 1);
    auto host_side = [&](int t) {
        for (size_t k = (size_t)t; k < nchunks; k += (size_t)T) {
            while (issued.load(std::memory_order_acquire) <= (int64_t)k && !failed.load()) std::this_thread::yield();
            if (failed.load()) return;
            const int slot = (int)(k % kD2HSlots);
            hipError_t e = hipEventSynchronize(r.ev[slot]);
            if (e != hipSuccess) {
                errs[t] = std::string("host copy: hipEventSynchronize: ") + hipGetErrorString(e);
                failed.store(1);
                return;
            }
            std::memcpy(dst + k * kD2HChunk, r.buf + slot * kD2HChunk, len_of(k));
            host_done[slot].store((int64_t)k, std::memory_order_release);
        }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(host_side, t);
    for (size_t k = 0; k < nchunks && !failed.load(); ++k) {
        const int slot = (int)(k % kD2HSlots);
        if (k >= (size_t)kD2HSlots)
            while (host_done[slot].load(std::memory_order_acquire) != (int64_t)(k - kD2HSlots) && !failed.load())
                std::this_thread::yield();
        if (failed.load()) break;
        launch_copy(r.buf + slot * kD2HChunk, src + k * kD2HChunk, len_of(k), s);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(r.ev[slot], s);
        if (e != hipSuccess) {
            errs[T] = std::string("host copy: chunk copy launch: ") + hipGetErrorString(e);
            failed.store(1);
            break;
        }
        issued.store((int64_t)k + 1, std::memory_order_release);
    }
    for (auto& x : th) x.join();
    if (failed.load()) {
        (void)hipStreamSynchronize(s);  // no slot write left in flight for the next call
        for (auto& m : errs)
            if (!m.empty()) {
                set_error(m);
                return 1;
            }
    }
    return 0;
}

int d2h_parallel(int device, void* dst, const void* src, size_t bytes) {
    return copy_to_host(device, dst, src, bytes, copy_stream(device));
}

// page-locked host memory (hipHostMalloc / hipHostRegister, e.g. torch's pin_memory()): the DMA engine
// reads or writes it directly, no staging
static bool host_pinned(const void* p) {
    hipPointerAttribute_t a{};
    const bool pinned = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    return pinned;
}

int copy_to_host(int device, void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes >= kD2HParallelMin && !host_pinned(dst)) return ring_copy(device, static_cast<char*>(dst), static_cast<const char*>(src), bytes, s);
    if (bytes) {
        MQR_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        MQR_CHECK_HIP(hipStreamSynchronize(s));
    }
    return 0;
}

// uploads: HIP's own pageable path already runs at the link's rate from present pages (1 GiB: 55.8 GB/s,
// against 44.1 through a ring like the one above, profiles/r05_d2h_probe.jsonl)
int copy_to_device(int device, void* dst, const void* src, size_t bytes, hipStream_t s) {
    (void)device;
    if (bytes) {
        MQR_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        MQR_CHECK_HIP(hipStreamSynchronize(s));
    }
    return 0;
}

static int geom_copy_one(int device, void* dst, const void* src, size_t bytes, hipMemcpyKind k) {
    if (k == hipMemcpyDeviceToHost && bytes >= kD2HParallelMin) return d2h_parallel(device, dst, src, bytes);
    MQR_CHECK_HIP(hipMemcpy(dst, src, bytes, k));
    return 0;
}
}  // namespace mqr

using namespace mqr;

extern "C" {

int mqr_geom_counts(mqr_geom* g, int64_t* nv, int64_t* nt) {
    MQR_REQUIRE(g, "null geometry");
    if (nv) *nv = g->nv;
    if (nt) *nt = g->nt;
    return 0;
}

int mqr_geom_copy(mqr_geom* g, float* positions, float* normals, int32_t* triangles, int loc) {
    MQR_REQUIRE(g, "null geometry");
    MQR_CHECK_HIP(hipSetDevice(g->device));
    const hipMemcpyKind k = loc == MQR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    // hipMemcpy orders after the null stream only: the caller's stream may still use the buffers
    if (loc == MQR_DEVICE && caller_stream()) MQR_CHECK_HIP(hipStreamSynchronize(caller_stream()));
    if (positions && g->nv && geom_copy_one(g->device, positions, g->pos, sizeof(float) * 3 * g->nv, k)) return 1;
    if (normals && g->nv && geom_copy_one(g->device, normals, g->nrm, sizeof(float) * 3 * g->nv, k)) return 1;
    if (triangles && g->nt && geom_copy_one(g->device, triangles, g->tri, sizeof(int32_t) * 3 * g->nt, k)) return 1;
    return 0;
}

int mqr_geom_device_ptrs(mqr_geom* g, void** positions, void** normals, void** triangles) {
    MQR_REQUIRE(g, "null geometry");
    if (positions) *positions = g->nv ? g->pos : nullptr;
    if (normals) *normals = g->nv ? g->nrm : nullptr;
    if (triangles) *triangles = g->nt ? g->tri : nullptr;
    return 0;
}

int mqr_geom_device_colors(mqr_geom* g, void** colors) {
    MQR_REQUIRE(g && colors, "null argument");
    *colors = g->nv ? g->col : nullptr;
    return 0;
}

int mqr_geom_copy_colors(mqr_geom* g, float* colors, int loc) {
    MQR_REQUIRE(g && colors, "null argument");
    MQR_REQUIRE(g->col, "geometry: the result has no colours");
    MQR_CHECK_HIP(hipSetDevice(g->device));
    const hipMemcpyKind k = loc == MQR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (loc == MQR_DEVICE && caller_stream()) MQR_CHECK_HIP(hipStreamSynchronize(caller_stream()));
    if (g->nv && geom_copy_one(g->device, colors, g->col, sizeof(float) * 3 * g->nv, k)) return 1;
    return 0;
}

int mqr_geom_free(mqr_geom* g) {
    if (!g) return 0;
    (void)hipSetDevice(g->device);
    if (g->blk) {
        // the block may still be read by work queued on a stream (a device-side copy): drain first
        (void)hipDeviceSynchronize();
        geom_block_release(g->device, g->blk, g->blk_cap);
    } else {
        if (g->pos) (void)hipFree(g->pos);
        if (g->nrm) (void)hipFree(g->nrm);
        if (g->tri) (void)hipFree(g->tri);
    }
    delete g;
    return 0;
}

}  // extern "C"
