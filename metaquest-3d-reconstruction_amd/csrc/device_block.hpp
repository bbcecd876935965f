// device_block.hpp -- the library's device memory helpers (csrc/devmem.hip): per-call device staging from the
// process's device-block cache (geom_block_alloc / geom_block_release): one block of a ScratchLayout's size
// (scratch_layout.hpp), its pieces bound into it, returned to the cache at scope exit, instead of a hipMalloc /
// hipFree pair per array per call (hipFree synchronises the device; fresh allocations map pages).  The owner
// synchronises its stream before the scope ends.  Also the grow-only buffer every module keeps between calls
// (GrowBuf), the per-device stream table (StreamTable) and the carve of a geometry result (geom_alloc).
#pragma once

#include <algorithm>
#include <cstddef>
#include <mutex>

#include "mqr_common.hpp"
#include "scratch_layout.hpp"

namespace mqr {

constexpr int kMaxDevices = 64;  // size of every per-device table (the index is checked against it)

struct CachedBlock {
    int device;
    void* p = nullptr;
    size_t cap = 0;
    // p == nullptr when the layout is invalid or the device is out of memory: the one check of a call site
    CachedBlock(int d, const ScratchLayout& L) : device(d) {
        if (L.valid()) p = geom_block_alloc(d, std::max<size_t>(L.total(), 256), &cap);
        if (p) L.bind(p);
    }
    ~CachedBlock() { geom_block_release(device, p, cap); }
    CachedBlock(const CachedBlock&) = delete;
    CachedBlock& operator=(const CachedBlock&) = delete;
};

// The owner's side of that contract: declared after the block (so destroyed before it), it drains the stream
// on every exit of the call before the block goes back to the cache.
struct StreamDrain {
    hipStream_t s;
    ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// Grow-only device buffer, kept between calls by its owner (which also frees it, if ever).  A buffer is
// regrown through hipFree, which waits for the device, so work a failed call left queued has finished with
// it: regrowing under queued work is safe.
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;
    // cap >= need on success.  A regrow frees the old buffer and allocates max(need, alloc_bytes) (the
    // caller's growth rule); when that fails the sticky HIP error is cleared and p = nullptr, cap = 0.
    hipError_t reserve(size_t need, size_t alloc_bytes);
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// One non-blocking stream per device, created on first use and kept (creating a stream costs ~2 ms).  Each
// module keeps a table of its own, so modules run beside each other.  get(): nullptr for a device outside
// the table, or when the stream cannot be created (the sticky error is cleared).
struct StreamTable {
    std::mutex mu;
    hipStream_t s[kMaxDevices] = {};
    hipStream_t get(int device) {
        std::lock_guard<std::mutex> lk(mu);
        if (device < 0 || device >= kMaxDevices) return nullptr;
        if (!s[device] && hipStreamCreateWithFlags(&s[device], hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            s[device] = nullptr;
        }
        return s[device];
    }
};

// One cached block for the positions, normals and triangles of a geometry result, recycled across results
// (geom_block_alloc; mqr_geom_free returns it), with a colour array behind them when asked for.  Non-zero with
// the error set when the device is out of memory.
int geom_alloc(mqr_geom* g, int64_t nv, int64_t nt, bool colors = false);

// A scratch request that did not arrive: clears the sticky HIP error, sets "<who>: device allocation failed
// (needed N bytes)", returns 1.
int scratch_failed(const char* who, size_t bytes);

}  // namespace mqr
