// scratch_layout.hpp -- how one device block is cut into arrays, stated once.  A piece is one statement:
//     uint64_t* keys;   L.add(keys, m);                        float* d_col;   L.add(d_col, 3 * nv, host_in && colors);
// (the pointer's type is the element type).  The layout sums the wanted pieces, each rounded up to 256 bytes,
// into total(): that is the request.  bind(base) then points every wanted piece into the block, in the order
// declared; an unwanted piece is nullptr and takes nothing; a wanted piece of count 0 still takes one slot, so
// its pointer is non-null and aliases nothing.  A negative count, a size past size_t or more than kMaxPieces
// pieces make the layout invalid (total() == 0); the owner reports that with its one allocation check.  The
// pointer variables must outlive the bind.  Pure size arithmetic: no HIP, so a host compiler builds it alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mqr {

inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

class ScratchLayout {
public:
    static constexpr int kMaxPieces = 32;

    template <class T>
    void add(T*& p, int64_t count, bool want = true) {
        p = nullptr;
        put(&p, [](void* var, char* at) { *static_cast<T**>(var) = reinterpret_cast<T*>(at); }, count, sizeof(T), want);
    }
    // several pieces of one count, in the order given
    template <class... T>
    void add_each(int64_t count, T*&... p) {
        (add(p, count), ...);
    }
    // an untyped piece (hipcub temporary storage)
    void add_bytes(void*& p, size_t bytes, bool want = true) {
        p = nullptr;
        put(&p, [](void* var, char* at) { *static_cast<void**>(var) = at; },
            bytes > size_t(INT64_MAX) ? -1 : (int64_t)bytes, 1, want);
    }

    bool valid() const { return ok_; }
    size_t total() const { return ok_ ? total_ : 0; }
    // every wanted piece -> its place in the block at `base` (which holds total() bytes)
    void bind(void* base) const {
        for (int i = 0; ok_ && i < n_; ++i) piece_[i].set(piece_[i].var, static_cast<char*>(base) + piece_[i].off);
    }

private:
    struct Piece {
        void* var;
        void (*set)(void*, char*);
        size_t off;
    };
    void put(void* var, void (*set)(void*, char*), int64_t count, size_t elem, bool want) {
        if (!want || !ok_) return;
        const size_t room = SIZE_MAX - 255 - total_;
        if (count < 0 || n_ == kMaxPieces || (uint64_t)count > room / elem) {
            ok_ = false;
            return;
        }
        piece_[n_++] = Piece{var, set, total_};
        total_ += count ? al256(elem * (size_t)count) : 256;
    }
    Piece piece_[kMaxPieces];
    int n_ = 0;
    size_t total_ = 0;
    bool ok_ = true;
};

}  // namespace mqr
