// The properties of csrc/scratch_layout.hpp, checked by a stand-alone host program (tests/test_scratch_layout.py
// builds it with the address and undefined-behaviour sanitizers and runs it): exits non-zero on the first
// property that does not hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>
#include <vector>

#include "scratch_layout.hpp"

using mqr::ScratchLayout;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

static size_t slot(size_t bytes) { return bytes ? (bytes + 255) / 256 * 256 : 256; }

template <int N>
struct Elem {
    unsigned char b[N];
};

struct Want {
    int elem;
    int64_t count;
    bool want;
};

// a pointer variable of any element type: created in place by add_one, read back as bytes
struct Var {
    alignas(void*) unsigned char raw[sizeof(void*)];
    char* get() const {
        char* p;
        std::memcpy(&p, raw, sizeof p);
        return p;
    }
};

// one piece of element size N
template <int N>
static void add_one(ScratchLayout& L, Var& var, int64_t count, bool want) {
    Elem<N>** p = new (var.raw) Elem<N>*(reinterpret_cast<Elem<N>*>(var.raw));  // (non-null before the add)
    L.add(*p, count, want);
}
using Adder = void (*)(ScratchLayout&, Var&, int64_t, bool);
static const Adder kAdd[16] = {add_one<1>,  add_one<2>,  add_one<3>,  add_one<4>, add_one<5>,  add_one<6>,
                               add_one<7>,  add_one<8>,  add_one<9>,  add_one<10>, add_one<11>, add_one<12>,
                               add_one<13>, add_one<14>, add_one<15>, add_one<16>};

// the properties of one piece list: builds the layout, binds it to a malloc'd base of exactly total() bytes
// and writes every byte of every piece
static void check_list(const std::vector<Want>& w) {
    ScratchLayout L;
    std::vector<Var> vars(w.size());
    size_t sum = 0;
    for (size_t i = 0; i < w.size(); ++i) {
        const size_t before = L.total();
        kAdd[w[i].elem - 1](L, vars[i], w[i].count, w[i].want);
        const size_t bytes = (size_t)w[i].elem * (size_t)w[i].count;
        CHECK(L.total() - before == (w[i].want ? slot(bytes) : 0));  // an unwanted piece adds nothing,
        if (w[i].want) sum += slot(bytes);                            // a wanted empty one exactly 256 bytes
    }
    CHECK(L.valid());
    CHECK(L.total() == sum);
    char* base = static_cast<char*>(std::malloc(sum ? sum : 1));
    CHECK(base);
    L.bind(base);
    size_t end_prev = 0;
    for (size_t i = 0; i < w.size(); ++i) {
        char* p = vars[i].get();
        if (!w[i].want) {
            CHECK(p == nullptr);
            continue;
        }
        CHECK(p != nullptr);
        const size_t off = (size_t)(p - base), bytes = (size_t)w[i].elem * (size_t)w[i].count;
        CHECK(off % 256 == 0);
        CHECK(off >= end_prev);  // pieces come in the order declared, so this is pairwise disjointness
        end_prev = off + slot(bytes);
        CHECK(end_prev <= L.total());
        std::memset(p, 0xa5, bytes);               // every byte of the piece ...
        if (!bytes) std::memset(p, 0x5a, 256);  // ... and the whole slot of an empty one
    }
    CHECK(end_prev == L.total());  // the last piece ends at the total
    std::free(base);
}

int main() {
    // fixed cases: optional pieces, empty pieces between neighbours, an empty layout
    check_list({});
    check_list({{4, 10, true}, {8, 0, true}, {1, 300, true}});
    check_list({{4, 10, true}, {8, 77, false}, {1, 300, true}, {2, 0, false}, {16, 1, true}});
    check_list({{1, 0, true}, {1, 0, true}, {1, 0, true}});
    check_list({{3, 256, true}, {1, 256, true}, {1, 257, true}});
    {  // the pointer of a wanted empty piece is its own: not its neighbours'
        ScratchLayout L;
        int32_t *a, *b, *c;
        L.add(a, 5);
        L.add(b, 0);
        L.add(c, 5);
        CHECK(L.valid() && L.total() == 3 * 256);
        std::vector<char> base(L.total());
        L.bind(base.data());
        CHECK(a && b && c && (char*)b == (char*)a + 256 && (char*)c == (char*)b + 256);
    }
    {  // several pieces of one count in one statement: the same as one add each, in the order given
        ScratchLayout L;
        float *a, *b;
        uint8_t* c;
        L.add_each(65, a, b, c);
        CHECK(L.valid() && L.total() == 512 + 512 + 256);
        std::vector<char> base(L.total());
        L.bind(base.data());
        CHECK((char*)a == base.data() && (char*)b == base.data() + 512 && (char*)c == base.data() + 1024);
    }
    {  // untyped pieces
        ScratchLayout L;
        void *t, *u;
        L.add_bytes(t, 1000);
        L.add_bytes(u, 5, false);
        CHECK(L.valid() && L.total() == 1024 && u == nullptr);
        std::vector<char> base(L.total());
        L.bind(base.data());
        CHECK(t == base.data());
        std::memset(t, 1, 1000);
    }
    {  // a negative count, and a byte size past size_t, invalidate the layout (and it stays invalid)
        ScratchLayout L;
        double* d;
        float* f;
        L.add(f, 4);
        CHECK(L.valid());
        L.add(d, -1);
        CHECK(!L.valid() && L.total() == 0);
        L.add(f, 4);
        CHECK(!L.valid());
        ScratchLayout M;
        L = M;
        L.add(d, INT64_MAX / 4);  // 8 x count > SIZE_MAX
        CHECK(!L.valid());
        ScratchLayout N2;
        Elem<16>* e;
        N2.add(f, 4);
        N2.add(e, INT64_MAX / 8 - 1);  // fits on its own, not behind the rounding and the first piece
        CHECK(!N2.valid());
        ScratchLayout U;  // an unwanted piece is not looked at
        U.add(d, -1, false);
        CHECK(U.valid() && U.total() == 0 && d == nullptr);
    }
    {  // more pieces than the layout holds: invalid, not an overrun
        ScratchLayout L;
        char* p[ScratchLayout::kMaxPieces + 1];
        for (auto& q : p) L.add(q, 1);
        CHECK(!L.valid());
    }
    std::mt19937_64 rng(20240611);
    for (int iter = 0; iter < 4000; ++iter) {
        std::vector<Want> w((size_t)(rng() % (ScratchLayout::kMaxPieces + 1)));
        for (Want& x : w) x = Want{(int)(rng() % 16) + 1, (int64_t)(rng() % 70001), rng() % 3 != 0};
        check_list(w);
    }
    std::puts("scratch layout ok");
    return 0;
}
