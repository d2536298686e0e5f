// Failure paths of jslpsolver_amd/csrc/jslp_host_mem.h on a host WITHOUT a GPU, where every HIP allocation is refused: built with the
// host sanitizers and run as a process of its own by tests/test_host_mem.py.  Includes that header and nothing else of the project.
//   hipcc -std=c++17 -Xarch_host -fsanitize=address,undefined -o host_mem_check tests/host_mem_check.cpp && ./host_mem_check
#include "../jslpsolver_amd/csrc/jslp_host_mem.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

static int g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        g_checks++;                                                                  \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// memory sources of the test's own: the heap, refusing on request; `live` counts what is allocated and not yet released
static int g_live = 0, g_heap_fail = 0, g_late_fail = 0;
struct HeapMem {
    static hipError_t alloc(void** p, size_t n, unsigned) {
        if (g_heap_fail) return hipErrorOutOfMemory;
        *p = malloc(n); g_live++;
        return hipSuccess;
    }
    static hipError_t release(void* p) { free(p); g_live--; return hipSuccess; }
};
struct LateMem {  // the second half of a pair
    static hipError_t alloc(void** p, size_t n, unsigned flags) { return g_late_fail ? hipErrorOutOfMemory : HeapMem::alloc(p, n, flags); }
    static hipError_t release(void* p) { return HeapMem::release(p); }
};
using HeapBuf = Buf<HeapMem>;
using HeapPair = Pair<HeapBuf, Buf<LateMem>>;

template <class B> static void reserve_fails_and_leaves_nothing() {
    B b;
    CHECK(b.reserve(4096) != hipSuccess);
    CHECK(b.p == nullptr && b.bytes == 0);
    CHECK(b.reserve(4096) != hipSuccess);  // ... and again the same way
    CHECK(b.p == nullptr && b.bytes == 0);
    CHECK(b.reserve(0) == hipSuccess && b.p == nullptr);  // nothing asked for: nothing to refuse
    B c(std::move(b));
    b = std::move(c);
    CHECK(b.p == nullptr && c.p == nullptr);
}

// the restated table of counts: a static arena (snapshot, flags, trace) of a 40 x 30 tableau, row capacity 60, ld 32
struct Piece { size_t size, count; };
static const Piece PIECES[] = {{1, 152}, {1, 152}, {8, 60 * 32}, {8, 60}, {8, 60 * 30}, {4, 60}, {4, 30}, {4, 152}, {4, 152}, {8, 1u << 20}, {8, 1}, {4, 1}, {1, 3}, {16, 5}};
static const int N_PIECES = (int)(sizeof PIECES / sizeof PIECES[0]);
struct Carved { char* p[N_PIECES]; };
static void layout(Carved& out, Carver& cv) {
    for (int i = 0; i < N_PIECES; i++) out.p[i] = cv.take<char>(PIECES[i].size * PIECES[i].count);
}

int main() {
    // 1. no device: every allocation of the two product sources is refused, and a refused reserve leaves nothing behind
    reserve_fails_and_leaves_nothing<DevBuf>();
    reserve_fails_and_leaves_nothing<PinBuf>();
    {
        PinBuf b;
        CHECK(b.reserve(64, hipHostMallocPortable) != hipSuccess && b.p == nullptr && b.bytes == 0);
    }
    // a buffer that had memory and cannot grow is EMPTY afterwards, not its old self with a new size
    {
        HeapBuf b;
        CHECK(b.reserve(100) == hipSuccess && b.p && b.bytes == 100 && g_live == 1);
        char* const first = b.p;
        CHECK(b.reserve(50) == hipSuccess && b.p == first && b.bytes == 100);  // grows only
        g_heap_fail = 1;
        CHECK(b.reserve(200) != hipSuccess && b.p == nullptr && b.bytes == 0 && g_live == 0);
        CHECK(b.reserve(200) != hipSuccess && b.p == nullptr && b.bytes == 0);
        g_heap_fail = 0;
        CHECK(b.reserve(200) == hipSuccess && b.bytes == 200 && g_live == 1);
    }
    CHECK(g_live == 0);
    // 2. the pair: the old pair stays usable until both new halves exist
    {
        StagePair s;  // the product's: its FIRST half is refused here
        bool pinned = true;
        CHECK(s.reserve(4096, &pinned) != hipSuccess && !pinned && s.bytes() == 0 && !s.d.p && !s.h.p);
        CHECK(s.reserve(4096) != hipSuccess && s.bytes() == 0);
        HeapPair p;
        CHECK(p.reserve(100) == hipSuccess && p.bytes() == 100 && g_live == 2);
        char *const d0 = p.d.p, *const h0 = p.h.p;
        d0[99] = 1; h0[99] = 2;
        g_late_fail = 1;  // the second half fails: the first new half is released, the old pair is untouched
        pinned = false;
        CHECK(p.reserve(1000, &pinned) != hipSuccess && pinned);
        CHECK(p.d.p == d0 && p.h.p == h0 && p.bytes() == 100 && g_live == 2 && d0[99] == 1 && h0[99] == 2);
        g_late_fail = 0; g_heap_fail = 1;  // the first half fails
        CHECK(p.reserve(1000, &pinned) != hipSuccess && !pinned && p.d.p == d0 && p.h.p == h0 && g_live == 2);
        g_heap_fail = 0;
        CHECK(p.reserve(1000) == hipSuccess && p.bytes() == 1000 && g_live == 2);  // both exist: the old pair is gone
        HeapPair q(std::move(p));
        CHECK(p.bytes() == 0 && !p.d.p && !p.h.p && q.bytes() == 1000);
    }
    CHECK(g_live == 0);
    // 3. the carve helper: sizing and carving agree, every piece on a 256-byte boundary; a refused reservation leaves no pointer behind
    {
        Carved sized, carved;
        Carver sizing{nullptr, 0};
        layout(sized, sizing);
        for (int i = 0; i < N_PIECES; i++) CHECK(sized.p[i] == nullptr);
        CHECK(carve_bytes([&](Carver& cv) { layout(sized, cv); }) == sizing.off + 256);
        HeapBuf arena;
        CHECK(carve_into(arena, [&](Carver& cv) { layout(carved, cv); }) == hipSuccess);
        CHECK(arena.bytes == sizing.off + 256);
        size_t off = 0;  // the offsets restated: each piece at the next multiple of 256 behind the one before
        for (int i = 0; i < N_PIECES; i++) {
            off = (off + 255) / 256 * 256;
            CHECK((size_t)(carved.p[i] - arena.p) == off && off % 256 == 0);
            off += PIECES[i].size * PIECES[i].count;
        }
        CHECK(off == sizing.off && off + 256 <= arena.bytes);
        carved.p[N_PIECES - 1][PIECES[N_PIECES - 1].size * PIECES[N_PIECES - 1].count - 1] = 7;  // the last byte is inside (the sanitizer looks)
        char* const before = arena.p;
        CHECK(carve_into(arena, [&](Carver& cv) { layout(carved, cv); }) == hipSuccess && arena.p == before && carved.p[0] == before);  // large enough: carved again in place
        DevBuf none;  // refused: the layout has only run its sizing pass
        CHECK(carve_into(none, [&](Carver& cv) { layout(carved, cv); }) != hipSuccess);
        for (int i = 0; i < N_PIECES; i++) CHECK(carved.p[i] == nullptr);
        CHECK(none.p == nullptr && none.bytes == 0);
    }
    CHECK(g_live == 0);
    // 4. bundles: empty, refused half way, moved from, parked in a vector, taken out again, destroyed
    {
        PooledRes a;
        CHECK(!a.complete());
        CHECK(hipStreamCreateWithFlags(&a.stream.h, hipStreamNonBlocking) != hipSuccess && !a.stream);  // no device: no stream either
        CHECK(hipEventCreate(&a.ev_begin.h) != hipSuccess && !a.ev_begin);
        CHECK(a.h_state.reserve(192) != hipSuccess && a.up.reserve(1 << 20) != hipSuccess && a.static_arena.reserve(1 << 20) != hipSuccess);
        CHECK(!a.complete());
        a.device = 3;
        std::vector<PooledRes> shelf;
        shelf.push_back(std::move(a));
        shelf.push_back(PooledRes());
        for (int i = 0; i < 6; i++) shelf.emplace_back();  // (reallocation moves the parked ones)
        CHECK(shelf[0].device == 3 && !shelf[0].stream && !a.stream && !a.h_state.p);
        PooledRes taken;
        taken = std::move(shelf[0]);
        shelf.erase(shelf.begin());
        CHECK(taken.device == 3 && shelf.size() == 7);
        a = std::move(taken);   // into a moved-from bundle
        a = PooledRes();        // released in place
        taken = std::move(a);   // from an empty one into a moved-from one
        std::vector<PooledRes> drop;
        drop.swap(shelf);
        for (auto& r : drop) r = PooledRes();
        Stream s1, s2(std::move(s1));
        s1 = std::move(s2);
        Event e1, e2(std::move(e1));
        e2.reset();
        CHECK(!s1 && !s2 && !e1 && !e2);
    }
    printf("host_mem_check ok: %d checks\n", g_checks);
    return 0;
}
