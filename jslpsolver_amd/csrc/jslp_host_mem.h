// jslp_host_mem.h -- host-only owners of what the engine allocates: device and pinned buffers, the device + pinned staging pair,
// streams and events (all move-only, freed by their destructors), and the Carver that lays several arrays out in one allocation.
// At its end PooledRes, the bundle of these an engine holds and the resource pool parks.  It needs the HIP runtime API only -- no kernel
// header, nothing of jslp_hip.hip --, so tests/host_mem_check.cpp compiles it alone and walks its failure paths.
#pragma once
#include <hip/hip_runtime_api.h>

#include <stddef.h>

#include <utility>

// a runtime handle with one destroy call (a stream, an event); converts to the handle so that the API calls take it as before
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.release()) {}
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) { reset(); h = o.release(); }
        return *this;
    }
    ~Handle() { reset(); }
    H release() { H t = h; h = nullptr; return t; }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

// where a Buf's memory comes from.  The product instantiates these two and no other; the parameter exists for tests/host_mem_check.cpp,
// whose sources of its own fail on request (on a host without a GPU these two can only fail)
struct DeviceMem {
    static hipError_t alloc(void** p, size_t n, unsigned) { return hipMalloc(p, n); }
    static hipError_t release(void* p) { return hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t n, unsigned flags) { return hipHostMalloc(p, n, flags); }
    static hipError_t release(void* p) { return hipHostFree(p); }
};
// one allocation and its byte count
template <class M>
struct Buf {
    char* p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~Buf() { reset(); }
    void reset() {
        if (p) (void)M::release(p);
        p = nullptr; bytes = 0;
    }
    // grows only (the old content is NOT kept); on failure the buffer is empty: never a stale pointer with a stale size
    hipError_t reserve(size_t n, unsigned flags = 0) {  // (flags: hipHostMalloc's, pinned memory only)
        if (n <= bytes) return hipSuccess;
        reset();
        void* q = nullptr;
        const hipError_t err = M::alloc(&q, n, flags);
        if (err != hipSuccess || !q) return err != hipSuccess ? err : hipErrorOutOfMemory;
        p = static_cast<char*>(q); bytes = n;
        return hipSuccess;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
using DevBuf = Buf<DeviceMem>;
using PinBuf = Buf<PinnedMem>;

// a staging buffer: a device allocation and its pinned twin of the same size
template <class D, class H>
struct Pair {
    D d;
    H h;
    size_t bytes() const { return d.bytes < h.bytes ? d.bytes : h.bytes; }
    // grows only; both new halves first, and the old pair stays usable until both exist (*pinned_failed: which half the error is about).
    // The caller makes sure nothing in flight still uses the old pair
    hipError_t reserve(size_t n, bool* pinned_failed = nullptr) {
        if (n <= bytes()) return hipSuccess;
        D nd;
        H nh;
        if (pinned_failed) *pinned_failed = false;
        if (const hipError_t err = nd.reserve(n); err != hipSuccess) return err;
        if (pinned_failed) *pinned_failed = true;
        if (const hipError_t err = nh.reserve(n); err != hipSuccess) return err;
        d = std::move(nd); h = std::move(nh);
        return hipSuccess;
    }
};
using StagePair = Pair<DevBuf, PinBuf>;

struct Carver {  // hands out 256-byte aligned pieces of one allocation; a sizing pass (base == nullptr) hands out nullptr and just adds up
    char* base;
    size_t off;
    template <class T>
    T* take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += sizeof(T) * count;
        return p;
    }
};
// bytes an arena needs for `layout` (a function of a Carver& that take()s every piece): the sizing pass, + 256 of slack
template <class F>
size_t carve_bytes(F&& layout) {
    Carver sizing{nullptr, 0};
    layout(sizing);
    return sizing.off + 256;
}
// size it, grow `arena` to that, carve it.  When the reservation fails only the sizing pass has run: every pointer `layout` sets is
// nullptr and the arena is empty, so a caller's "already set up" test reads false
template <class B, class F>
hipError_t carve_into(B& arena, F&& layout) {
    const hipError_t err = arena.reserve(carve_bytes(layout));
    if (err != hipSuccess) return err;
    Carver cv{arena.p, 0};
    layout(cv);
    return hipSuccess;
}

// ---- the bundle the resource pool keeps -----------------------------------------------------------------------------
// A Solve() of a small model creates and destroys an engine; stream / event / pinned-memory creation and the device
// arenas cost ~4 ms per engine on this stack -- more than every pivot of the reference's fixtures.  What is worth keeping is ONE
// bundle: the engine holds it as `res`, a destroyed engine parks it in the resource pool of jslp_hip.hip (a handful of entries,
// arenas up to 1 GiB each) and the next create() on the same device moves it in, re-carving the arenas when they are large enough.
struct PooledRes {
    int device = 0;
    Stream stream;
    Event ev_begin, ev_end;
    PinBuf h_state;                 // DevState | completion flag and its neighbours (64 bytes): the flag's sequence travels with it
    DevBuf static_arena;            // snapshot, flags, pivot trace
    DevBuf slot_arena;              // the tableau copies; a taker keeps it as its spare until ensure_slots(1) has run
    DevBuf r_arena;                 // the resident kernel's hand-off buffers + backup
    StagePair cuts, out, up;        // staging of the cut lists, the read-back, the upload
    Stream copy_stream; Event ev_group;  // read-back of a finished group of nodes while the next group computes (created on first use)
    bool complete() const { return stream && ev_begin && ev_end && h_state.p && static_arena.p && slot_arena.p; }  // worth parking
};
