// jslp_hip.hip -- host side of the MI355X engine: the C ABI of include/jslp_engine.h over the kernels in
// jslp_kernels.hip.h.  Build (see __graft_entry__.build):
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared -o libjslp_hip.so jslp_hip.hip
//
// Launch strategy (DESIGN.md "Kernels"):
//   * large tableau  -> per pivot one k_select (1 workgroup) + one k_update (whole chip) on the engine's
//     stream; pivots are enqueued in chunks and the 128-byte device state is polled once per chunk, so the
//     GPU never waits for the host inside a chunk.  Kernels launched after the solve ended exit at once.
//   * small tableau / batch of branch-and-bound nodes -> k_simplex_wg: one workgroup runs the whole
//     simplex() of one tableau copy ("slot"); a batch is one launch with grid = #nodes.
// (see xl_fits below: the XCD-local kernels live in the test library; defined up here because jslp_engine_create reads it first)
#if (defined(JSLP_CHAOS_BUILD) || defined(JSLP_DEV_XL_ONLY)) && !defined(JSLP_WITH_XL)
#define JSLP_WITH_XL 1
#endif
#include "../../include/jslp_engine.h"
#include "../../include/jslpx_branch.h"
#include "../../include/jslpm_many.h"
#include "../../include/jslpf_f32.h"
#include "../../include/jslpr_mir.h"
#include "../../include/jslpp_packed.h"
#include "../../include/jslpt_tree.h"
#include "../../include/jslps_soft.h"
#include "../../include/jslpc_tree_mir.h"
#include "../../include/jslpe_tree_enhanced.h"
#include "../../include/jslpi_tree_incremental.h"
#include "../../include/jslpg_tree_tolerance.h"
#include "../../include/jslpb_big_lds.h"
#include "jslp_kernels.hip.h"
#include "jslp_host_mem.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

static thread_local char g_err[512];
static int fail(int code, const char* fmt, const char* a = "", const char* b = "") {
    snprintf(g_err, sizeof g_err, fmt, a, b);
    return code;
}
#define HIPC(expr)                                                                              \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) return fail(JSLP_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
// carve_into(arena, layout) with the error text of an allocation: the arena's name, not the layout's code
#define HIPC_CARVE(arena, ...)                                                                                    \
    do {                                                                                                          \
        hipError_t _e = carve_into(arena, __VA_ARGS__);                                                           \
        if (_e != hipSuccess) return fail(JSLP_ERR_DEVICE, "%s: %s", "carve_into(" #arena ")", hipGetErrorString(_e)); \
    } while (0)
#define JSLP_TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)  // (an engine call's own error code travels up unchanged)

static const size_t WGLDS_MAX_BYTES = 64 * 1024;  // largest dynamic LDS the LDS-resident one-workgroup kernels are launched with
struct jslp_engine {
    int device = 0;
    PooledRes res;
    int32_t H0 = 0, W = 0, ld = 0, cap_rows = 0, n_idx = 0;
    double precision = 1e-8;
    int32_t batch = 50, use_partial = 0;
    int uploaded = 0, has_save = 0;
    int slot0_synced = 0;  // slot 0 = current snapshot except for its dirty rows (st.gen == st.s_gen): k_node_wg may be used
    int slots_synced = 0;  // slots 1 .. slots_synced-1 are in that state too (only slot 0 ever leaves it on its own)
    double evaluation = 0;
    // slots (slot 0 = the live tableau).  All per-slot arrays live in ONE device allocation (res.slot_arena), the
    // snapshot / flags / trace in another (res.static_arena): an allocation and its release cost ~0.1 ms apiece, and a Solve of a
    // small model creates and destroys an engine
    int n_slots = 0;
    Slots s{};
    DevBuf spare_slot_arena;  // the slot arena of the bundle the resource pool handed over at create()
    // snapshot
    double* snap_A = nullptr; double* snap_rhs = nullptr;
    double* snap_AT = nullptr; int snap_ldT = 0;  // the saved root transposed (tableaus the LDS node kernels take; else nullptr)
    int32_t *snap_vibr = nullptr, *snap_vibc = nullptr, *snap_rbv = nullptr, *snap_cbv = nullptr;
    uint8_t* d_unr = nullptr;
    uint8_t* d_isint = nullptr;  // variable.isInteger per variable index (MIR cuts)
    int has_int = 0;             // jslp_engine_set_integer_variables registered at least one since the last upload
    StagePair mir_rec;           // jslpr_engine_relax_mir: one MirRec per node (device / pinned), or the 8 bytes of k_fractional_volume
    int32_t n_opt = 0; double* snap_oo = nullptr;  // optional objectives (slot copies live in s.oo)
    DevBuf oo_mem, snap_oo_mem;                      // ... what s.oo and snap_oo point into (resize_optional_objectives)
    // cuts staging (res.cuts): ONE pinned host buffer -> ONE device buffer per call: [value | offs | var | type]
    int32_t* d_cut_offs = nullptr; int8_t* d_cut_type = nullptr; int32_t* d_cut_var = nullptr; double* d_cut_val = nullptr;
    int32_t* d_cut_order = nullptr; int* d_queue = nullptr;  // batch hand-out order (most cuts first) + queue counter, uploaded with the cuts
    std::vector<int32_t> order_scratch;
    bool queue_wgs_opt = false; int node_queue_launches = 0; long long resident_fetch_retries = 0;  // (which build the count below is for; batches that went through k_node_queue)
    int queue_wgs = 0; size_t queue_wgs_lds = 0;             // resident workgroups of k_node_queue<512> for this LDS size
    // read-back staging (res.out): ONE device buffer -> ONE pinned buffer per group: [states | rhs | rows]
    double* d_rhs = nullptr; int32_t* d_rows = nullptr; DevState* d_states = nullptr;
    double* h_rhs = nullptr; int32_t* h_rows = nullptr; DevState* h_states = nullptr;
    DevState* h_state = nullptr;  // res.h_state: pinned, 1 entry, followed by the completion flag of the one-launch node kernel
    unsigned done_seq = 0;
    // upload staging (res.up, pinned half): [matrix, row stride W | vibr | vibc | unrestricted list]; the matrix part is what
    // jslp_engine_host_matrix hands to the host to build the tableau in; the device half = twin of the blob
    // (and of the matrix when it needs the W -> ld repack)
    int host_matrix_out = 0;  // the host holds a pointer into res.up.h
    // compact read-back (jslp_engine_relax_watched)
    DevBuf d_watch; int32_t n_watch = 0;
    // work counters
    int counting = 0;
    DevBuf d_cnt;
    jslp_work_counters wc{};
    // snapshot generation as the device pool sees it: bumped by save() and upload()
    unsigned long long root_seq = 0;
    // safety net of the register-resident kernel: copy of slot 0 taken before the cooperative launch
    DevState* r_backup_st = nullptr;  // (hand-off buffers + this backup: res.r_arena, ONE allocation)
    double* rb_A = nullptr; int32_t *rb_vibr = nullptr, *rb_vibc = nullptr, *rb_rbv = nullptr, *rb_cbv = nullptr;
    int* d_done_count = nullptr;  // workgroups of a small batch that have delivered their outcome (k_node_lds: the last one raises the completion flag)
    unsigned long long* d_nnz = nullptr; long long nnz = -1;  // non-zero cells of the uploaded tableau (counted on the device)
    unsigned spin_limit = 0; int test_abort_epoch = -1; int test_late_wave0 = 0;
    int test_iters_cap = 0;  // tests only (JSLP_TEST_ITERS_CAP): a lower iteration cap, 0 = none
    int resident_fallbacks = 0;  // solves that were rolled back and re-run through the streaming kernels
    int resident_handovers = 0;  // solves the lean resident kernel handed to the general one (cycle-check history beyond its LDS copy)
    int resident_launches = 0;   // cooperative launches of k_simplex_resident the runtime accepted
    int resident_refusals = 0;   // ... it refused (or that no build exists for): the solve went through the streaming kernels
    std::vector<jslp_simplex_result> rec_results;  // per-node results of a branch-record call (the record is what the caller gets)
    StagePair rec;  // branch records of a batch (device / pinned)
    double dev_prev_evaluation = 0.0;  // jslp_engine_relax_batch_device: the evaluation its nodes started from (results_from_states)
    int dev_prev_valid = 0;
    // checkpoints (incremental-branch-and-cut.ts:31-44): equally sized device buffers, recycled through a free list
    struct Ckpt {
        DevBuf mem;
        double* A = nullptr; double* rhs = nullptr;
        int32_t *vibr = nullptr, *vibc = nullptr, *rbv = nullptr, *cbv = nullptr;
        int32_t H = 0, last_element_index = 0;
        double evaluation = 0;
        int live = 0;
    };
    std::vector<Ckpt> ckpts;
    std::vector<DevBuf> ck_free;
    // fp32 twin of slot 0 (jslp_engine_simplex_f32), allocated on first use
    f32::Slots s32{};
    DevBuf arena32;
    int32_t n32 = 0;  // tableau copies the arena holds (ensure_f32)
    // policy
    int force_path = 0;  // 0 auto, 1 workgroup kernel, 2 select+update kernels only, 3 fused phase 2
    int force_xl = 0, xl_on = 0;  // JSLP_FORCE_PATH=xl / JSLP_XL=0: the XCD-local register-resident geometry (resident_geometry 6)
    int force_resident = 0;  // JSLP_FORCE_PATH=resident: also the register-resident geometries the default policy leaves to the streaming kernels
    int32_t n_unr = 0;
    int nt = 0;  // JSLP_NT=1: non-temporal hints in the fused kernel
    // fused phase-2 pipeline (ping-pong buffer + per-workgroup candidates)
    DevBuf f_buf1, f_cands[2], f_pcol[2], f_st[2];
    DevBuf f_uflags;  // fused pipeline with unrestricted variables: 2 x (column flags | row flags)
    int f_ready = 0;  // every buffer above exists and is zeroed (ensure_fused)
    DevBuf f_oo1; int f_oo1_rows = 0;  // fused pipeline: the optional objectives' second (ping-pong) buffer
    long long p1_slow_pivots = 0;  // pivots the fused phase 1 handed to k_select + k_update (tiny pivot-row entries, see k_fused_p1)
    // register-resident phase 2 (one cooperative launch): hand-off buffers
    u64_t* r_gran = nullptr;  // [2][G][8] granules then [2][G] row flags (one allocation, zeroed per launch)
    int32_t max_uploaded_idx = -1;  // largest variable index in the row / column maps of the last upload()
    int abort_injected = 0;  // JSLP_INJECT_RESIDENT_ABORT_US fired in this simplex() already
    unsigned* h_abort_ptr = nullptr;  // pinned word the lean resident kernels look at every 1024 pivots (host-requested abort)
    size_t r_slot_doubles = 0;  // doubles per candidate-row slot the arena was carved for
    u64_t* r_rows[2] = {nullptr, nullptr}; unsigned* r_sync = nullptr; int2* r_hist_all = nullptr; int r_want_hist = 0; Ctx* r_ctx_dev = nullptr;
    int no_resident = 0;
    int res_cpt = 2;  // columns per lane of the resident kernel (JSLP_RES_CPT=2|4)
    int one_launch_nodes = 1;  // JSLP_NO_NODE_KERNEL=1: single children go through the five-launch sequence
    int use_wglds = 1;         // JSLP_NO_WGLDS=1: the generic one-workgroup kernels (global-memory selection state) only
    const char* last_path = "none";
    // timing
    int timing = 0;
    double upd_ms = 0, total_ms = 0;
    long long upd_launches = 0;
    std::vector<Event> ev_pool;
};

static const long long WG_CELLS_SINGLE = 64 * 1024;         // one workgroup beats 2 launches/pivot below this
static const long long WG_CELLS_BATCH = 4LL * 1024 * 1024;  // batches use one workgroup per node up to this
// The pack of small LPs (include/jslpp_packed.h): an LP of at most this many cells (height x width) is solved by the one-wave build of
// k_simplex_packed, a larger one by the 256-thread build.  A pivot's row update is cells / threads turns of a lane plus, in the 256-thread
// build only, six workgroup barriers and three cross-wave reductions through LDS; one wave pays neither and leaves the CU's other
// wave slots to other LPs.  At 2048 cells a lane's share of the update is 32 cells, about what those barriers and reductions cost, and
// every fuzz root (<= 1260 cells) and every fixture but the few hundred-column ones stays on one wave.  Set from that reasoning and the
// timing table (profiles/packed_lp_times.md), not from a sweep.
static const long long PACK_CELLS_WAVE = 2048;
#ifndef JSLP_SMALL_BATCH_1024_DEFAULT
#define JSLP_SMALL_BATCH_1024_DEFAULT 256  // batches of at most this many nodes (one per CU) take the 1024-thread node kernel: 16 nodes 111 -> 102 us, 64 nodes 147 -> 132 us (r03_o); 0 = never
#endif
// ---- tuning knobs of the node path ------------------------------------------------------------------------------------
// Every knob below is LATCHED: read from the environment at its first use and kept for the life of the process (the tests give each setting a
// process of its own).  JSLP_DEBUG_LAUNCH is the one switch the node path reads on every call: tests turn it on and off inside one process.
struct Knob { bool set; long long v; };  // set: the variable exists at all
static Knob read_knob(const char* name, long long dflt) { const char* t = getenv(name); return Knob{t != nullptr, t ? atoll(t) : dflt}; }
#define KNOB(type, fn, name, dflt) static type fn() { static const type v = (type)read_knob(name, dflt).v; return v; }
// workgroup size of the per-node kernel when a call carries several nodes (tools/relax_batch_scaling.py); measured on Monster_II node batches (tools/wg_shape_sweep.sh): 512 > 1024 > 256
KNOB(int, wg_batch_threads_raw, "JSLP_WG_BATCH_THREADS", 512)
static int wg_batch_threads() { const int v = wg_batch_threads_raw(); return v == 256 || v == 1024 ? v : 512; }
// nodes per group of a batch (= tableau copies alive at once); whether it was given at all decides what the queue's grid defaults to (plan_node_call)
static Knob group_max_knob() { static const Knob k = read_knob("JSLP_GROUP_MAX", 1024); return k; }
static int group_max() { const long long v = group_max_knob().v; return v < 1 ? 1024 : (int)v; }
KNOB(int, zero_copy, "JSLP_ZERO_COPY", 1)  // batch outcomes written by the kernels straight into the pinned read-back buffer (no copy stream)
KNOB(int, snapshot_transpose_on, "JSLP_SNAPSHOT_TRANSPOSE", 1)  // pivot-column reads of untouched rows from the transposed root
KNOB(int, node_cow_single, "JSLP_NODE_COW_SINGLE", 1)  // single-node call: copy-on-write start (0: restore eagerly, as the batch groups do)
KNOB(int, node_cow, "JSLP_NODE_COW", 1)  // queue kernel: copy-on-write slots (no restore between nodes)
// (round 6) copy-on-write start in the small batch too, as the queue kernel and the single-node call have it: a node READS what its slot's earlier nodes
// dirtied from the root instead of restoring those rows first -- the eager restore was 8.6 k of the 78 k cycles of a node of an 8-node batch
// (tools/wglds_timing.py one 8, debug build), in front of everything else; JSLP_NODE_COW_SMALL=0: eager restores
KNOB(int, node_cow_small, "JSLP_NODE_COW_SMALL", 1)
// a batch that leaves most CUs idle anyway (speculative batches of a real tree: <= 16 nodes) is served by latency, not by occupancy: the 1024-thread shape of the single-node path, one workgroup per CU
KNOB(int, small_batch_1024, "JSLP_SMALL_BATCH_1024", JSLP_SMALL_BATCH_1024_DEFAULT)
// a batch in one launch of resident workgroups pulling nodes from a queue: 0 = one launch per group, 1 = the queue hands the nodes out in call order, 2 (default since round 6) = most cuts first.
// The cut count predicts a node's repair pivots, and 2416 nodes on 768 resident workgroups are 3.15 rounds: longest-first keeps the last
// workgroups to finish on the cheap nodes.  Round 2 measured it SLOWER (2.73 M/s against 2.94 M in call order: a node then cost ~3x what it
// costs now and the order array's extra trip per node showed); re-measured on round 6's kernels, same session, compact read-back,
// tools/wglds_timing.py: 4.94-5.06 M relaxations/s against 4.14-4.41 M in call order (+14 %); outcome digests identical (tools/queue_check.py)
KNOB(int, node_queue, "JSLP_NODE_QUEUE", 2)
// 1 hands the FULL read-back out longest-first too; its bound is the PCIe link and it measured 3.41-3.42 M against 3.52-3.54 M relaxations/s in call order: the heavy nodes' outcomes then leave in one burst
KNOB(int, node_queue_order_full, "JSLP_NODE_QUEUE_ORDER_FULL", 0)
KNOB(long long, wg_cells_child, "JSLP_WG_CELLS_CHILD", 1536LL * 1024)  // a single B&B child (few repair pivots) stays in one workgroup up to this (tools/child_path_times.py)
// the solve path's two latched knobs
KNOB(int, fused_wide_on, "JSLP_FUSED_WIDE", 1)  // 0: tableaus wider than 4096 columns through k_select + k_update, as before round 5
KNOB(int, fused_p1_on, "JSLP_FUSED_P1", 1)  // 0: phase 1 of the large LPs through k_select + k_update instead of k_fused_p1 (one launch per pivot)
#undef KNOB
// ... and the switches simplex() reads on EVERY call, one reader each (tests flip them inside one process); JSLP_RES_GEOM / JSLP_RES_RPB (experiments) and
// JSLP_INJECT_RESIDENT_ABORT_US are read where they act
static bool res_lean_on() { const char* t = getenv("JSLP_RES_LEAN"); return !(t && atoi(t) == 0); }  // 0: the general build of the register-resident kernel only
static int res_wide_tall() { const char* t = getenv("JSLP_RES_WIDE_TALL"); return t ? atoi(t) : -1; }  // -1: not given (resident_geometry)
static bool debug_launch_on() { return getenv("JSLP_DEBUG_LAUNCH") != nullptr; }
// a one-group batch of the 1024-thread node kernel ends by polling its completion flag (JSLP_BATCH_POLL=0: stream synchronisation; the first character decides)
static int batch_poll_on() { static const int v = [] { const char* t = getenv("JSLP_BATCH_POLL"); return (t && t[0] == '0') ? 0 : 1; }(); return v; }
// JSLP_DEBUG_STALL=<ms> (diagnosis): a dependent batch normally takes ~70 us; say on stderr when one took longer than that many milliseconds and where the time went (report_stall)
static double debug_stall_ms() { static const double v = [] { const char* t = getenv("JSLP_DEBUG_STALL"); return t ? atof(t) : 0.0; }(); return v; }
static const size_t HIST_CAP_MAIN = 1u << 20;
static const size_t HIST_CAP_SLOT = 1u << 16;
static const long long TRACE_CAP = 1LL << 20;

extern "C" const char* jslp_backend_name(void) { return "hip-gfx950"; }
extern "C" const char* jslp_last_error(void) { return g_err; }
extern "C" int jslp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int32_t round_up(int32_t x, int32_t m) { return (x + m - 1) / m * m; }
static dim3 copy_grid(const jslp_engine* e, int slots);

// ---- the resource pool's shelf (PooledRes: jslp_host_mem.h) --------------------------------------------------------------
// (both shelves are never destroyed: a static destructor would call into a runtime that may be gone at exit; jslp_release_pooled_resources empties them)
static std::mutex g_pool_mu;
static std::vector<PooledRes>& g_pool = *new std::vector<PooledRes>();
static const size_t POOL_MAX_ENTRIES = 4;
static const size_t POOL_MAX_ARENA = (size_t)1 << 30;

static bool pool_enabled() {
    static int v = -1;
    if (v < 0) { const char* t = getenv("JSLP_NO_POOL"); v = (t && t[0] == '1') ? 0 : 1; }
    return v == 1;
}
static bool pool_take(int device, PooledRes* out) {
    if (!pool_enabled()) return false;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); i++)
        if (g_pool[i].device == device) {
            *out = std::move(g_pool[i]);
            g_pool.erase(g_pool.begin() + (long)i);
            return true;
        }
    return false;
}
static bool pool_give(PooledRes&& r) {  // (refused: `r` is left as it was and dies with its owner)
    if (!pool_enabled() || r.static_arena.bytes > POOL_MAX_ARENA || r.slot_arena.bytes > POOL_MAX_ARENA || r.out.bytes() > POOL_MAX_ARENA / 4 ||
        r.up.bytes() > POOL_MAX_ARENA / 4 || r.r_arena.bytes > POOL_MAX_ARENA)
        return false;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_pool.size() >= POOL_MAX_ENTRIES) return false;
    g_pool.push_back(std::move(r));
    return true;
}

static void release_many_resources();
extern "C" void jslp_release_pooled_resources(void) {
    release_many_resources();  // (the jslpm_simplex_many buffers)
    std::vector<PooledRes> drop;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        drop.swap(g_pool);
    }
    for (auto& r : drop) {
        hipSetDevice(r.device);
        r = PooledRes();
    }
}

static void carve_slots(Slots& s, Carver& cv, int n) {
    s.A = cv.take<double>((size_t)s.A_stride * n);
    s.vibr = cv.take<int32_t>((size_t)s.vibr_stride * n);
    s.vibc = cv.take<int32_t>((size_t)s.vibc_stride * n);
    s.rbv = cv.take<int32_t>((size_t)s.idx_stride * n);
    s.cbv = cv.take<int32_t>((size_t)s.idx_stride * n);
    s.prow = cv.take<double>((size_t)s.prow_stride * n);
    s.pcol = cv.take<double>((size_t)s.pcol_stride * n);
    s.dirty = cv.take<uint8_t>((size_t)s.pcol_stride * n);
    s.rhs = cv.take<double>((size_t)s.pcol_stride * n);
    s.st = cv.take<DevState>((size_t)n);
    s.hist = cv.take<int2>((size_t)s.hist_cap * n);
}

// the fallible half of ensure_slots: `arena` (empty, or the spare) and `oo` carved / allocated for n slots, zeroed, the live tableau carried over
static int fill_slots(jslp_engine* e, int n, const Slots& o, Slots& s, DevBuf& arena, DevBuf& oo) {
    hipStream_t st = e->res.stream;
    HIPC_CARVE(arena, [&](Carver& cv) { carve_slots(s, cv, n); });
    // slot 0's matrix is zero-filled by upload(); other slots are filled by their first (full) restore
    HIPC(hipMemsetAsync(s.dirty, 0, (size_t)s.pcol_stride * n, st));
    HIPC(hipMemsetAsync(s.st, 0, sizeof(DevState) * n, st));  // gen = 0: slots hold no snapshot copy yet
    s.n_opt = e->n_opt;
    s.oo_stride = (long long)e->n_opt * e->ld;
    s.oo = nullptr;
    if (e->n_opt > 0) {
        HIPC(oo.reserve(sizeof(double) * (size_t)s.oo_stride * n));
        s.oo = oo.as<double>();
        HIPC(hipMemsetAsync(s.oo, 0, sizeof(double) * (size_t)s.oo_stride * n, st));
    }
    if (e->n_slots == 0) return JSLP_OK;
    // carry the live tableau over
    HIPC(hipMemcpyAsync(s.A, o.A, sizeof(double) * o.A_stride, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(s.vibr, o.vibr, sizeof(int32_t) * o.vibr_stride, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(s.vibc, o.vibc, sizeof(int32_t) * o.vibc_stride, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(s.rbv, o.rbv, sizeof(int32_t) * o.idx_stride, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(s.cbv, o.cbv, sizeof(int32_t) * o.idx_stride, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(s.st, o.st, sizeof(DevState), hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(s.dirty, o.dirty, (size_t)o.pcol_stride, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(s.rhs, o.rhs, sizeof(double) * (size_t)o.pcol_stride, hipMemcpyDeviceToDevice, st));
    if (e->n_opt > 0 && o.oo) HIPC(hipMemcpyAsync(s.oo, o.oo, sizeof(double) * (size_t)o.oo_stride, hipMemcpyDeviceToDevice, st));
    HIPC(hipStreamSynchronize(st));
    return JSLP_OK;
}
// (re)allocate the slot arrays for n slots, preserving slot 0; on failure the engine keeps what it had, its spare arena included
static int ensure_slots(jslp_engine* e, int n) {
    if (n <= e->n_slots) return JSLP_OK;
    Slots s = e->s;
    s.A_stride = (long long)e->cap_rows * e->ld;
    s.vibr_stride = e->cap_rows;
    s.vibc_stride = e->W;
    s.idx_stride = e->n_idx;
    s.prow_stride = e->ld;
    s.pcol_stride = e->cap_rows;
    s.hist_cap = n == 1 ? (int32_t)HIST_CAP_MAIN : (int32_t)HIST_CAP_SLOT;
    s.ld = e->ld; s.W = e->W; s.batch = e->batch; s.use_partial = e->use_partial; s.precision = e->precision;
    s.has_unr = e->n_unr > 0 ? 1 : 0;
    s.unr = e->d_unr;
    const bool from_spare = e->spare_slot_arena.bytes >= carve_bytes([&](Carver& cv) { carve_slots(s, cv, n); });  // from the resource pool
    DevBuf arena, oo;
    if (from_spare) arena = std::move(e->spare_slot_arena);
    if (const int rc = fill_slots(e, n, e->s, s, arena, oo)) {
        if (from_spare) e->spare_slot_arena = std::move(arena);
        return rc;
    }
    e->s = s;
    e->res.slot_arena = std::move(arena);  // (the old arena and the old objective rows go: slot 0 has been carried over)
    e->oo_mem = std::move(oo);
    e->n_slots = n;
    e->slots_synced = std::min(e->slots_synced, 1);  // only slot 0 was carried over
    e->spare_slot_arena.reset();                     // too small: not needed any more
    return JSLP_OK;
}

// forget every checkpoint; their buffers go to the free list
static void drop_checkpoints(jslp_engine* e) {
    for (auto& c : e->ckpts)
        if (c.live) e->ck_free.push_back(std::move(c.mem));
    e->ckpts.clear();
}

// every getenv of create(), read per engine
static int read_engine_policy(jslp_engine* e) {
    const char* fp = getenv("JSLP_FORCE_PATH");
    if (fp && !strcmp(fp, "wg")) e->force_path = 1;
    if (fp && !strcmp(fp, "sp")) e->force_path = 2;
    if (fp && !strcmp(fp, "fused")) { e->force_path = 3; e->no_resident = 1; }
    if (fp && !strcmp(fp, "resident")) { e->force_path = 3; e->force_resident = 1; }
#ifdef JSLP_WITH_XL
    if (fp && !strcmp(fp, "xl")) { e->force_path = 3; e->force_resident = 1; e->force_xl = 1; }  // the XCD-local resident geometry whatever the size (<= 1024 x 1024)
#else
    if (fp && !strcmp(fp, "xl")) return fail(JSLP_ERR_UNSUPPORTED, "JSLP_FORCE_PATH=xl: the XCD-local kernels are compiled into the test library only (libjslp_hip_chaos.so, or build with -DJSLP_WITH_XL)");
#endif
    // JSLP_XL=1: the XCD-local geometry for every tableau it takes.  OFF by default: as measured in round 4 (profiles/r04_xl_*) it is
    // correct on every golden but not faster than what these sizes had -- 6.4-6.8 us per pivot on dense 501 x 501 / 1001 x 1001 against
    // 6.0 chip-wide, 8.6 against 6.9 (one LDS workgroup) on the sparse Monster LP: its pivot is bound by the instruction stream of
    // the 32-row unrolled loops, not by the hand-offs it shortens
    const char* xl = getenv("JSLP_XL");
    e->xl_on = (xl && xl[0] == '1') ? 1 : 0;
    const char* nr = getenv("JSLP_NO_RESIDENT");
    if (nr && nr[0] == '1') e->no_resident = 1;
    const char* rcpt = getenv("JSLP_RES_CPT");
    if (rcpt && rcpt[0] == '4') e->res_cpt = 4;
    if (rcpt && rcpt[0] == '2') e->res_cpt = 2;
    const char* nk = getenv("JSLP_NO_NODE_KERNEL");
    if (nk && nk[0] == '1') e->one_launch_nodes = 0;
    const char* nl = getenv("JSLP_NO_WGLDS");
    if (nl && nl[0] == '1') e->use_wglds = 0;
    const char* nt = getenv("JSLP_NT");
    e->nt = (nt && nt[0] == '1') ? 1 : 0;
    const char* sl = getenv("JSLP_SPIN_LIMIT");  // polls before a hand-off of the resident kernel gives up (tests shorten it)
    e->spin_limit = sl ? (unsigned)std::max(1LL, atoll(sl)) : JSLP_SPIN_LIMIT_DEFAULT;
    const char* ta = getenv("JSLP_TEST_RESIDENT_ABORT");  // tests only: abort the resident kernel's hand-off at this pivot
    e->test_abort_epoch = ta ? atoi(ta) : -1;
    const char* tl = getenv("JSLP_TEST_RESIDENT_LATE_WAVE0");  // tests only: wave 0 of every workgroup reaches each row fetch late
    e->test_late_wave0 = tl ? atoi(tl) : 0;
    const char* tc = getenv("JSLP_TEST_ITERS_CAP");  // tests only: the iteration cap (iters_cap) comes down to this many pivots per simplex call
    e->test_iters_cap = tc ? std::max(0, atoi(tc)) : 0;
    return JSLP_OK;
}
// snapshot, unrestricted flags and pivot trace: one allocation
static void carve_static(jslp_engine* e, Carver& cv) {
    e->d_unr = cv.take<uint8_t>((size_t)e->n_idx);
    e->d_isint = cv.take<uint8_t>((size_t)e->n_idx);
    e->snap_A = cv.take<double>((size_t)e->cap_rows * e->ld);
    e->snap_rhs = cv.take<double>((size_t)e->cap_rows);
    e->snap_ldT = (e->cap_rows + 1) & ~1;
    e->snap_AT = wglds_bytes(e->ld, e->cap_rows) <= WGLDS_MAX_BYTES ? cv.take<double>((size_t)e->snap_ldT * e->W) : nullptr;
    e->snap_vibr = cv.take<int32_t>((size_t)e->cap_rows);
    e->snap_vibc = cv.take<int32_t>((size_t)e->W);
    e->snap_rbv = cv.take<int32_t>((size_t)e->n_idx);
    e->snap_cbv = cv.take<int32_t>((size_t)e->n_idx);
    e->s.trace = cv.take<int2>((size_t)TRACE_CAP);
    e->d_nnz = cv.take<unsigned long long>(1);
    e->d_done_count = cv.take<int>(1);
}
// the device side of create(): a parked bundle or a new stream, the arenas, slot 0, the pinned state
static int engine_init(jslp_engine* e) {
    const bool have = pool_take(e->device, &e->res);
    e->res.device = e->device;
    if (have) e->spare_slot_arena = std::move(e->res.slot_arena);
    else HIPC(hipStreamCreateWithFlags(&e->res.stream.h, hipStreamNonBlocking));
    HIPC_CARVE(e->res.static_arena, [&](Carver& cv) { carve_static(e, cv); });
    e->s.trace_cap = TRACE_CAP;
    HIPC(hipMemsetAsync(e->d_unr, 0, e->n_idx, e->res.stream));
    HIPC(hipMemsetAsync(e->d_done_count, 0, sizeof(int), e->res.stream));
    JSLP_TRY(ensure_slots(e, 1));
    if (!have) {
        HIPC(e->res.h_state.reserve(sizeof(DevState) + 64));
        memset(e->res.h_state.p, 0, sizeof(DevState) + 64);
        HIPC(hipEventCreate(&e->res.ev_begin.h));
        HIPC(hipEventCreate(&e->res.ev_end.h));
    }
    e->h_state = e->res.h_state.as<DevState>();
    // (no synchronisation here: the two memsets above are ordered in front of everything this engine will ever enqueue -- one
    //  stream --, and a Solve() of a mid-size LP creates an engine per call)
    // the completion flag lives behind the pinned state and travels with it through the resource pool: continue the
    // previous owner's sequence (a fresh counter would meet the old owner's numbers again)
    e->done_seq = *reinterpret_cast<unsigned*>(e->res.h_state.p + sizeof(DevState));
    return JSLP_OK;
}

extern "C" int jslp_engine_create(jslp_engine** out, int device, int32_t height, int32_t width, int32_t row_capacity,
                                  double precision) {
    if (!out || height < 1 || width < 1 || row_capacity < height) return fail(JSLP_ERR_ARG, "create: bad dimensions");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(JSLP_ERR_DEVICE, "create: no HIP device visible (this engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(JSLP_ERR_ARG, "create: device ordinal out of range");
    HIPC(hipSetDevice(device));
    jslp_engine* e = new jslp_engine();
    e->device = device;
    e->H0 = height; e->W = width; e->cap_rows = row_capacity; e->precision = precision;
    e->ld = round_up(width, 16);
    e->n_idx = width + 2 * row_capacity + 2;
    // partial pricing parameters (simplex.ts:118-127)
    const int32_t n_columns = width - 1;
    int32_t b = (int32_t)floor(sqrt((double)n_columns));
    b = std::min(500, std::max(50, b));
    e->batch = b;
    e->use_partial = n_columns > b * 2;
    int rc = read_engine_policy(e);
    if (!rc) rc = engine_init(e);
    if (rc) { jslp_engine_destroy(e); return rc; }
    *out = e;
    return JSLP_OK;
}

extern "C" void jslp_engine_destroy(jslp_engine* e) {
    if (!e) return;
    hipSetDevice(e->device);
    if (e->res.stream) hipStreamSynchronize(e->res.stream);
    if (e->res.copy_stream) hipStreamSynchronize(e->res.copy_stream);
    if (e->res.complete()) pool_give(std::move(e->res));  // parked -- or it dies with everything else the engine owns
    delete e;
}

// upload staging: pinned [matrix H0 x W | vibr | vibc | unrestricted list] and its device twin
static size_t up_matrix_bytes(const jslp_engine* e) { return ((sizeof(double) * (size_t)e->H0 * e->W) + 255) & ~(size_t)255; }
static size_t up_blob_bytes(const jslp_engine* e) { return sizeof(int32_t) * ((size_t)e->H0 + e->W + e->n_idx); }
static int ensure_up(jslp_engine* e) {
    HIPC(e->res.up.reserve(up_matrix_bytes(e) + up_blob_bytes(e)));
    return JSLP_OK;
}
// the number of optional objectives changes: their rows in every slot (zeroed) and in the snapshot; nothing may be in flight.
// The counts are committed only once both buffers exist: a failed call leaves an engine without optional objectives
static int resize_optional_objectives(jslp_engine* e, int32_t n) {
    e->oo_mem.reset(); e->snap_oo_mem.reset();
    e->s.oo = nullptr; e->snap_oo = nullptr;
    e->n_opt = 0; e->s.n_opt = 0; e->s.oo_stride = 0;
    if (n == 0) return JSLP_OK;
    const size_t per = sizeof(double) * (size_t)n * e->ld, all = per * std::max(1, e->n_slots);
    HIPC(e->oo_mem.reserve(all));
    HIPC(e->snap_oo_mem.reserve(per));
    e->s.oo = e->oo_mem.as<double>(); e->snap_oo = e->snap_oo_mem.as<double>();
    e->n_opt = n; e->s.n_opt = n;
    e->s.oo_stride = (long long)n * e->ld;
    HIPC(hipMemsetAsync(e->s.oo, 0, all, e->res.stream));
    HIPC(hipStreamSynchronize(e->res.stream));
    return JSLP_OK;
}

extern "C" int jslp_engine_host_matrix(jslp_engine* e, double** matrix, int64_t* n_doubles) {
    if (!e || !matrix) return fail(JSLP_ERR_ARG, "host_matrix: null pointer");
    HIPC(hipSetDevice(e->device));
    int rc = ensure_up(e);
    if (rc) return rc;
    memset(e->res.up.h.p, 0, sizeof(double) * (size_t)e->H0 * e->W);  // a fresh Float64Array is zero-filled (tableau.ts:304)
    e->host_matrix_out = 1;
    *matrix = reinterpret_cast<double*>(e->res.up.h.p);
    if (n_doubles) *n_doubles = (int64_t)e->H0 * e->W;
    return JSLP_OK;
}

extern "C" int jslp_engine_upload(jslp_engine* e, const double* matrix, const int32_t* var_index_by_row,
                                  const int32_t* var_index_by_col, const int32_t* unrestricted_var_indexes,
                                  int32_t n_unrestricted) {
    if (!e || !matrix || !var_index_by_row || !var_index_by_col) return fail(JSLP_ERR_ARG, "upload: null pointer");
    if (n_unrestricted < 0 || (n_unrestricted > 0 && !unrestricted_var_indexes)) return fail(JSLP_ERR_ARG, "upload: bad unrestricted list");
    if (n_unrestricted > e->n_idx) return fail(JSLP_ERR_ARG, "upload: more unrestricted variables than variable indexes");
    HIPC(hipSetDevice(e->device));
    const int32_t H = e->H0, W = e->W;
    int rc = ensure_up(e);
    if (rc) return rc;
    // everything crosses PCIe from pinned memory: the matrix as ONE DMA (straight from the buffer the host built it in when
    // it used jslp_engine_host_matrix), the maps as one small blob; the inverse maps, flags and state are built on the device
    const size_t mat = sizeof(double) * (size_t)H * W, mat_pad = up_matrix_bytes(e);
    int32_t* b_vibr = reinterpret_cast<int32_t*>(e->res.up.h.p + mat_pad);
    int32_t* b_vibc = b_vibr + H;
    int32_t* b_unr = b_vibc + W;
    b_vibr[0] = -1; b_vibc[0] = -1;
    int32_t max_idx = -1;
    for (int32_t r = 1; r < H; r++) {
        const int32_t v = var_index_by_row[r];
        if (v < 0 || v >= e->n_idx) return fail(JSLP_ERR_ARG, "upload: row variable index out of range");
        b_vibr[r] = v;
        max_idx = std::max(max_idx, v);
    }
    for (int32_t c = 1; c < W; c++) {
        const int32_t v = var_index_by_col[c];
        if (v < 0 || v >= e->n_idx) return fail(JSLP_ERR_ARG, "upload: column variable index out of range");
        b_vibc[c] = v;
        max_idx = std::max(max_idx, v);
    }
    e->max_uploaded_idx = max_idx;
    for (int32_t i = 0; i < n_unrestricted; i++) {
        const int32_t v = unrestricted_var_indexes[i];
        if (v < 0 || v >= e->n_idx) return fail(JSLP_ERR_ARG, "upload: unrestricted variable index out of range");
        b_unr[i] = v;
    }
    if (matrix != reinterpret_cast<const double*>(e->res.up.h.p)) memcpy(e->res.up.h.p, matrix, mat);  // pageable caller memory: stage it once
    hipStream_t s = e->res.stream;
    const size_t blob = sizeof(int32_t) * ((size_t)H + W + (size_t)n_unrestricted);
    char* d_blob = e->res.up.d.p + mat_pad;
    if (W == e->ld) {
        HIPC(hipMemcpyAsync(e->s.A, e->res.up.h.p, mat, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(d_blob, e->res.up.h.p + mat_pad, blob, hipMemcpyHostToDevice, s));
    } else {  // one DMA for matrix + blob, then the W -> ld repack on the device (padding columns become 0)
        HIPC(hipMemcpyAsync(e->res.up.d.p, e->res.up.h.p, mat_pad + blob, hipMemcpyHostToDevice, s));
        const long long cells = (long long)H * e->ld;
        hipLaunchKernelGGL(k_repack, dim3((unsigned)std::min<long long>(2048, (cells + 255) / 256)), dim3(256), 0, s, e->s.A,
                           reinterpret_cast<const double*>(e->res.up.d.p), (int)H, (int)W, (int)e->ld);
    }
    HIPC(hipMemsetAsync(e->d_nnz, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_count_nnz, dim3(256), dim3(256), 0, s, e->s.A, (int)H, (int)e->ld, e->d_nnz);
    UploadBlob ub;
    ub.vibr = reinterpret_cast<const int32_t*>(d_blob);
    ub.vibc = ub.vibr + H;
    ub.unr = ub.vibc + W;
    ub.H = H; ub.n_unr = n_unrestricted; ub.n_idx = e->n_idx; ub.cap_rows = e->cap_rows;
    hipLaunchKernelGGL(k_upload_finish, dim3(1), dim3(1024), 0, s, e->s, ub, e->d_unr, e->d_isint);
    e->has_int = 0;
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(e->h_state, e->d_nnz, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));  // the staging buffer (and the host's view of it) is free again
    e->nnz = (long long)*reinterpret_cast<unsigned long long*>(e->h_state);
    e->uploaded = 1;
    e->has_save = 0;
    e->root_seq += 1;
    e->slot0_synced = 0;
    e->slots_synced = 0;
    drop_checkpoints(e);
    e->evaluation = 0;
    e->n_unr = n_unrestricted;
    e->s.has_unr = n_unrestricted > 0 ? 1 : 0;
    return e->n_opt > 0 ? resize_optional_objectives(e, 0) : JSLP_OK;  // a new model: optional objectives are set again by the caller
}

extern "C" int jslp_engine_set_optional_objectives(jslp_engine* e, int32_t n, const double* rows) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "set_optional_objectives before upload");
    if (n < 0 || (n > 0 && !rows)) return fail(JSLP_ERR_ARG, "set_optional_objectives: bad arguments");
    HIPC(hipSetDevice(e->device));
    HIPC(hipStreamSynchronize(e->res.stream));
    JSLP_TRY(resize_optional_objectives(e, n));
    if (n > 0) {
        HIPC(hipMemcpy2D(e->s.oo, sizeof(double) * e->ld, rows, sizeof(double) * e->W, sizeof(double) * e->W, n,
                         hipMemcpyHostToDevice));
    }
    return JSLP_OK;
}

extern "C" int jslp_engine_get_optional_objectives(jslp_engine* e, double* rows, int32_t* n_out) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "get_optional_objectives before upload");
    HIPC(hipSetDevice(e->device));
    if (n_out) *n_out = e->n_opt;
    if (rows && e->n_opt > 0) {
        HIPC(hipStreamSynchronize(e->res.stream));
        HIPC(hipMemcpy2D(rows, sizeof(double) * e->W, e->s.oo, sizeof(double) * e->ld, sizeof(double) * e->W, e->n_opt,
                         hipMemcpyDeviceToHost));
    }
    return JSLP_OK;
}

static Ctx host_ctx(const jslp_engine* e, int check_cycles) {
    Ctx c{};
    c.A = e->s.A; c.vibr = e->s.vibr; c.vibc = e->s.vibc; c.rbv = e->s.rbv; c.cbv = e->s.cbv; c.unr = e->s.unr;
    c.prow = e->s.prow; c.pcol = e->s.pcol; c.dirty = e->s.dirty; c.rhs = nullptr; c.oo = e->s.oo; c.n_opt = e->n_opt; c.st = e->s.st; c.hist = e->s.hist; c.hist_cap = e->s.hist_cap;
    c.trace = e->s.trace; c.trace_cap = e->s.trace_cap; c.ld = e->ld; c.W = e->W; c.check_cycles = check_cycles;
    c.batch = e->batch; c.use_partial = e->use_partial; c.precision = e->precision; c.stop_at_phase2 = 0;
    c.has_unr = e->n_unr > 0 ? 1 : 0;
    c.cnt = e->s.cnt;
    return c;
}

static int iters_cap(const jslp_engine* e) {
    // the reference has no iteration limit; this cap only turns an endless cycle (cycle check disabled) into
    // an error instead of a hung GPU
    long long cap = 2000000LL + 200LL * ((long long)e->cap_rows + e->W);
    if (e->test_iters_cap > 0) cap = std::min<long long>(cap, e->test_iters_cap);  // (tests: the exit at the cap after a handful of pivots)
    return (int)std::min<long long>(cap, 2000000000LL);
}

// dynamic LDS of the LDS-resident one-workgroup kernels (jslp_wglds.hip.h); 0 = use the generic kernels
static size_t wglds_smem(const jslp_engine* e) {
    if (!e->use_wglds) return 0;  // (optional objectives: round 3 -- their rows stay in the slot's global copy, jslp_wglds.hip.h)
    const size_t b = wglds_bytes(e->ld, e->cap_rows);
    return b <= WGLDS_MAX_BYTES ? b : 0;
}

// one workgroup for the whole simplex(): tiny tableaus, and SPARSE ones up to a few million cells -- a pivot of the
// LDS-resident one-workgroup kernel touches only the rows and columns the reference's gates let through (Monster LP, 1 %
// dense: ~5 us per pivot against ~12 for the chip-wide register-resident kernel, whose hand-off latency does not shrink with
// the work); dense tableaus of that size belong to the chip
static bool xl_fits(const jslp_engine* e, int H);
static const long long WG_CELLS_SPARSE = 1024LL * 1024;  // (Vendor Selection, 2.8 M cells, 0.3 % dense: 38.7 ms in one workgroup against 9.0 ms register-resident -- fill-in makes its pivots touch hundreds of rows)
static const double WG_SPARSE_DENSITY = 0.05;
static bool use_wg_single(const jslp_engine* e) {
    if (e->force_path == 1) return true;
    if (e->force_path == 2 || e->force_path == 3) return false;
    const long long cells = (long long)e->cap_rows * e->ld;
    if (e->force_xl) return false;
    if (cells <= WG_CELLS_SINGLE) return true;
    // (JSLP_XL=1: the XCD-local resident geometry takes the sparse mid-size LPs too)
    if (xl_fits(e, e->cap_rows) && !e->no_resident && e->force_path == 0) return false;
    return wglds_smem(e) != 0 && cells <= WG_CELLS_SPARSE && e->nnz >= 0 &&
           (double)e->nnz <= WG_SPARSE_DENSITY * (double)e->H0 * (double)e->W;
}
// ... that solve: the LDS-resident kernel when the tableau fits its LDS, else the generic one
static int solve_one_workgroup(jslp_engine* e, int check_cycles) {
    hipStream_t s = e->res.stream;
    const int cap = iters_cap(e);
    e->last_path = "workgroup";
    if (const size_t lds = wglds_smem(e); lds && e->s.n_opt > 0)  // optional objectives: a build of their own (jslp_wglds.hip.h)
        hipLaunchKernelGGL((k_simplex_lds<JSLP_WG_THREADS, true>), dim3(1), dim3(JSLP_WG_THREADS), lds, s, e->s, 0, check_cycles, cap, (int)e->cap_rows);
    else if (lds)
        hipLaunchKernelGGL((k_simplex_lds<JSLP_WG_THREADS>), dim3(1), dim3(JSLP_WG_THREADS), lds, s, e->s, 0, check_cycles, cap, (int)e->cap_rows);
    else
        hipLaunchKernelGGL((k_simplex_wg<JSLP_WG_THREADS, 4096>), dim3(1), dim3(JSLP_WG_THREADS), 0, s, e->s, 0, check_cycles, cap);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(e->h_state, e->s.st, sizeof(DevState), hipMemcpyDeviceToHost, s));
    return JSLP_OK;
}

#define JSLP_F_MAXNT 4
// the fused one-launch-per-pivot phase 2 (see k_pivot_fused for the preconditions)
static bool fused_eligible(const jslp_engine* e) {
    if (e->force_path == 2) return false;
    // (round 5: three and four column tiles per lane -- 4096 < ld <= 8192 -- for tableaus without unrestricted variables / optional objectives:
    //  3001 x 5001 ran k_update at 0.83 of the HBM peak but, with the one-workgroup k_select in front of every pivot, 17.3 k pivots/s = 0.52
    //  end to end, profiles/r05_streaming_workload_rows.md)
    const int max_tiles = (e->n_unr == 0 && e->n_opt == 0 && fused_wide_on()) ? JSLP_F_MAXNT : 2;
    return e->ld <= max_tiles * JSLP_F_TW && e->cap_rows <= 64 * JSLP_F_MAXG && e->precision >= 1e-15;
}

// ---- the register-resident kernel: geometries, instances, policy -----------------------------------------------------------------------------
#include "jslp_resident_table.hip.h"  // RES_GEOM (what each geometry number means) and resident_dispatch (key -> launch)
static bool xl_fits(const jslp_engine* e, int H) {
    return RES_WITH_XL && (e->xl_on || e->force_xl) && e->n_unr == 0 && e->n_opt == 0 && e->ld <= RES_GEOM[RES_GEOM_XL].max_ld && H <= JSLP_XL_MAXG * JSLP_R_MAXROWS &&
           e->precision >= 1e-15 && res_lean_on();
}
// variable indexes that can be live in a tableau of height H: constraints and variables are numbered first, cut slacks continue from
// lastElementIndex = width + height - 2 (tableau.ts:312-316) -- e->n_idx is the CAPACITY (every cut row the engine has room for)
// (an uploaded tableau need not follow the reference's contiguous numbering -- Model index reuse / removal, a direct C-API caller --
//  so the largest index upload() saw in the two maps counts too: the lean kernels' LDS copy of the "unrestricted" flags is indexed with it)
static int live_index_bound(const jslp_engine* e, int H) { return std::min<int>(e->n_idx, std::max<int>(e->W + H + 2, e->max_uploaded_idx + 1)); }
// The LEAN build takes this tableau: every one without unrestricted variables, optional objectives included (up to three rows of them in registers,
// round 3: resident_geometry); with unrestricted variables (round 4: per-lane column masks, the flags of all variable indexes in LDS) when the live
// indexes fit that LDS copy and there is no optional objective -- OPT && UNR is no instance: the fused pipeline takes those.
// (for resident_geometry the n_opt == 0 term changes nothing -- it admits optional objectives only when there are no unrestricted variables, so
//  with them n_unr == 0 has decided already; for the launch it is what keeps a key from naming an OPT && UNR instance)
static bool lean_takes(const jslp_engine* e, int H) {
    return res_lean_on() && (e->n_unr == 0 || (e->n_opt == 0 && live_index_bound(e, H) <= JSLP_R_LUNR));
}
static bool geometry_fits(const jslp_engine* e, int rpb, int g) { return e->ld <= RES_GEOM[g].max_ld && rpb <= RES_GEOM[g].rows; }
static int resident_geometry(const jslp_engine* e, int H) {
    if (e->no_resident || e->force_path == 2 || e->precision < 1e-15) return 0;  // (see k_pivot_fused for the precision condition)
    const int rpb = (H + JSLP_F_MAXG - 1) / JSLP_F_MAXG;
    const char* const gx = getenv("JSLP_RES_GEOM");
    // (JSLP_FORCE_PATH=resident keeps meaning the chip-wide geometries: the tests that force them at small sizes must keep covering them)
    if (xl_fits(e, H) && !gx && (e->force_xl || !e->force_resident)) return RES_GEOM_XL;
    const bool lean = lean_takes(e, H);
    const bool wide_tall_off = res_wide_tall() == 0 && !e->force_resident;
    if (e->n_opt > 0) {
        // optional objectives: the lean build of the headline geometry keeps up to three rows of them in registers (round 3);
        // everything else (unrestricted variables, taller / wider tableaus, more rows) runs them through the fused pipeline
        if (!lean || e->n_opt > 3) return 0;
        if (geometry_fits(e, rpb, 1)) return 1;
        // round 4: the tall geometry too (its lean phase 2 has the registers for three more rows per lane: 512 lanes x 4 columns);
        // the 6- and 8-column geometries do not (the objective rows would spill): the fused pipeline keeps those shapes
        return !wide_tall_off && geometry_fits(e, rpb, 3) ? 3 : 0;
    }
    if (gx) {  // experiments: force a geometry the tableau fits (lean build, no unrestricted variables)
        const int g = atoi(gx);
        if (g >= 1 && g <= 5 && e->n_unr == 0 && geometry_fits(e, rpb, g)) return g;
    }
    if (geometry_fits(e, rpb, 1)) return e->res_cpt == 4 ? 2 : 1;
    // The taller / wider geometries hold 64-72 MB of tableau in the 128 MB of vector registers and spill ~0.5 KB per lane to
    // scratch (560+ scratch loads in the pivot loop): measured at the end of round 2 they LOSE to the streaming kernels --
    // 4001 x 2001: 22.3 k pivots/s against 36.4 k through k_pivot_fused; 2501 x 2001: 26.6 k against 48.8 k; 3001 x 3001: 21.5 k
    // against 23.7 k through k_select + k_update; 2001 x 4001: 20.1 k against 26.1 k (tools/tall_one.py, r02_z).  They stay
    // built and tested (JSLP_FORCE_PATH=resident, JSLP_RES_WIDE_TALL=1) but the default policy no longer picks them.
    // Round 3: the LEAN build's pipelined phase 2 does fit (jslp_resident_pipe.hip.h; 4 scratch loads per pivot) and beats the
    // streaming kernels 2-3x on these shapes (r03_j), so tableaus it can take -- no unrestricted variables -- get these geometries
    // by default for their phase 2 (phase 1 through the fused pipeline: run_simplex).  JSLP_RES_WIDE_TALL=0 switches that off, =1
    // also sends the general build's (unrestricted variables) there.
    // (round 4: the lean build takes unrestricted variables too -- lean_takes; the tall / wide geometries have NO general build any more -- it
    //  spilled ~0.5 KB per lane and lost to the streaming kernels -- so what the lean build cannot take goes to the fused pipeline)
    if (!lean || wide_tall_off) return 0;
    for (int g = 3; g <= 5; g++)
        if (geometry_fits(e, rpb, g)) return g;
    return 0;
}
static bool resident_eligible(const jslp_engine* e, int H) { return resident_geometry(e, H) != 0; }

static int ensure_resident(jslp_engine* e, bool want_hist = false) {
    // (`want_hist`: the lean kernel's per-workgroup copies of the cycle-check history, 256 MiB -- carved only once a solve with the
    //  cycle check on takes the lean build: pool members, short-lived engines and check-off solves never pay for it)
    if (want_hist) e->r_want_hist = 1;
    //  (JSLP_RES_GEOM can force a geometry WIDER than the tableau needs -- 6 or 8 columns per lane on ld <= 2048 / <= 3072 --, whose slots are
    //   lanes x columns per lane doubles whatever ld is: with the knob set every slot is sized for the widest geometry, 4096 doubles + skew;
    //   the knob is read per call, so an engine carved without it is carved again)
    const size_t slot_doubles = getenv("JSLP_RES_GEOM") ? (size_t)4096 + JSLP_PUB_SKEW / 8
                                : (e->ld <= 2048 ? (size_t)e->ld : ((size_t)e->ld + 1023) / 1024 * 1024 + JSLP_PUB_SKEW / 8);
    if (e->r_sync && (!e->r_want_hist || e->r_hist_all) && e->r_slot_doubles >= slot_doubles) return JSLP_OK;
    if (e->r_sync) HIPC(hipStreamSynchronize(e->res.stream));  // re-carving: nothing in flight may still use the old layout
    // hand-off buffers and the safety-net copy of slot 0 (matrix, maps, state) carved from ONE allocation, which the
    // resource pool hands from engine to engine (allocating and freeing these cost a small Solve more than its pivots)
    HIPC_CARVE(e->res.r_arena, [&](Carver& cv) {
        e->r_gran = cv.take<u64_t>(JSLP_R_SYNC_WORDS);
        // (slots ld doubles apart; the 6- and 8-column geometries' permuted layout -- jslp_resident_pipe.hip.h, SLOT -- takes lanes x columns per lane
        //  = 3072 / 4096 doubles plus a skew per slot)
        for (int i = 0; i < 2; i++) e->r_rows[i] = cv.take<u64_t>((size_t)JSLP_F_MAXG * slot_doubles);
        e->r_hist_all = e->r_want_hist ? cv.take<int2>((size_t)JSLP_F_MAXG * JSLP_PIPE_GHIST) : nullptr;  // every workgroup's own copy of the cycle-check history (lean kernel)
        e->r_sync = cv.take<unsigned>(16);
        e->rb_A = cv.take<double>((size_t)e->cap_rows * e->ld);
        e->rb_vibr = cv.take<int32_t>((size_t)e->cap_rows);
        e->rb_vibc = cv.take<int32_t>((size_t)e->W);
        e->rb_rbv = cv.take<int32_t>((size_t)e->n_idx);
        e->rb_cbv = cv.take<int32_t>((size_t)e->n_idx);
        e->r_backup_st = cv.take<DevState>(1);
        e->r_ctx_dev = reinterpret_cast<Ctx*>(cv.take<char>(sizeof(Ctx) + 16));  // (+ the address of the host-abort word: JSLP_HOST_ABORT_CHECK)
        e->r_slot_doubles = slot_doubles;
    });
    return JSLP_OK;
}

static int ensure_fused(jslp_engine* e) {
    if (e->f_ready) return JSLP_OK;  // (set last: a call that failed half way is not taken for done by the next)
    const size_t cells = (size_t)e->cap_rows * e->ld;
    HIPC(e->f_buf1.reserve(sizeof(double) * cells));
    HIPC(hipMemsetAsync(e->f_buf1.p, 0, sizeof(double) * cells, e->res.stream));
    for (int i = 0; i < 2; i++) {
        HIPC(e->f_cands[i].reserve(sizeof(FCand) * JSLP_F_MAXG));
        HIPC(e->f_pcol[i].reserve(sizeof(double) * e->cap_rows));
        HIPC(e->f_st[i].reserve(sizeof(DevState)));
        HIPC(hipMemsetAsync(e->f_st[i].p, 0, sizeof(DevState), e->res.stream));
    }
    HIPC(e->f_uflags.reserve(2 * ((size_t)e->ld + (size_t)e->cap_rows)));
    HIPC(hipMemsetAsync(e->f_uflags.p, 0, 2 * ((size_t)e->ld + (size_t)e->cap_rows), e->res.stream));
    e->f_ready = 1;
    return JSLP_OK;
}

static int ensure_fused_oo(jslp_engine* e) {  // (the number of optional objectives is set per model, after create())
    if (e->n_opt <= e->f_oo1_rows) return JSLP_OK;
    HIPC(hipStreamSynchronize(e->res.stream));
    e->f_oo1_rows = 0;
    HIPC(e->f_oo1.reserve(sizeof(double) * (size_t)e->n_opt * e->ld));
    HIPC(hipMemsetAsync(e->f_oo1.p, 0, sizeof(double) * (size_t)e->n_opt * e->ld, e->res.stream));
    e->f_oo1_rows = e->n_opt;
    return JSLP_OK;
}
static FusedCtx make_fused_ctx(const jslp_engine* e, const Ctx& c, int H) {
    FusedCtx f;
    f.c = c;
    f.buf[0] = e->s.A; f.buf[1] = e->f_buf1.as<double>();
    for (int i = 0; i < 2; i++) { f.cands[i] = e->f_cands[i].as<FCand>(); f.pcol[i] = e->f_pcol[i].as<double>(); f.fst[i] = e->f_st[i].as<DevState>(); }
    f.rpb = (H + JSLP_F_MAXG - 1) / JSLP_F_MAXG;
    f.G = (H + f.rpb - 1) / f.rpb;
    f.H = H;
    f.nt = e->nt;
    for (int i = 0; i < 2; i++) {
        f.ucol[i] = e->f_uflags.as<uint8_t>() + (size_t)i * ((size_t)e->ld + e->cap_rows);
        f.urow[i] = f.ucol[i] + e->ld;
    }
    f.oo[0] = e->s.oo; f.oo[1] = e->f_oo1.as<double>();
    return f;
}

static dim3 update_grid(const jslp_engine* e, int H) {
    return dim3((e->ld + JSLP_UPD_COLS - 1) / JSLP_UPD_COLS, (H + JSLP_UPD_ROWS - 1) / JSLP_UPD_ROWS, 1);
}

// Math.round: nearest integer, ties toward +Infinity
static double js_round(double x) {
    if (!std::isfinite(x)) return x;
    const double f = floor(x);
    return (x - f >= 0.5) ? f + 1.0 : f;
}

// checkForCycles (simplex.ts:415-440) on the downloaded history: only to rebuild the exact [start, length]
// the reference pushes to model.messages; hit / no-hit was decided on the device.
static void cycle_message(const std::vector<int2>& h, int32_t* start, int32_t* len) {
    const long long n = (long long)h.size();
    for (long long e1 = 0; e1 < n - 1; e1++)
        for (long long e2 = e1 + 1; e2 < n; e2++)
            if (h[e1].x == h[e2].x && h[e1].y == h[e2].y) {
                if (e2 - e1 > n - e2) break;
                bool found = true;
                for (long long i = 1; i < e2 - e1; i++)
                    if (h[e1 + i].x != h[e2 + i].x || h[e1 + i].y != h[e2 + i].y) { found = false; break; }
                if (found) { *start = (int32_t)e1; *len = (int32_t)(e2 - e1); return; }
            }
    *start = -1; *len = 0;
}

static int state_error(const DevState& st) {
    switch (st.err) {
        case ERR_NONE: return JSLP_OK;
        case ERR_HIST_FULL: return fail(JSLP_ERR_CAPACITY, "simplex: cycle-check history capacity exceeded");
        case ERR_ITER_LIMIT: return fail(JSLP_ERR_CAPACITY, "simplex: iteration safety cap reached (endless cycle?)");
        case ERR_CUT_ARG: return fail(JSLP_ERR_ARG, "add_cuts: variable index out of range or neither basic nor non-basic");
        case ERR_CAPACITY: return fail(JSLP_ERR_CAPACITY, "add_cuts: row / element-index capacity exceeded");
        case ERR_BARRIER: return fail(JSLP_ERR_DEVICE, "resident simplex kernel: grid barrier timed out (workgroups not co-resident?)");
        case ERR_NOT_SYNCED: return fail(JSLP_ERR_STATE, "internal: one-launch node kernel used on a slot that is not in sync with the snapshot");
        case ERR_MIR_ROUNDS: return fail(JSLP_ERR_CAPACITY, "relax_mir: the MIR loop reached JSLPR_MAX_ROUNDS without a stop");
    }
    return fail(JSLP_ERR_DEVICE, "unknown device error code");
}

// fold a finished DevState into the ABI result (evaluation semantics: see jslp_simplex_result)
// (decode_state: everything but the cycle message, which needs the history; shared with the pack of small LPs, jslpp_pack_simplex)
static void decode_state(const DevState& st, double precision, double prev_evaluation, jslp_simplex_result* out, double* evaluation_out) {
    memset(out, 0, sizeof *out);
    out->feasible = st.feasible;
    out->bounded = st.bounded;
    out->optimal = st.optimal;
    out->unbounded_var_index = st.bounded ? -1 : st.unbounded_var;
    out->pivots_phase1 = st.it1;
    out->pivots_phase2 = st.entered_phase2 ? st.it2 : -1;
    out->cycle_phase = st.cycle_phase;
    out->height = st.H;
    out->obj_cell = st.obj_cell;
    double ev = prev_evaluation;
    if (st.optimal) {  // setEvaluation (tableau.ts:420-426)
        const double rc = js_round(1.0 / precision);
        ev = js_round((2.220446049250313e-16 + st.obj_cell) * rc) / rc;
    } else if (!st.bounded) {
        ev = -INFINITY;
    }
    out->evaluation = ev;
    if (evaluation_out) *evaluation_out = ev;
}
static int fill_result(jslp_engine* e, const DevState& st, int slot, double prev_evaluation, jslp_simplex_result* out,
                       double* evaluation_out) {
    decode_state(st, e->precision, prev_evaluation, out, evaluation_out);
    if (st.cycle_phase && st.hist_n > 0) {
        std::vector<int2> h(st.hist_n);
        if (hipMemcpy(h.data(), e->s.hist + (size_t)slot * e->s.hist_cap, sizeof(int2) * st.hist_n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(JSLP_ERR_DEVICE, "cycle history read-back failed");
        cycle_message(h, &out->cycle_start, &out->cycle_length);
    }
    return JSLP_OK;
}

static int ensure_events(jslp_engine* e, size_t n) {
    while (e->ev_pool.size() < n) {
        Event ev;
        HIPC(hipEventCreate(&ev.h));
        e->ev_pool.push_back(std::move(ev));
    }
    return JSLP_OK;
}

// host half of the work counters: one finished simplex() (a relaxation when it came with restore + cuts)
static void account(jslp_engine* e, const DevState& st, int is_relaxation) {
    if (!e->counting) return;
    e->wc.simplex_calls += 1;
    e->wc.relaxations += is_relaxation ? 1 : 0;
    e->wc.pivots += (long long)st.it1 + st.it2;
    e->wc.height_sum += st.H;
}
// The dense half of gated_cells / gated_rows (include/jslp_engine.h, jslp_work_counters): k_fused_p1, k_pivot_fused and k_simplex_resident stream every
// row and every cell and carry no counting code, so the host adds (H - 1) rows x W cells for each pivot THEY performed -- every call site passes
// the pivots of its own launches only.  The one-workgroup kernels and k_select (the slow pivot included) count through the gate on the device.
static void count_dense(jslp_engine* e, int H, long long pivots) {
    if (!e->counting || pivots <= 0) return;
    e->wc.gated_cells += pivots * (long long)(H - 1) * e->W;
    e->wc.gated_rows += pivots * (long long)(H - 1);
}
static long long pivots_done(const jslp_engine* e) { return (long long)e->h_state->it1 + e->h_state->it2; }  // of the host's copy of the state

// ---- simplex() of the live tableau (slot 0) ------------------------------------------------------------------------------------------------
// What one simplex() call fixes once (plan_solve); every phase below takes the engine and this.
struct SolveRun {
    Ctx c;                     // the streaming kernels' context; c.stop_at_phase2 = fused
    int H = 0;                 // height: fixed during a simplex call, read once
    int cap = 0;               // iteration cap (iters_cap)
    int check_cycles = 0;
    dim3 grid;                 // k_update's
    int geometry = 0;          // of the register-resident kernel (RES_GEOM), 0: it does not take this tableau
    bool lean = false;         // ... and its lean build does (lean_takes)
    bool phase2_only = false;  // ... but only phase 2 of it (the tall / wide geometries: plan_solve)
    bool fused = false;        // the fused one-launch-per-pivot pipeline applies (fused_eligible)
    bool dbg = false;          // JSLP_DEBUG_LAUNCH: one parseable stderr line per launch decision (tests/test_grid_edges.py)
};
static int plan_solve(jslp_engine* e, int check_cycles, SolveRun* p) {
    hipStream_t s = e->res.stream;
    p->check_cycles = check_cycles;
    p->cap = iters_cap(e);
    p->c = host_ctx(e, check_cycles);
    p->fused = fused_eligible(e);
    p->c.stop_at_phase2 = p->fused ? 1 : 0;
    p->dbg = debug_launch_on();
    e->last_path = "select+update";
    // height is fixed during a simplex call; read it once
    HIPC(hipMemcpyAsync(e->h_state, e->s.st, sizeof(DevState), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    p->H = e->h_state->H;
    p->grid = update_grid(e, p->H);
    p->geometry = resident_geometry(e, p->H);
    p->lean = lean_takes(e, p->H);
    // The headline geometries run the WHOLE solve register-resident (phase 1 included).  The tall / wide ones (H > 2048 or more
    // than 2048 columns) take only phase 2 there -- their phase-1 loop does not fit the 256 registers a lane has next to 64-72 MB
    // of tableau (it spills: 22 k pivots/s against 33.7 k through k_fused_p1 on 4001 x 2001) while the lean kernel's pipelined
    // phase 2 does (4 scratch loads per pivot): phase 1 goes through the fused pipeline first, which hands over with
    // ST_PHASE1_DONE.  r03_j: 4001 x 2001 113.4 k pivots/s against 35.7 k fused, 2501 x 2001 128.6 k against 48.5 k,
    // 2001 x 4001 75.5 k against 34.8 k.
    p->phase2_only = p->geometry >= 3 && p->geometry != RES_GEOM_XL;  // (XCD-local: the whole solve, like the headline geometry)
    return JSLP_OK;
}
static int fetch_state(jslp_engine* e, const DevState* from) {  // the host's copy of a device state, waited for
    HIPC(hipMemcpyAsync(e->h_state, from, sizeof(DevState), hipMemcpyDeviceToHost, e->res.stream));
    HIPC(hipStreamSynchronize(e->res.stream));
    return JSLP_OK;
}

// ---- register-resident path: the WHOLE simplex (phase 1 and phase 2) in one cooperative launch -----------------------------------------------
enum class Resident {
    NotTried,
    Done,        // the kernel finished the solve: e->h_state is final
    Streaming,   // the lean kernel left mid-solve and no general build can continue: the streaming kernels go on from the state it wrote back
    RolledBack,  // a hand-off timed out (or the host asked): slot 0 and e->h_state are what they were before the launch
    Refused,     // the runtime refused the cooperative launch, or no such instance exists: nothing ran
};
// Word offsets of the hand-off areas in e->r_gran.  They mirror, term by term, the sums JSLP_R_SYNC_WORDS_GENERAL and JSLP_R_SYNC_WORDS are
// written as (jslp_resident.hip.h): [2][G][8] granules | [2][G] row flags | 32 words of decision / verdict | [2][G] chip-wide OR flags || the lean kernel's
// [2][G] summary granules, 64 bytes apart | [2][copies][G] row-flag copies | the row records | the XCD-local build's placement census
enum : size_t {
    R_OFF_GRAN = 0,
    R_OFF_ROWFLAG = R_OFF_GRAN + 2 * JSLP_F_MAXG * JSLP_R_GRAN,
    R_OFF_DECISION = R_OFF_ROWFLAG + 2 * JSLP_F_MAXG,  // decision[0], decision[1], verdict[0], verdict[1]: 8 words each
    R_OFF_GOR = R_OFF_DECISION + 32,
    R_OFF_GRAN16 = R_OFF_GOR + 2 * JSLP_F_MAXG,
    R_OFF_ROWFLAGC = R_OFF_GRAN16 + 2 * JSLP_F_MAXG * 8,
    R_OFF_REC = R_OFF_ROWFLAGC + 2 * JSLP_R_FLAGCOPIES * JSLP_F_MAXG,
    R_OFF_CENSUS = R_OFF_REC + JSLP_R_REC_WORDS,
    R_OFF_END = R_OFF_CENSUS + JSLP_F_MAXG,
};
static_assert(R_OFF_GRAN16 == JSLP_R_SYNC_WORDS_GENERAL && R_OFF_END == JSLP_R_SYNC_WORDS, "the offsets add up to the sizes the kernels' header states");
static_assert((R_OFF_REC - R_OFF_GRAN16) * 8 == JSLP_R_REC_OFF, "the kernels reach the row records from gran16");
// the kernel's argument, carved out of the hand-off words (ensure_resident first: it may move them)
static ResCtx make_res_ctx(const jslp_engine* e, const SolveRun& p) {
    ResCtx rc;
    rc.c = p.c;
    for (int i = 0; i < 2; i++) {
        rc.gran[i] = e->r_gran + R_OFF_GRAN + (size_t)i * JSLP_F_MAXG * JSLP_R_GRAN;
        rc.rowflag[i] = e->r_gran + R_OFF_ROWFLAG + (size_t)i * JSLP_F_MAXG;
        rc.rows_pub[i] = e->r_rows[i];
        rc.decision[i] = e->r_gran + R_OFF_DECISION + (size_t)i * 8;
        rc.verdict[i] = e->r_gran + R_OFF_DECISION + 16 + (size_t)i * 8;
        rc.gor[i] = e->r_gran + R_OFF_GOR + (size_t)i * JSLP_F_MAXG;
        rc.rowflagc[i] = e->r_gran + R_OFF_ROWFLAGC + (size_t)i * JSLP_R_FLAGCOPIES * JSLP_F_MAXG;
    }
    rc.gran16 = e->r_gran + R_OFF_GRAN16;  // [2][MAXG] granules, 64 bytes apart
    rc.census = e->r_gran + R_OFF_CENSUS;
    rc.hist_all = e->r_hist_all;
    rc.abort_flag = e->r_sync + 4;
    rc.cdev = e->r_ctx_dev;
    const int maxg = p.geometry == RES_GEOM_XL ? JSLP_XL_MAXG : JSLP_F_MAXG;
    rc.rpb = (p.H + maxg - 1) / maxg;
    if (const char* rx = getenv("JSLP_RES_RPB"); rx && p.geometry != RES_GEOM_XL) {  // experiments: more rows per workgroup = fewer workgroups (<= the geometry's rows)
        const int want = atoi(rx);
        if (want > rc.rpb && want <= RES_GEOM[p.geometry].rows) rc.rpb = want;
    }
    rc.G = (p.H + rc.rpb - 1) / rc.rpb;
    rc.H = p.H;
    rc.n_idx = live_index_bound(e, p.H);
    rc.iters_cap = p.cap;
    rc.spin_limit = e->spin_limit;
    rc.test_abort_epoch = e->test_abort_epoch;
    rc.test_late_wave0 = e->test_late_wave0;
    rc.dbg = nullptr;
    return rc;
}
// what a launch needs on the stream in front of it: zeroed hand-off words, the device copy of the context, the host-abort word
static int resident_setup(jslp_engine* e, const SolveRun& p, ResCtx& rc) {
    hipStream_t s = e->res.stream;
    HIPC(hipMemsetAsync(e->r_gran, 0, sizeof(u64_t) * JSLP_R_SYNC_WORDS, s));  // tags restart at 1
    HIPC(hipMemcpyAsync(e->r_ctx_dev, &rc.c, sizeof(Ctx), hipMemcpyHostToDevice, s));  // (200 bytes; the kernel's one committing thread reads the map / trace pointers from it)
    // the host-abort word (pinned, behind the state and the retry counter) and its address behind the device copy of the context
    unsigned* const h_abort = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(e->h_state) + sizeof(DevState) + 16);
    *h_abort = 0u;
    e->h_abort_ptr = h_abort;
    HIPC(hipMemcpyAsync(reinterpret_cast<char*>(e->r_ctx_dev) + sizeof(Ctx), &e->h_abort_ptr, sizeof(unsigned*), hipMemcpyHostToDevice, s));
#ifdef JSLP_DEBUG_RESIDENT
    static DevBuf& dbg_mem = *new DevBuf();  // (never destroyed: see g_pool)
    HIPC(dbg_mem.reserve(sizeof(u64_t) * (512 * JSLP_F_MAXG * 2 + 16384)));
    u64_t* const dbg_buf = dbg_mem.as<u64_t>();
    HIPC(hipMemsetAsync(dbg_buf, 0, sizeof(u64_t) * (512 * JSLP_F_MAXG * 2 + 16384), s));
    rc.dbg = dbg_buf;
#endif
    HIPC(hipMemsetAsync(e->r_sync, 0, sizeof(unsigned) * 16, s));
    if (p.geometry == RES_GEOM_XL) {
        // the XCD-local build's rows carry their epoch tag INSIDE the data and every launch's tags restart at 1: what an earlier
        // launch left in the row slots would pass for this launch's rows (found by the Knapsack fixture's fifth relaxation: same
        // pivots, another RHS) -- the slots start from zero (tag 0 is never used)
        for (int i = 0; i < 2; i++) HIPC(hipMemsetAsync(e->r_rows[i], 0, (size_t)rc.G * e->ld * 16, s));
    }
    return JSLP_OK;
}
// Safety net.  The kernel commits every pivot's index-map swap as it goes but writes the matrix back only in
// its epilogue, and a timed-out hand-off (workgroups not co-resident, a stalled GPU) skips that epilogue: keep a
// copy of slot 0 (one pass over the matrix, ~15 us at 2001 x 2001 against a ~100 ms solve) to roll back to.
static void resident_safety_net(jslp_engine* e, const SolveRun& p, int save) {  // save 1: slot 0 -> the copy; 0: the copy -> slot 0
    SnapshotW bk{e->rb_A, e->rb_vibr, e->rb_vibc, e->rb_rbv, e->rb_cbv, e->n_idx, nullptr, nullptr};
    hipLaunchKernelGGL(k_res_backup, dim3(copy_grid(e, 1).x), dim3(256), 0, e->res.stream, e->s, bk, e->r_backup_st, p.H, save);
}
// JSLP_INJECT_RESIDENT_ABORT_US=<n>: raise the host-abort word n microseconds into the launch -- the rollback path (kernel gives
// up mid-solve, slot 0 restored from the safety-net copy, the solve re-run through the streaming kernels) exercised on the
// library users load, whose kernels have no test hooks.  Read per launch (tests set it inside one process); once per solve.
// (parsed strictly -- a stray or garbage value no longer aborts every resident solve -- and announced once)
static void inject_resident_abort(jslp_engine* e) {
    const char* inj = getenv("JSLP_INJECT_RESIDENT_ABORT_US");
    if (!inj || !*inj || e->abort_injected) return;
    char* endp = nullptr;
    const long us = strtol(inj, &endp, 10);
    if (endp == inj || *endp != 0 || us < 0 || us > 10000000L) return;
    static std::atomic<int> told{0};
    if (!told.exchange(1)) fprintf(stderr, "[jslp] JSLP_INJECT_RESIDENT_ABORT_US=%ld: every register-resident solve is aborted %ld us after its launch and re-run through the streaming kernels (fault injection)\n", us, us);
    e->abort_injected = 1;
    std::this_thread::sleep_for(std::chrono::microseconds(us));
    __atomic_store_n(e->h_abort_ptr, 1u, __ATOMIC_RELEASE);
}
// One cooperative launch of the instance the plan's geometry and `lean` name; *le: what the runtime said (hipErrorInvalidValue: no such instance).
// The LEAN build (all-gather protocol only, software-pipelined phase 2: jslp_resident_pipe.hip.h) takes every solve it can (lean_takes); the general
// build is what a lean solve of the 8-row geometries is handed to (resident_attempt).  Lane geometry: up to 8 rows per workgroup: 1024 lanes x 2 columns
// (or 512 x 4, half the waves per workgroup barrier, measured slower); 9..16 rows (2048 < H <= 4096): 512 lanes x 4 columns x 16 rows -- 2 waves per SIMD
// leave 256 VGPRs per lane for the 64 MB of tableau.
static int resident_launch(jslp_engine* e, const SolveRun& p, const ResCtx& rc, bool lean, hipError_t* le) {
    const ResGeom& g = RES_GEOM[p.geometry];
    const bool unr = e->n_unr > 0;  // unrestricted variables: the UNR build threads the per-column flags through
    // (chk: the instance's template key -- the general build is compiled with CHK = true and reads check_cycles at run time)
    const int key[8] = {g.threads, g.cols, g.rows, unr ? 1 : 0, lean ? 1 : 0, e->n_opt > 0 ? 1 : 0, (p.check_cycles != 0 || !lean) ? 1 : 0, p.geometry == RES_GEOM_XL ? 1 : 0};
    const int r = resident_dispatch(key, (unsigned)rc.G, &rc, e->res.stream);
    if (r == -1 && RES_DEV_REFUSAL) return fail(JSLP_ERR_UNSUPPORTED, "%s", RES_DEV_REFUSAL);
    *le = r == -1 ? hipErrorInvalidValue : (hipError_t)r;  // (-1: no such instance -- the refusal branch counts it)
    if (*le != hipSuccess) return JSLP_OK;
    e->resident_launches += 1;
    if (p.dbg)  // which instance ran, one parseable line per accepted launch (tests/test_grid_edges.py)
        fprintf(stderr, "[jslp] launch k_simplex_resident<%d,%d,%d> unr %d lean %d opt %d chk %d xl %d G %d rpb %d\n", key[0], key[1], key[2], key[3], key[4], key[5],
                key[6], key[7], rc.G, rc.rpb);
    if (lean) inject_resident_abort(e);
    return JSLP_OK;
}
// the launch's share of upd_ms / upd_launches, between the events around it; unit = one pivot (16*H*W algorithmic bytes)
static void account_resident_time(jslp_engine* e, long long it_before) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e->ev_pool[0], e->ev_pool[1]) == hipSuccess) e->upd_ms += ms;
    e->upd_launches += e->h_state->it1 + e->h_state->it2 - it_before;
}
// an accepted launch has run to its end: the final state, or the roll back to the safety-net copy
static int resident_finish(jslp_engine* e, const SolveRun& p, const ResCtx& rc, long long it_before, Resident* out) {
    hipStream_t s = e->res.stream;
    if (e->timing) HIPC(hipEventRecord(e->ev_pool[1], s));
    JSLP_TRY(fetch_state(e, e->s.st));
    if (e->timing) account_resident_time(e, it_before);
    if (e->h_state->err == ERR_BARRIER) {
        // roll slot 0 back to its state before the launch and solve through the streaming kernels instead
        resident_safety_net(e, p, 0);
        HIPC(hipGetLastError());
        // ... and the host's copy of the state with it: the streaming loops start from what h_state says (the tall /
        // wide geometries come here with ST_PHASE1_DONE: without this the aborted kernel's ST_DONE + ERR_BARRIER ended the
        // solve as a device error instead of finishing it through k_pivot_fused)
        JSLP_TRY(fetch_state(e, e->s.st));
        e->resident_fallbacks += 1;
        *out = Resident::RolledBack;
        return JSLP_OK;
    }
    *out = Resident::Done;
    e->last_path = p.geometry == RES_GEOM_XL ? "resident-xl" : "resident";
    count_dense(e, p.H, pivots_done(e) - it_before);  // (not what a fused phase 1 in front of the launch did: that is counted there)
#ifdef JSLP_DEBUG_RESIDENT
    {   // phase timing + micro-costs of the debug build (tools/resident_phase_timing.py reads this file)
        std::vector<u64_t> d(16384);
        HIPC(hipMemcpy(d.data(), rc.dbg + (size_t)512 * rc.G * 2, sizeof(u64_t) * 16384, hipMemcpyDeviceToHost));
        FILE* fb = fopen("gpurun_out/resident_r0.bin", "wb");
        if (fb) { fwrite(d.data(), 8, 16384, fb); fclose(fb); }
        HIPC(hipMemcpy(d.data(), rc.dbg, sizeof(u64_t) * 16384, hipMemcpyDeviceToHost));  // RT_STAMP: [8 epochs][MAXG][8 events]
        fb = fopen("gpurun_out/resident_stamps.bin", "wb");
        if (fb) { fwrite(d.data(), 8, 16384, fb); fclose(fb); }
    }
#else
    (void)rc;
#endif
    return JSLP_OK;
}
// `it_before`: pivots the solve had done when the kernel is launched (0, or a phase 1 done by the fused pipeline)
static int resident_attempt(jslp_engine* e, const SolveRun& p, long long it_before, Resident* out) {
    hipStream_t s = e->res.stream;
    // (the lean kernel's per-workgroup copies of the cycle-check history are carved once a lean solve with the check on comes by: ensure_resident)
    JSLP_TRY(ensure_resident(e, p.lean && p.check_cycles != 0));
    ResCtx rc = make_res_ctx(e, p);
    JSLP_TRY(resident_setup(e, p, rc));
    resident_safety_net(e, p, 1);
    if (e->timing) { JSLP_TRY(ensure_events(e, 2)); HIPC(hipEventRecord(e->ev_pool[0], s)); }
    // The lean build first.  Should its cycle-check history outgrow LDS it hands the solve over (status ST_RUNNING / ST_PHASE1_DONE instead of
    // ST_DONE) and the general build continues it in a second launch: at most two trips
    bool lean = p.lean;
    hipError_t le = hipErrorInvalidValue;
    for (int trip = 0; trip < 2; trip++) {
        JSLP_TRY(resident_launch(e, p, rc, lean, &le));
        if (le != hipSuccess || !lean) break;
        // did the lean kernel finish the solve?
        unsigned* const h_retries = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(e->h_state) + sizeof(DevState) + 8);
        HIPC(hipMemcpyAsync(e->h_state, e->s.st, sizeof(DevState), hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(h_retries, e->r_sync + 5, sizeof(unsigned), hipMemcpyDeviceToHost, s));  // repeated looks of the checksummed row hand-over
        HIPC(hipStreamSynchronize(s));
        e->resident_fetch_retries += *h_retries;
        if (e->h_state->err != ERR_NONE || e->h_state->status == ST_DONE) break;
        e->resident_handovers += 1;
        if (e->n_opt > 0 || p.geometry >= 3) {
            // (XCD-local and tall / wide geometries: there is no general build of them)
            // optional objectives: the general build does not take them -- the streaming kernels continue from the state the
            // lean kernel left (tableau, maps and objective rows written back; status ST_RUNNING or ST_PHASE1_DONE)
            if (e->timing) { HIPC(hipEventRecord(e->ev_pool[1], s)); HIPC(hipEventSynchronize(e->ev_pool[1])); account_resident_time(e, it_before); }
            count_dense(e, p.H, pivots_done(e) - it_before);  // the pivots the lean kernel did before it left
            *out = Resident::Streaming;
            return JSLP_OK;
        }
        lean = false;
        HIPC(hipMemsetAsync(e->r_gran, 0, sizeof(u64_t) * JSLP_R_SYNC_WORDS, s));  // the second launch's tags restart at 1
    }
    if (le == hipSuccess) return resident_finish(e, p, rc, it_before, out);
    (void)hipGetLastError();  // not co-resident on this device: use one launch per pivot instead
    e->resident_refusals += 1;
    if (p.dbg)
        fprintf(stderr, "[jslp] cooperative launch of k_simplex_resident refused (geometry %d, lean %d, unr %d, G %d): %s\n", p.geometry, (int)lean,
                (int)(e->n_unr > 0), rc.G, hipGetErrorString(le));
    *out = Resident::Refused;
    return JSLP_OK;
}

// ---- the streaming kernels: k_select + k_update per pivot, or one fused launch per pivot -----------------------------------------------------
struct FusedKernel {  // one descriptor per instantiation of k_fused_p1 / k_pivot_fused
    void (*fn)(FusedCtx, int);
    const char* name;  // the JSLP_DEBUG_LAUNCH line
};
// column tiles per lane (ld <= 2048: one) x unrestricted variables present; beyond two tiles plain tableaus only (fused_eligible)
static const FusedKernel FUSED_P1[6] = {
    {k_fused_p1<1, true>, "k_fused_p1<1,1>"}, {k_fused_p1<1, false>, "k_fused_p1<1,0>"}, {k_fused_p1<2, true>, "k_fused_p1<2,1>"},
    {k_fused_p1<2, false>, "k_fused_p1<2,0>"}, {k_fused_p1<3, false>, "k_fused_p1<3,0>"}, {k_fused_p1<4, false>, "k_fused_p1<4,0>"}};
// ... x optional objectives present
static const FusedKernel PIVOT_FUSED[10] = {
    {k_pivot_fused<1, true, true>, "k_pivot_fused<1,1,1>"}, {k_pivot_fused<1, true, false>, "k_pivot_fused<1,1,0>"},
    {k_pivot_fused<1, false, true>, "k_pivot_fused<1,0,1>"}, {k_pivot_fused<1, false, false>, "k_pivot_fused<1,0,0>"},
    {k_pivot_fused<2, true, true>, "k_pivot_fused<2,1,1>"}, {k_pivot_fused<2, true, false>, "k_pivot_fused<2,1,0>"},
    {k_pivot_fused<2, false, true>, "k_pivot_fused<2,0,1>"}, {k_pivot_fused<2, false, false>, "k_pivot_fused<2,0,0>"},
    {k_pivot_fused<3, false, false>, "k_pivot_fused<3,0,0>"}, {k_pivot_fused<4, false, false>, "k_pivot_fused<4,0,0>"}};
static int fused_tiles(const jslp_engine* e) { return std::min((e->ld + JSLP_F_TW - 1) / JSLP_F_TW, JSLP_F_MAXNT); }
static const FusedKernel& fused_p1_kernel(const jslp_engine* e) {
    const int t = fused_tiles(e);
    return FUSED_P1[t <= 2 ? 2 * (t - 1) + (e->n_unr > 0 ? 0 : 1) : t + 1];
}
static const FusedKernel& pivot_fused_kernel(const jslp_engine* e) {
    const int t = fused_tiles(e);
    return PIVOT_FUSED[t <= 2 ? 4 * (t - 1) + (e->n_unr > 0 ? 0 : 2) + (e->n_opt > 0 ? 0 : 1) : t + 5];
}
static void launch_fused(const jslp_engine* e, const FusedKernel& k, const FusedCtx& f, int launch) {
    hipLaunchKernelGGL(k.fn, dim3(f.G), dim3(JSLP_F_THREADS), 0, e->res.stream, f, launch);
}
// add up the event pairs of the pivots of a chunk that really ran: launches after the solve ended are no-ops, only the first `real` did a pivot.
// Returns the solve's pivot count, the next chunk's `done_prev`
static long long account_chunk_time(jslp_engine* e, int chunk, long long done_prev) {
    const long long done = (long long)e->h_state->it1 + e->h_state->it2;
    const long long real = std::min<long long>(chunk, done - done_prev);
    for (long long i = 0; i < real; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, e->ev_pool[2 * i], e->ev_pool[2 * i + 1]) == hipSuccess) e->upd_ms += ms;
    }
    e->upd_launches += real;
    return done;
}
// Pivots enqueued in chunks, the device state polled once per chunk (the GPU never waits for the host inside a chunk), the chunk doubled up to
// `chunk_cap`, until the state leaves ST_RUNNING.  k == nullptr: k_select + k_update per pivot, the state is slot 0's; else one launch of the fused
// kernel k per pivot, numbered by *launch, the state the pipeline's own (f->fst).  `timed`: an event pair around every k_update / fused launch
static int stream_pivots(jslp_engine* e, const SolveRun& p, const FusedKernel* k, const FusedCtx* f, int* launch, int chunk, int chunk_cap, bool timed, long long done_prev) {
    hipStream_t s = e->res.stream;
    for (;;) {
        if (timed) JSLP_TRY(ensure_events(e, 2 * (size_t)chunk));
        for (int i = 0; i < chunk; i++) {
            if (!k) hipLaunchKernelGGL(k_select, dim3(1), dim3(JSLP_WG_THREADS), 0, s, p.c);
            if (timed) HIPC(hipEventRecord(e->ev_pool[2 * i], s));
            if (k) launch_fused(e, *k, *f, (*launch)++);
            else hipLaunchKernelGGL(k_update, p.grid, dim3(JSLP_UPD_THREADS), 0, s, p.c);
            if (timed) HIPC(hipEventRecord(e->ev_pool[2 * i + 1], s));
        }
        HIPC(hipGetLastError());
        JSLP_TRY(fetch_state(e, k ? f->fst[*launch & 1] : e->s.st));
        if (timed) done_prev = account_chunk_time(e, chunk, done_prev);
        if (e->h_state->status != ST_RUNNING) return JSLP_OK;
        chunk = std::min(chunk * 2, chunk_cap);
    }
}
// the ONE pivot a fused pipeline cannot decide alone (ST_P1_SLOW, see k_fused_p1 / k_pivot_fused): through k_select + k_update
static int slow_pivot(jslp_engine* e, const SolveRun& p) {
    hipStream_t s = e->res.stream;
    hipLaunchKernelGGL(k_p1_resume, dim3(1), dim3(1), 0, s, e->s.st, (int)ST_RUNNING);
    hipLaunchKernelGGL(k_select, dim3(1), dim3(JSLP_WG_THREADS), 0, s, p.c);
    hipLaunchKernelGGL(k_update, p.grid, dim3(JSLP_UPD_THREADS), 0, s, p.c);
    HIPC(hipGetLastError());
    JSLP_TRY(fetch_state(e, e->s.st));
    e->p1_slow_pivots += 1;
    return JSLP_OK;
}
// phase 1 through the fused pipeline (one launch per pivot; k_fused_p1); hands over with ST_PHASE1_DONE.  `done`: pivots the solve had done before
static int fused_phase1(jslp_engine* e, const SolveRun& p, long long done) {
    JSLP_TRY(ensure_fused(e));
    JSLP_TRY(ensure_fused_oo(e));
    const FusedCtx f = make_fused_ctx(e, p.c, p.H);
    const FusedKernel& k = fused_p1_kernel(e);
    if (p.dbg) fprintf(stderr, "[jslp] launch %s\n", k.name);
    for (;;) {
        int launch = 0;
        launch_fused(e, k, f, launch++);
        JSLP_TRY(stream_pivots(e, p, &k, &f, &launch, 2, 512, false, 0));
        hipLaunchKernelGGL(k_fused_finish, dim3(512), dim3(256), 0, e->res.stream, f, launch - 1);  // state -> slot 0's, tableau -> buf[0]
        HIPC(hipGetLastError());
        count_dense(e, p.H, pivots_done(e) - done);  // this run of the pipeline (the state stream_pivots fetched is the pipeline's last)
        if (e->h_state->status != ST_P1_SLOW) break;
        JSLP_TRY(slow_pivot(e, p));  // ... then the pipeline again (k_select counted that pivot on the device)
        done = pivots_done(e);
        if (e->h_state->status != ST_RUNNING) break;
    }
    e->last_path = "fused";
    return JSLP_OK;
}
// phase 1 (and phase 2 when the fused pipeline does not apply): k_select + k_update per pivot
static int select_update_loop(jslp_engine* e, const SolveRun& p) {
    if (p.dbg) fprintf(stderr, "[jslp] launch select+update\n");
    return stream_pivots(e, p, nullptr, nullptr, nullptr, p.fused ? 1 : 8, 256, e->timing && !p.fused, 0);
}
// phase 2: one fused launch per pivot (k_pivot_fused)
static int fused_phase2(jslp_engine* e, const SolveRun& p) {
    hipStream_t s = e->res.stream;
    while (e->h_state->status == ST_PHASE1_DONE) {
        JSLP_TRY(ensure_fused(e));
        JSLP_TRY(ensure_fused_oo(e));
        e->last_path = "fused";
        const FusedCtx f = make_fused_ctx(e, p.c, p.H);
        const FusedKernel& k = pivot_fused_kernel(e);
        if (p.dbg) fprintf(stderr, "[jslp] launch %s\n", k.name);
        int launch = 0;
        const long long done = pivots_done(e);  // (e->h_state is current here: every way into this loop ends with a fetch of the state)
        launch_fused(e, k, f, launch++);
        JSLP_TRY(stream_pivots(e, p, &k, &f, &launch, 16, 512, e->timing != 0, done));
        hipLaunchKernelGGL(k_fused_finish, dim3(512), dim3(256), 0, s, f, launch - 1);
        HIPC(hipGetLastError());
        count_dense(e, p.H, pivots_done(e) - done);  // this run of the pipeline, not the pivot it hands over below
        if (e->h_state->status == ST_P1_SLOW) {
            // an entering column named by an optional objective with a ~0 main cost and a tiny pivot-row entry: that ONE pivot
            // through k_select + k_update (see k_pivot_fused), then the pipeline again from its first launch
            JSLP_TRY(slow_pivot(e, p));
            if (e->h_state->status != ST_RUNNING) break;  // that pivot ended the solve
            hipLaunchKernelGGL(k_p1_resume, dim3(1), dim3(1), 0, s, e->s.st, (int)ST_PHASE1_DONE);
            e->h_state->status = ST_PHASE1_DONE;
            continue;
        }
        JSLP_TRY(fetch_state(e, e->s.st));  // the solve's final state, as k_fused_finish adopted it (waited for: close_solve reads it)
        break;
    }
    return JSLP_OK;
}
// the closing events; e->h_state is the solve's final state
static int close_solve(jslp_engine* e) {
    HIPC(hipEventRecord(e->res.ev_end, e->res.stream));
    HIPC(hipStreamSynchronize(e->res.stream));
    float ms = 0;
    if (e->timing && hipEventElapsedTime(&ms, e->res.ev_begin, e->res.ev_end) == hipSuccess) e->total_ms += ms;
    return state_error(*e->h_state);
}

// simplex() of the live tableau (slot 0), leaving the final DevState in e->h_state
static int run_simplex(jslp_engine* e, int check_cycles) {
    e->slot0_synced = 0;  // the chip-wide kernels do not maintain the dirty-row flags (k_begin zeroes st.gen)
    e->abort_injected = 0;
    HIPC(hipEventRecord(e->res.ev_begin, e->res.stream));
    if (use_wg_single(e)) {
        JSLP_TRY(solve_one_workgroup(e, check_cycles));
        return close_solve(e);
    }
    SolveRun p;
    JSLP_TRY(plan_solve(e, check_cycles, &p));
    hipLaunchKernelGGL(k_begin, dim3(1), dim3(1), 0, e->res.stream, e->s, 0, p.cap);
    Resident res = Resident::NotTried;
    if (p.geometry != 0 && !p.phase2_only) JSLP_TRY(resident_attempt(e, p, 0, &res));
    if (res != Resident::Done) {
        // (a lean kernel that left mid-solve may have left behind phase 1: h_state is current in that case only)
        bool phase1_over = res == Resident::Streaming && e->h_state->status == ST_PHASE1_DONE;
        if (!phase1_over && p.fused && fused_p1_on()) {
            // (h_state is the solve's only behind a launch that ran: before that it still holds what plan_solve read in front of k_begin)
            JSLP_TRY(fused_phase1(e, p, res == Resident::Streaming || res == Resident::RolledBack ? pivots_done(e) : 0));
            phase1_over = true;
        }
        if (!phase1_over) JSLP_TRY(select_update_loop(e, p));
        // phase 2 of the tall / wide geometries: register-resident (plan_solve)
        if (p.phase2_only && e->h_state->status == ST_PHASE1_DONE && e->h_state->err == ERR_NONE)
            JSLP_TRY(resident_attempt(e, p, (long long)e->h_state->it1 + e->h_state->it2, &res));
        if (res != Resident::Done) JSLP_TRY(fused_phase2(e, p));
    }
    return close_solve(e);
}

extern "C" int jslp_engine_simplex(jslp_engine* e, int check_cycles, jslp_simplex_result* out) {
    if (!e || !out) return fail(JSLP_ERR_ARG, "simplex: null pointer");
    if (!e->uploaded) return fail(JSLP_ERR_STATE, "simplex before upload");
    HIPC(hipSetDevice(e->device));
    int rc = run_simplex(e, check_cycles);
    if (rc) return rc;
    account(e, *e->h_state, 0);
    return fill_result(e, *e->h_state, 0, e->evaluation, out, &e->evaluation);
}

extern "C" int jslp_engine_pivot(jslp_engine* e, int32_t row, int32_t col) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "pivot before upload");
    HIPC(hipSetDevice(e->device));
    hipStream_t s = e->res.stream;
    HIPC(hipMemcpyAsync(e->h_state, e->s.st, sizeof(DevState), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    const int H = e->h_state->H;
    if (row < 0 || row >= H || col < 0 || col >= e->W) return fail(JSLP_ERR_ARG, "pivot: index out of range");
    e->slot0_synced = 0;  // k_prepare zeroes st.gen
    const Ctx c = host_ctx(e, 0);
    hipLaunchKernelGGL(k_prepare, dim3(1), dim3(JSLP_WG_THREADS), 0, s, c, (int)row, (int)col);
    hipLaunchKernelGGL(k_update, update_grid(e, H), dim3(JSLP_UPD_THREADS), 0, s, c);
    hipLaunchKernelGGL(k_end_pivot, dim3(1), dim3(1), 0, s, c);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    return JSLP_OK;
}

static dim3 copy_grid(const jslp_engine* e, int slots) {
    const long long n2 = (long long)e->cap_rows * e->ld / 2;
    long long bx = std::max<long long>(8, std::min<long long>(256, 4096 / std::max(1, slots)));
    bx = std::min<long long>(bx, (n2 + 255) / 256);
    return dim3((unsigned)std::max<long long>(bx, 1), slots, 1);
}

// the saved root once more, column-major, for the node kernels' pivot-column reads (WgLds::snapT)
static void launch_snapshot_transpose(jslp_engine* e) {
    if (!e->snap_AT) return;
    hipLaunchKernelGGL(k_snapshot_transpose, dim3((e->W + 31) / 32, (e->cap_rows + 31) / 32), dim3(256), 0, e->res.stream, e->s.st, e->snap_A,
                       (int)e->ld, (int)e->W, e->snap_AT, e->snap_ldT);
}
static Snapshot root_snapshot(const jslp_engine* e) {
    return Snapshot{e->snap_A, e->snap_vibr, e->snap_vibc, e->snap_rbv, e->snap_cbv, e->n_idx, e->snap_oo, -1, 0, e->snap_rhs,
                    snapshot_transpose_on() ? e->snap_AT : nullptr, e->snap_ldT};
}

extern "C" int jslp_engine_save(jslp_engine* e) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "save before upload");
    HIPC(hipSetDevice(e->device));
    SnapshotW w{e->snap_A, e->snap_vibr, e->snap_vibc, e->snap_rbv, e->snap_cbv, e->n_idx, e->snap_oo, e->snap_rhs};
    e->slot0_synced = 0;  // new snapshot generation
    e->slots_synced = 0;
    hipLaunchKernelGGL(k_save, dim3(copy_grid(e, 1).x), dim3(256), 0, e->res.stream, e->s, w);
    launch_snapshot_transpose(e);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(e->res.stream));
    e->has_save = 1;
    e->root_seq += 1;
    return JSLP_OK;
}

// restore slots [first_slot, first_slot + n) from the saved root (checkpoint < 0) or from a checkpoint
static int enqueue_restore(jslp_engine* e, int first_slot, int n, int checkpoint = -1) {
    if (first_slot == 0) {
        if (checkpoint < 0 && e->has_save) {
            e->slot0_synced = 1;
            e->slots_synced = std::max(e->slots_synced, n);
        } else {
            e->slot0_synced = 0;
            if (checkpoint >= 0) e->slots_synced = 0;  // these slots now hold a checkpoint, not the snapshot
        }
    }
    if (checkpoint < 0) {
        if (!e->has_save) return JSLP_OK;  // backup.ts:54-56
        Snapshot sn = root_snapshot(e);
        hipLaunchKernelGGL(k_restore, copy_grid(e, n), dim3(256), 0, e->res.stream, e->s, sn, first_slot);
    } else {
        const jslp_engine::Ckpt& c = e->ckpts[checkpoint];
        Snapshot sn{c.A, c.vibr, c.vibc, c.rbv, c.cbv, e->n_idx, nullptr, c.H, c.last_element_index, c.rhs};
        hipLaunchKernelGGL(k_restore, copy_grid(e, n), dim3(256), 0, e->res.stream, e->s, sn, first_slot);
    }
    hipLaunchKernelGGL(k_restore_commit, dim3(n), dim3(1), 0, e->res.stream, e->s, first_slot, checkpoint < 0 ? 1 : 0);
    HIPC(hipGetLastError());
    return JSLP_OK;
}

static int checkpoint_check(const jslp_engine* e, int32_t id, const char* who) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "%s%s", who, ": before upload");
    if (id < 0 || id >= (int32_t)e->ckpts.size() || !e->ckpts[id].live) return fail(JSLP_ERR_ARG, "%s%s", who, ": no such checkpoint");
    return JSLP_OK;
}

extern "C" int jslp_engine_checkpoint_create(jslp_engine* e, int32_t* id_out) {
    if (!e || !id_out) return fail(JSLP_ERR_ARG, "checkpoint_create: null pointer");
    if (!e->uploaded) return fail(JSLP_ERR_STATE, "checkpoint_create before upload");
    HIPC(hipSetDevice(e->device));
    // height / lastElementIndex of the live tableau
    HIPC(hipMemcpyAsync(e->h_state, e->s.st, sizeof(DevState), hipMemcpyDeviceToHost, e->res.stream));
    HIPC(hipStreamSynchronize(e->res.stream));
    jslp_engine::Ckpt c;
    if (!e->ck_free.empty()) {  // every buffer is sized for the row capacity, so freed ones fit any later checkpoint
        c.mem = std::move(e->ck_free.back());
        e->ck_free.pop_back();
    }
    const hipError_t err = carve_into(c.mem, [&](Carver& cv) {
        c.A = cv.take<double>((size_t)e->cap_rows * e->ld);
        c.rhs = cv.take<double>((size_t)e->cap_rows);
        c.vibr = cv.take<int32_t>((size_t)e->cap_rows);
        c.vibc = cv.take<int32_t>((size_t)e->W);
        c.rbv = cv.take<int32_t>((size_t)e->n_idx);
        c.cbv = cv.take<int32_t>((size_t)e->n_idx);
    });
    if (err != hipSuccess) {
        (void)hipGetLastError();
        return fail(JSLP_ERR_NOMEM, "checkpoint_create: out of device memory");
    }
    c.H = e->h_state->H;
    c.last_element_index = e->h_state->last_element_index;
    c.evaluation = e->evaluation;
    c.live = 1;
    SnapshotW w{c.A, c.vibr, c.vibc, c.rbv, c.cbv, e->n_idx, nullptr, c.rhs};
    hipLaunchKernelGGL(k_checkpoint, dim3(copy_grid(e, 1).x), dim3(256), 0, e->res.stream, e->s, w, (int)c.H);
    HIPC(hipGetLastError());
    int32_t id = -1;
    for (size_t i = 0; i < e->ckpts.size(); i++)
        if (!e->ckpts[i].live) { id = (int32_t)i; break; }
    if (id < 0) { id = (int32_t)e->ckpts.size(); e->ckpts.push_back(std::move(c)); } else e->ckpts[id] = std::move(c);
    *id_out = id;
    return JSLP_OK;  // stream-ordered: no synchronisation needed before the next engine call
}

extern "C" int jslp_engine_checkpoint_restore(jslp_engine* e, int32_t id) {
    int rc = checkpoint_check(e, id, "checkpoint_restore");
    if (rc) return rc;
    HIPC(hipSetDevice(e->device));
    rc = enqueue_restore(e, 0, 1, id);
    if (rc) return rc;
    HIPC(hipStreamSynchronize(e->res.stream));
    e->evaluation = e->ckpts[id].evaluation;  // incremental-branch-and-cut.ts:105
    return JSLP_OK;
}

extern "C" int jslp_engine_checkpoint_release(jslp_engine* e, int32_t id) {
    int rc = checkpoint_check(e, id, "checkpoint_release");
    if (rc) return rc;
    HIPC(hipSetDevice(e->device));
    HIPC(hipStreamSynchronize(e->res.stream));  // a restore from it may still be in flight
    e->ck_free.push_back(std::move(e->ckpts[id].mem));
    e->ckpts[id] = jslp_engine::Ckpt();
    return JSLP_OK;
}

extern "C" int jslp_engine_restore(jslp_engine* e) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "restore before upload");
    HIPC(hipSetDevice(e->device));
    int rc = enqueue_restore(e, 0, 1);
    if (rc) return rc;
    HIPC(hipStreamSynchronize(e->res.stream));
    return JSLP_OK;
}

// stage the cut lists of n_nodes nodes on the device: packed into one pinned buffer, one async copy, no sync
// (the pinned buffer is reused only after the call's final stream synchronisation)
static int upload_cuts(jslp_engine* e, int32_t n_nodes, const int32_t* offs, const int8_t* type, const int32_t* var,
                       const double* value, bool to_device = true) {
    if (offs[0] != 0) return fail(JSLP_ERR_ARG, "cuts: cut_offsets[0] must be 0");
    for (int32_t i = 0; i < n_nodes; i++)
        if (offs[i + 1] < offs[i]) return fail(JSLP_ERR_ARG, "cuts: cut_offsets must not decrease");
    const size_t C = (size_t)offs[n_nodes], N1 = (size_t)n_nodes + 1;
    if (C > 0 && (!type || !var || !value)) return fail(JSLP_ERR_ARG, "cuts: null pointer");
    // [values | offsets | variables | types | hand-out order of a batch | its queue counter (0)]
    const size_t off_offs = 8 * C, off_var = off_offs + 4 * N1, off_type = off_var + 4 * C, off_order = (off_type + C + 3) & ~(size_t)3,
                 off_queue = off_order + 4 * (size_t)n_nodes, total = off_queue + 4;
    if (total > e->res.cuts.bytes()) {  // grow: the old pair goes only when both new halves exist
        HIPC(hipStreamSynchronize(e->res.stream));  // nothing in flight may still read the old pair
        bool pinned = false;
        if (e->res.cuts.reserve(std::max<size_t>(2 * total, 4096), &pinned) != hipSuccess) {
            (void)hipGetLastError();
            return fail(JSLP_ERR_NOMEM, pinned ? "cuts: out of pinned memory" : "cuts: out of device memory");
        }
    }
    if (C) memcpy(e->res.cuts.h.p, value, 8 * C);
    memcpy(e->res.cuts.h.p + off_offs, offs, 4 * N1);
    if (C) { memcpy(e->res.cuts.h.p + off_var, var, 4 * C); memcpy(e->res.cuts.h.p + off_type, type, C); }
    if (node_queue() == 2) {  // most cuts first (a counting sort, stable): k_node_queue hands the nodes out in this order
        int32_t* order = reinterpret_cast<int32_t*>(e->res.cuts.h.p + off_order);
        int most = 0;
        for (int32_t i = 0; i < n_nodes; i++) most = std::max(most, (int)(offs[i + 1] - offs[i]));
        std::vector<int32_t>& start = e->order_scratch;
        start.assign((size_t)most + 2, 0);
        for (int32_t i = 0; i < n_nodes; i++) start[(size_t)(most - (offs[i + 1] - offs[i])) + 1]++;
        for (int c = 0; c <= most; c++) start[(size_t)c + 1] += start[c];
        for (int32_t i = 0; i < n_nodes; i++) order[start[(size_t)(most - (offs[i + 1] - offs[i]))]++] = i;
    }
    *reinterpret_cast<int32_t*>(e->res.cuts.h.p + off_queue) = 0;
    // to_device == false: the one-launch node kernel reads the (tiny) cut list straight from the pinned buffer
    char* base = e->res.cuts.d.p;
    if (to_device) {
        HIPC(hipMemcpyAsync(e->res.cuts.d.p, e->res.cuts.h.p, total, hipMemcpyHostToDevice, e->res.stream));
    } else {
        void* dev = nullptr;
        HIPC(hipHostGetDevicePointer(&dev, e->res.cuts.h.p, 0));
        base = static_cast<char*>(dev);
    }
    e->d_cut_val = reinterpret_cast<double*>(base);
    e->d_cut_offs = reinterpret_cast<int32_t*>(base + off_offs);
    e->d_cut_var = reinterpret_cast<int32_t*>(base + off_var);
    e->d_cut_type = reinterpret_cast<int8_t*>(base + off_type);
    e->d_cut_order = reinterpret_cast<int32_t*>(base + off_order);
    e->d_queue = reinterpret_cast<int*>(base + off_queue);
    return JSLP_OK;
}

extern "C" int jslp_engine_add_cuts(jslp_engine* e, int32_t n, const int8_t* type, const int32_t* var_index,
                                    const double* value) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "add_cuts before upload");
    if (n < 0) return fail(JSLP_ERR_ARG, "add_cuts: negative count");
    HIPC(hipSetDevice(e->device));
    const int32_t offs[2] = {0, n};
    int rc = upload_cuts(e, 1, offs, type, var_index, value);
    if (rc) return rc;
    if (e->counting) e->wc.cut_rows += n;
    Cuts cu{e->d_cut_offs, e->d_cut_type, e->d_cut_var, e->d_cut_val};
    hipLaunchKernelGGL(k_add_cuts, dim3(1), dim3(256), 0, e->res.stream, e->s, cu, 0, 0, (int)e->cap_rows);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(e->h_state, e->s.st, sizeof(DevState), hipMemcpyDeviceToHost, e->res.stream));
    HIPC(hipStreamSynchronize(e->res.stream));
    return state_error(*e->h_state);
}

// read-back buffers for `nodes` nodes laid out [states | rhs | rows] so that one copy brings a group back
static size_t out_bytes(const jslp_engine* e, size_t nodes) {
    return nodes * (sizeof(DevState) + (((size_t)e->cap_rows + 3) & ~(size_t)3) * 12) + 192;
}
// rows per node in the engine's own read-back buffers: a multiple of 4, so that every node's slice starts 16-byte aligned and
// the kernels write it with 8/16-byte stores per lane (4-byte stores into pinned host memory cost the Monster_II batch a
// quarter of its time); the device pool lays its shared buffer out itself, with the plain row capacity
struct PinnedDest { DevState* states = nullptr; double* rhs = nullptr; int32_t* rows = nullptr; };  // a range of the device pool's shared pinned buffer
static size_t out_stride_of(const jslp_engine* e, const PinnedDest& shared = {}) {
    return shared.states ? (size_t)e->cap_rows : (((size_t)e->cap_rows + 3) & ~(size_t)3);
}
static void out_layout(jslp_engine* e, size_t nodes, const PinnedDest& shared) {
    const size_t stride = out_stride_of(e, shared);
    const size_t o_rhs = (nodes * sizeof(DevState) + 63) & ~(size_t)63, o_rows = (o_rhs + nodes * stride * 8 + 63) & ~(size_t)63;
    e->d_states = reinterpret_cast<DevState*>(e->res.out.d.p);
    e->d_rhs = reinterpret_cast<double*>(e->res.out.d.p + o_rhs);
    e->d_rows = reinterpret_cast<int32_t*>(e->res.out.d.p + o_rows);
    e->h_states = reinterpret_cast<DevState*>(e->res.out.h.p);
    e->h_rhs = reinterpret_cast<double*>(e->res.out.h.p + o_rhs);
    e->h_rows = reinterpret_cast<int32_t*>(e->res.out.h.p + o_rows);
    if (shared.states) {  // device pool: this call's outcomes go straight into the pool's pinned buffer
        e->h_states = shared.states; e->h_rhs = shared.rhs; e->h_rows = shared.rows;
    }
}
static int ensure_out(jslp_engine* e, size_t nodes, const PinnedDest& shared = {}) {
    if (out_bytes(e, nodes) > e->res.out.bytes()) HIPC(e->res.out.reserve(out_bytes(e, std::max<size_t>(nodes, 16))));
    out_layout(e, nodes, shared);
    return JSLP_OK;
}

extern "C" int jslp_engine_read_rhs(jslp_engine* e, double* rhs, int32_t* var_index_by_row) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "read_rhs before upload");
    HIPC(hipSetDevice(e->device));
    int rc = ensure_out(e, 1);
    if (rc) return rc;
    hipStream_t s = e->res.stream;
    hipLaunchKernelGGL(k_gather, dim3(1), dim3(256), 0, s, e->s, 0, e->d_rhs, e->d_rows, e->d_states, (int)e->cap_rows, 0);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(e->res.out.h.p, e->res.out.d.p, out_bytes(e, 1), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    const int H = e->h_states[0].H;
    if (rhs) memcpy(rhs, e->h_rhs, sizeof(double) * H);
    if (var_index_by_row) memcpy(var_index_by_row, e->h_rows, sizeof(int32_t) * H);
    return JSLP_OK;
}

extern "C" int jslp_engine_set_integer_variables(jslp_engine* e, const int32_t* var_indexes, int32_t n) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "set_integer_variables before upload");
    if (n < 0 || (n > 0 && !var_indexes)) return fail(JSLP_ERR_ARG, "set_integer_variables: bad arguments");
    HIPC(hipSetDevice(e->device));
    std::vector<uint8_t> flags(e->n_idx, 0);
    for (int32_t i = 0; i < n; i++) {
        if (var_indexes[i] < 0 || var_indexes[i] >= e->n_idx) return fail(JSLP_ERR_ARG, "set_integer_variables: index out of range");
        flags[var_indexes[i]] = 1;
    }
    HIPC(hipMemcpyAsync(e->d_isint, flags.data(), e->n_idx, hipMemcpyHostToDevice, e->res.stream));
    HIPC(hipStreamSynchronize(e->res.stream));
    e->has_int = n > 0;
    return JSLP_OK;
}

// Tableau.applyMIRCuts() (cutting-strategies.ts:199-212)
extern "C" int jslp_engine_apply_mir_cuts(jslp_engine* e, int32_t* n_added) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "apply_mir_cuts before upload");
    HIPC(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_mir_cuts, dim3(1), dim3(256), 0, e->res.stream, e->s, e->d_isint, 10, (int)e->cap_rows);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(e->h_state, e->s.st, sizeof(DevState), hipMemcpyDeviceToHost, e->res.stream));
    HIPC(hipStreamSynchronize(e->res.stream));
    int rc = state_error(*e->h_state);
    if (rc) return rc;
    if (n_added) *n_added = e->h_state->mir_added;
    return JSLP_OK;
}

extern "C" int jslp_engine_mir_round(jslp_engine* e, int check_cycles, int32_t* n_added, jslp_simplex_result* out,
                                     double* rhs, int32_t* var_index_by_row) {
    int rc = jslp_engine_apply_mir_cuts(e, n_added);
    if (rc) return rc;
    rc = jslp_engine_simplex(e, check_cycles, out);
    if (rc) return rc;
    return jslp_engine_read_rhs(e, rhs, var_index_by_row);
}

// ---- fp32 twin -----------------------------------------------------------------------------------------------------
// the fp32 arena holds `n` copies (copy 0: what jslp_engine_simplex_f32 runs on; copies 0 .. n-1: the runs of a one-launch sweep,
// include/jslpf_f32.h).  It only grows, into a fresh allocation: a failed reservation leaves the old arena and its slots in place
static int ensure_f32(jslp_engine* e, int32_t n = 1) {
    if (e->arena32.p && n <= e->n32) return JSLP_OK;
    f32::Slots s = e->s32;
    s.A_stride = (long long)e->cap_rows * e->ld;
    s.vibr_stride = e->cap_rows; s.vibc_stride = e->W; s.idx_stride = e->n_idx;
    s.prow_stride = e->ld; s.pcol_stride = e->cap_rows;
    s.hist_cap = (int32_t)HIST_CAP_SLOT;
    s.ld = e->ld; s.W = e->W; s.batch = e->batch; s.use_partial = e->use_partial;
    s.oo = nullptr; s.oo_stride = 0; s.n_opt = 0;
    s.rhs = nullptr;
    s.trace = nullptr; s.trace_cap = 0;
    const size_t copies = (size_t)n;
    DevBuf grown;
    HIPC_CARVE(grown, [&](Carver& cv) {
        s.A = cv.take<float>(copies * (size_t)s.A_stride);
        s.vibr = cv.take<int32_t>(copies * (size_t)s.vibr_stride);
        s.vibc = cv.take<int32_t>(copies * (size_t)s.vibc_stride);
        s.rbv = cv.take<int32_t>(copies * (size_t)s.idx_stride);
        s.cbv = cv.take<int32_t>(copies * (size_t)s.idx_stride);
        s.prow = cv.take<float>((size_t)s.prow_stride);  // (the select + update kernels' vectors: copy 0 only)
        s.pcol = cv.take<float>((size_t)s.pcol_stride);
        s.dirty = cv.take<uint8_t>((size_t)s.pcol_stride);
        s.st = cv.take<DevState>(copies);
        s.hist = cv.take<int2>(copies * (size_t)s.hist_cap);
    });
    HIPC(hipStreamSynchronize(e->res.stream));  // nothing in flight reads the old arena
    e->arena32 = std::move(grown);
    e->s32 = s;
    e->n32 = n;
    HIPC(hipMemsetAsync(s.A, 0, sizeof(float) * copies * (size_t)s.A_stride, e->res.stream));  // padding columns / rows stay 0
    return JSLP_OK;
}

extern "C" int jslp_engine_simplex_f32(jslp_engine* e, double precision, int check_cycles, jslp_simplex_result* out,
                                       double* rhs, int32_t* var_index_by_row, double* device_ms) {
    if (!e || !out) return fail(JSLP_ERR_ARG, "simplex_f32: null pointer");
    if (!e->uploaded) return fail(JSLP_ERR_STATE, "simplex_f32 before upload");
    if (e->n_opt > 0) return fail(JSLP_ERR_UNSUPPORTED, "simplex_f32: optional objectives are not part of the fp32 experiment");
    if (!(precision > 0)) return fail(JSLP_ERR_ARG, "simplex_f32: precision must be positive");
    HIPC(hipSetDevice(e->device));
    int rc = ensure_f32(e);
    if (rc) return rc;
    rc = ensure_out(e, 1);
    if (rc) return rc;
    hipStream_t s = e->res.stream;
    f32::Slots& d = e->s32;
    d.unr = e->d_unr;
    d.has_unr = e->n_unr > 0 ? 1 : 0;
    d.precision = (float)precision;
    hipLaunchKernelGGL(k32_convert, dim3(copy_grid(e, 1).x), dim3(256), 0, s, e->s, d, 0);
    hipLaunchKernelGGL(f32::k_begin, dim3(1), dim3(1), 0, s, d, 0, iters_cap(e));
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(e->h_state, d.st, sizeof(DevState), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    const int H = e->h_state->H;
    f32::Ctx c{};  // (cnt = nullptr: the fp32 experiment is not counted)
    c.A = d.A; c.vibr = d.vibr; c.vibc = d.vibc; c.rbv = d.rbv; c.cbv = d.cbv; c.unr = d.unr;
    c.prow = d.prow; c.pcol = d.pcol; c.dirty = d.dirty; c.rhs = nullptr; c.oo = nullptr; c.n_opt = 0; c.st = d.st; c.hist = d.hist;
    c.hist_cap = d.hist_cap; c.trace = nullptr; c.trace_cap = 0; c.ld = e->ld; c.W = e->W; c.check_cycles = check_cycles;
    c.batch = e->batch; c.use_partial = e->use_partial; c.precision = (float)precision; c.stop_at_phase2 = 0;
    c.has_unr = d.has_unr;
    const dim3 grid = update_grid(e, H);
    HIPC(hipEventRecord(e->res.ev_begin, s));
    for (int chunk = 8;; chunk = std::min(chunk * 2, 256)) {
        for (int i = 0; i < chunk; i++) {
            hipLaunchKernelGGL(f32::k_select, dim3(1), dim3(JSLP_WG_THREADS), 0, s, c);
            hipLaunchKernelGGL(f32::k_update, grid, dim3(JSLP_UPD_THREADS), 0, s, c);
        }
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(e->h_state, d.st, sizeof(DevState), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        if (e->h_state->status != ST_RUNNING) break;
    }
    HIPC(hipEventRecord(e->res.ev_end, s));
    hipLaunchKernelGGL(k32_gather, dim3(1), dim3(256), 0, s, d, e->d_rhs, e->d_rows, e->d_states);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(e->res.out.h.p, e->res.out.d.p, out_bytes(e, 1), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    const DevState st = e->h_states[0];
    rc = state_error(st);
    if (rc) return rc;
    if (device_ms) {
        float ms = 0;
        *device_ms = hipEventElapsedTime(&ms, e->res.ev_begin, e->res.ev_end) == hipSuccess ? ms : -1.0;
    }
    memset(out, 0, sizeof *out);
    out->feasible = st.feasible;
    out->bounded = st.bounded;
    out->optimal = st.optimal;
    out->unbounded_var_index = st.bounded ? -1 : st.unbounded_var;
    out->pivots_phase1 = st.it1;
    out->pivots_phase2 = st.entered_phase2 ? st.it2 : -1;
    out->cycle_phase = st.cycle_phase;
    out->height = st.H;
    out->obj_cell = st.obj_cell;
    out->evaluation = e->evaluation;
    if (st.optimal) {
        const double rcoef = js_round(1.0 / precision);
        out->evaluation = js_round((2.220446049250313e-16 + st.obj_cell) * rcoef) / rcoef;
    } else if (!st.bounded) {
        out->evaluation = -INFINITY;
    }
    if (rhs) memcpy(rhs, e->h_rhs, sizeof(double) * st.H);
    if (var_index_by_row) memcpy(var_index_by_row, e->h_rows, sizeof(int32_t) * st.H);
    return JSLP_OK;
}

// ---- node relaxation: restore + cuts + simplex + gather for a batch of nodes -------------------------------------------------------
// What a caller asks of relax_batch_impl.  Every entry point fills one of these with named fields.
// Full: the whole RHS column / row map of every node; Watched: the watched variables' rows / RHS cells only; BranchRecord (include/jslpx_branch.h):
// the node kernels' compact (watched) read-back stays in device memory and k_branch_record reduces it to 32 bytes per node
enum class ReadBack { Full, Watched, BranchRecord };
struct CutLists {  // node i adds the cuts [offsets[i], offsets[i + 1])
    int32_t n_nodes = 0; const int32_t* offsets = nullptr; const int8_t* type = nullptr; const int32_t* var_index = nullptr; const double* value = nullptr;
};
struct DeviceDest {  // the caller's DEVICE memory takes the outcomes (no host copy at all): `states` set = this destination
    DevState* states = nullptr; double* rhs = nullptr; int32_t* rows = nullptr;
    int32_t stride = 0; double* rec = nullptr;  // entries per node in rhs / rows; ReadBack::BranchRecord: where the records go
};
struct MirCall { int32_t max_rounds, need_feasible; jslpr_mir_outcome* outcomes; };  // (include/jslpr_mir.h)
struct NodeCall {
    CutLists cuts;
    int check_cycles = 0;
    int checkpoint = -1;  // the start: a checkpoint, or (-1) the saved root / the live tableau
    ReadBack read_back = ReadBack::Full;
    bool want_rhs = false, want_rows = false;
    // where the outcomes go, exactly one of three:
    jslp_simplex_result* out = nullptr;  // per-node results (1 and 2)
    double* rhs = nullptr; int32_t* var_index_by_row = nullptr; int32_t out_stride = 0;  // 1. the caller's host arrays
    bool pinned = false;                 // 2. the caller reads the engine's pinned buffers itself (no second host copy)
    PinnedDest shared;                   //    ... or, with `pinned`, the device pool's: this call's range of its shared pinned buffer
    DeviceDest dev;                      // 3. the caller's device memory
    const struct MirCall* mir = nullptr;  // jslpr_engine_relax_mir: every node runs its MIR loop inside the node kernel (one-launch shapes only)
    bool to_device() const { return dev.states != nullptr; }
    bool compact() const { return read_back != ReadBack::Full; }
    bool records() const { return read_back == ReadBack::BranchRecord; }
};

// ---- the node kernels: one descriptor per instantiation the node path can launch ---------------------------------------------------
struct NodeArgs {  // the union of what the node kernels take
    const Slots* s; Snapshot sn; Cuts cu;
    int check_cycles, iters_cap, cap_rows; double* rhs; int32_t* rows; DevState* states;
    int out_stride;  // gather mode: >= 0 = the whole RHS column / row map with this row stride; < 0 = the watched variables only
    int first = 0;   // k_node_lds / k_node_wg: first node of the launch = index of its outcome
    unsigned* done_flag = nullptr; unsigned done_seq = 0; int* done_count = nullptr;
    int n_nodes = -1; const int32_t* order = nullptr; int* queue = nullptr;  // k_node_queue (n_nodes: also the `n` of its debug line)
    MirJob mj{};  // the MIR builds (jslp_mir_kernels.hip.h)
};
struct NodeKernel {
    const char* name;       // the JSLP_DEBUG_LAUNCH line (tests/test_node_edges.py asserts every one)
    int threads; bool lds;  // lds: launched with the tableau's dynamic LDS (wglds_smem)
    void (*launch)(const NodeArgs&, int grid, size_t lds, hipStream_t); const void* fn;  // fn: for occupancy queries
};
// (a default argument does not travel through a function pointer: k_node_lds gets its done_count explicitly)
template <auto K, int T> static void launch_node_lds(const NodeArgs& a, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(K, dim3(grid), dim3(T), lds, s, *a.s, a.sn, a.cu, a.first, a.check_cycles, a.iters_cap, a.cap_rows, a.rhs, a.rows, a.states, a.out_stride, a.first, a.done_flag, a.done_seq, a.done_count);
}
template <auto K, int T> static void launch_node_wg(const NodeArgs& a, int grid, size_t, hipStream_t s) {
    hipLaunchKernelGGL(K, dim3(grid), dim3(T), 0, s, *a.s, a.sn, a.cu, a.first, a.check_cycles, a.iters_cap, a.cap_rows, a.rhs, a.rows, a.states, a.out_stride, a.first, a.done_flag, a.done_seq);
}
template <auto K, int T> static void launch_node_queue(const NodeArgs& a, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(K, dim3(grid), dim3(T), lds, s, *a.s, a.sn, a.cu, a.n_nodes, a.order, a.queue, a.check_cycles, a.iters_cap, a.cap_rows, a.rhs, a.rows, a.states, a.out_stride);
}
template <auto K, int T> static void launch_simplex_lds(const NodeArgs& a, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(K, dim3(grid), dim3(T), lds, s, *a.s, 0, a.check_cycles, a.iters_cap, a.cap_rows);
}
template <auto K, int T> static void launch_simplex_wg(const NodeArgs& a, int grid, size_t, hipStream_t s) {
    hipLaunchKernelGGL(K, dim3(grid), dim3(T), 0, s, *a.s, 0, a.check_cycles, a.iters_cap);
}
#define NODE_KERNEL(launcher, threads, lds, name, ...) \
    {name, threads, lds, launcher<&__VA_ARGS__, threads>, reinterpret_cast<const void*>(&__VA_ARGS__)}
// (the rows' order is the order the compiler instantiates the kernels in, and their code depends on it: k_simplex_wg<256,1024> came out with another register
//  allocation behind <512,2048> -- a new row goes where tools/asm_digest.py shows every kernel's assembly unchanged)
static const NodeKernel NODE_LDS_1024_OPT = NODE_KERNEL(launch_node_lds, 1024, true, "k_node_lds<1024,opt 1,cow 0>", k_node_lds<1024, true, false>);
static const NodeKernel NODE_LDS_1024_COW = NODE_KERNEL(launch_node_lds, 1024, true, "k_node_lds<1024,opt 0,cow 1>", k_node_lds<1024, false, true>);
static const NodeKernel NODE_LDS_1024 = NODE_KERNEL(launch_node_lds, 1024, true, "k_node_lds<1024,opt 0,cow 0>", k_node_lds<1024, false, false>);
static const NodeKernel NODE_WG_1024 = NODE_KERNEL(launch_node_wg, 1024, false, "k_node_wg<1024,4096>", k_node_wg<1024, 4096>);
static const NodeKernel NODE_QUEUE_OPT = NODE_KERNEL(launch_node_queue, 512, true, "k_node_queue<512,cow 0,opt 1>", k_node_queue<512, false, true>);
static const NodeKernel NODE_QUEUE_COW = NODE_KERNEL(launch_node_queue, 512, true, "k_node_queue<512,cow 1,opt 0>", k_node_queue<512, true, false>);
static const NodeKernel NODE_QUEUE = NODE_KERNEL(launch_node_queue, 512, true, "k_node_queue<512,cow 0,opt 0>", k_node_queue<512, false, false>);
static const NodeKernel NODE_LDS_512 = NODE_KERNEL(launch_node_lds, 512, true, "k_node_lds<512,opt 0,cow 0>", k_node_lds<512, false, false>);
static const NodeKernel NODE_WG_512 = NODE_KERNEL(launch_node_wg, 512, false, "k_node_wg<512,2048>", k_node_wg<512, 2048>);
// the eager groups: k_restore + k_add_cuts in front, k_gather behind
static const NodeKernel EAGER_LDS_1024_OPT = NODE_KERNEL(launch_simplex_lds, 1024, true, "restore+add_cuts+simplex+gather k_simplex_lds<1024,opt 1>", k_simplex_lds<1024, true>);
static const NodeKernel EAGER_LDS_1024 = NODE_KERNEL(launch_simplex_lds, 1024, true, "restore+add_cuts+simplex+gather k_simplex_lds<1024,opt 0>", k_simplex_lds<1024, false>);
static const NodeKernel EAGER_LDS_512 = NODE_KERNEL(launch_simplex_lds, 512, true, "restore+add_cuts+simplex+gather k_simplex_lds<512,opt 0>", k_simplex_lds<512, false>);
static const NodeKernel EAGER_WG_256 = NODE_KERNEL(launch_simplex_wg, 256, false, "restore+add_cuts+simplex+gather k_simplex_wg<256,1024>", k_simplex_wg<256, 1024>);
static const NodeKernel EAGER_WG_512 = NODE_KERNEL(launch_simplex_wg, 512, false, "restore+add_cuts+simplex+gather k_simplex_wg<512,2048>", k_simplex_wg<512, 2048>);
static const NodeKernel EAGER_WG_1024 = NODE_KERNEL(launch_simplex_wg, 1024, false, "restore+add_cuts+simplex+gather k_simplex_wg<1024,4096>", k_simplex_wg<1024, 4096>);
#undef NODE_KERNEL
// the MIR builds (include/jslpr_mir.h) live in a unit of their own (jslp_tu_mir.hip), which launches them by number: no row above moves
#ifdef JSLP_SPLIT_TU
extern "C" __attribute__((visibility("hidden"))) int jslpr_mir_launch_tu(int which, unsigned grid, size_t lds, const void* args, void* stream);
static int mir_launch(int which, unsigned grid, size_t lds, const MirLaunch& m, hipStream_t s) { return jslpr_mir_launch_tu(which, grid, lds, &m, s); }
#else
static int mir_launch_impl(int which, unsigned grid, size_t lds, const void* bytes, hipStream_t st);  // (jslp_mir_kernels.hip.h, at the end of this file)
static int mir_launch(int which, unsigned grid, size_t lds, const MirLaunch& m, hipStream_t s) { return mir_launch_impl(which, grid, lds, &m, s); }
#endif
template <int WHICH> static void launch_node_mir(const NodeArgs& a, int grid, size_t lds, hipStream_t s) {
    MirLaunch m{};
    m.s = *a.s; m.sn = a.sn; m.cu = a.cu; m.mj = a.mj;
    m.check_cycles = a.check_cycles; m.iters_cap = a.iters_cap; m.cap_rows = a.cap_rows;
    m.rhs = a.rhs; m.rows = a.rows; m.states = a.states; m.out_stride = a.out_stride; m.first = a.first;
    m.done_flag = a.done_flag; m.done_seq = a.done_seq; m.done_count = a.done_count;
    m.n_nodes = a.n_nodes; m.order = a.order; m.queue = a.queue;
    (void)mir_launch(WHICH, (unsigned)grid, lds, m, s);  // (the unit only peeks at the launch's error: hipGetLastError in launch_node_kernel takes and reports it)
}
static const NodeKernel NODE_LDS_1024_MIR = {"k_node_lds<1024,opt 0,cow 0,mir 1>", 1024, true, launch_node_mir<MIR_K_NODE_LDS_1024>, nullptr};
static const NodeKernel NODE_LDS_512_MIR = {"k_node_lds<512,opt 0,cow 0,mir 1>", 512, true, launch_node_mir<MIR_K_NODE_LDS_512>, nullptr};
static const NodeKernel NODE_QUEUE_MIR = {"k_node_queue<512,cow 0,opt 0,mir 1>", 512, true, launch_node_mir<MIR_K_NODE_QUEUE_512>, nullptr};
static_assert(JSLP_WG_THREADS == 1024, "the single-node shape of the table above");

// JSLP_DEBUG_LAUNCH: which node kernel a relax call launched, one parseable stderr line per launch (tests/test_node_edges.py)
static void debug_node_launch(const char* kernel, int grid, int n_nodes, size_t lds) {
    char tail[64] = "";
    if (n_nodes >= 0) snprintf(tail, sizeof tail, " n %d", n_nodes);
    if (lds) fprintf(stderr, "[jslp] launch %s g %d%s lds %zu\n", kernel, grid, tail, lds);
    else fprintf(stderr, "[jslp] launch %s g %d%s\n", kernel, grid, tail);
}
// the one place a node kernel is launched: its line (when asked for), the launch, the launch's error
static int launch_node_kernel(const NodeKernel& k, const NodeArgs& a, int grid, size_t lds, hipStream_t s, bool dbg) {
    if (!k.lds) lds = 0;
    if (dbg) debug_node_launch(k.name, grid, a.n_nodes, lds);
    k.launch(a, grid, lds, s);
    HIPC(hipGetLastError());
    return JSLP_OK;
}

// which kernel, from what the call site can observe (lds = wglds_smem(e): 0 = the tableau does not fit the LDS builds)
static const NodeKernel& single_node_kernel(const jslp_engine* e, size_t lds, bool mir = false) {
    if (mir) return NODE_LDS_1024_MIR;  // (eager start; mir_one_launch() has made sure of the LDS build)
    if (!lds) return NODE_WG_1024;
    if (e->s.n_opt > 0) return NODE_LDS_1024_OPT;
    return node_cow_single() ? NODE_LDS_1024_COW : NODE_LDS_1024;  // copy-on-write start, slot 0 made whole again behind the completion flag (jslp_wglds.hip.h)
}
static const NodeKernel& queue_kernel(const jslp_engine* e, bool mir = false) {
    if (mir) return NODE_QUEUE_MIR;
    if (e->s.n_opt > 0) return NODE_QUEUE_OPT;  // optional objectives: the OPT build (eager restores)
    return node_cow() ? NODE_QUEUE_COW : NODE_QUEUE;
}
// a one-group batch small enough for the 1024-thread latency shape (small_batch_1024): the only shape that can end in a polled completion flag
static bool small_batch_shape(const jslp_engine* e, size_t lds, int g) { return lds && e->s.n_opt == 0 && g <= small_batch_1024(); }
static const NodeKernel& group_kernel(const jslp_engine* e, size_t lds, int g, bool mir = false) {
    if (mir) return small_batch_shape(e, lds, g) ? NODE_LDS_1024_MIR : NODE_LDS_512_MIR;
    if (!lds) return NODE_WG_512;
    if (e->s.n_opt > 0) return NODE_LDS_1024_OPT;  // optional objectives: the 1024-thread build only, whatever the batch size
    if (small_batch_shape(e, lds, g)) return node_cow_small() && node_cow() ? NODE_LDS_1024_COW : NODE_LDS_1024;
    return NODE_LDS_512;
}
static const NodeKernel& eager_kernel(const jslp_engine* e, size_t lds, int g) {
    // one node: the 1024-thread latency shape; a batch: smaller workgroups, more nodes in flight per CU
    const bool opt = lds && e->s.n_opt > 0;
    const int shape = (g == 1 || opt) ? 1024 : wg_batch_threads();
    if (opt) return EAGER_LDS_1024_OPT;
    if (lds && shape == 1024) return EAGER_LDS_1024;
    if (lds && shape == 512) return EAGER_LDS_512;  // (no LDS build for 256 threads)
    if (shape == 256) return EAGER_WG_256;
    return shape == 512 ? EAGER_WG_512 : EAGER_WG_1024;
}

// ---- the completion flag: a node kernel's last act is a system-scope release store of a sequence number into pinned memory ------------
struct DoneFlag { unsigned* host = nullptr; unsigned* dev = nullptr; unsigned seq = 0; };
static hipError_t arm_done_flag(jslp_engine* e, DoneFlag* f) {
    unsigned* h_flag = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(e->h_state) + sizeof(DevState));
    void* flag_dev = nullptr;
    const hipError_t err = hipHostGetDevicePointer(&flag_dev, h_flag, 0);
    if (err != hipSuccess) return err;  // (no mapped pinned memory: the single child refuses, the batch ends with a stream synchronisation)
    const unsigned seq = ++e->done_seq ? e->done_seq : ++e->done_seq;  // never 0 (the flag's initial value)
    *f = DoneFlag{h_flag, static_cast<unsigned*>(flag_dev), seq};
    return hipSuccess;
}
// poll it (a stream synchronisation costs tens of microseconds of wake-up latency per node of a sequential tree walk); false after 5 s: a
// fault or a hang, and the caller synchronises the stream so that the runtime reports it
static bool wait_done_flag(const unsigned* h_flag, unsigned seq, unsigned& spins) {
    const auto t_begin = std::chrono::steady_clock::now();
    for (spins = 0; __atomic_load_n(h_flag, __ATOMIC_ACQUIRE) != seq;) {
        if ((++spins & 0x3fffu) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() > 5.0) return false;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    return true;
}
// JSLP_DEBUG_STALL: whether the time went in front of the wait (cut-list staging, the launch calls) or in it (the GPU side)
static void report_stall(int n_nodes, bool polled, std::chrono::steady_clock::time_point t_enter, std::chrono::steady_clock::time_point t_wait, unsigned spins) {
    const double host_ms = std::chrono::duration<double, std::milli>(t_wait - t_enter).count();
    const double wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_wait).count();
    if (!(host_ms + wait_ms > debug_stall_ms())) return;
    if (polled)
        fprintf(stderr, "[jslp] stall: a %d-node polled batch took %.3f ms in front of the poll (staging + launch) and %.3f ms polling (%u spins)\n", n_nodes, host_ms, wait_ms, spins);
    else
        fprintf(stderr, "[jslp] stall: a %d-node batch took %.3f ms to enqueue (staging + launches) and %.3f ms in hipStreamSynchronize\n", n_nodes, host_ms, wait_ms);
}

// ---- the phases of a node call --------------------------------------------------------------------------------------------------------
static long long tableau_cells(const jslp_engine* e) { return (long long)e->cap_rows * e->ld; }
// the checks, in the order the refused-call tests know (tests/test_branch_abi.py, tests/test_many_abi.py)
static int node_call_check(jslp_engine* e, const NodeCall& c) {
    if (e && !c.to_device()) e->dev_prev_valid = 0;
    if (!e || c.cuts.n_nodes < 0 || !c.cuts.offsets || (!c.out && !c.to_device())) return fail(JSLP_ERR_ARG, "relax_batch: null pointer");
    if (!e->uploaded) return fail(JSLP_ERR_STATE, "relax before upload");
    if (c.compact() && (e->n_watch <= 0 || e->n_watch > e->cap_rows))
        return fail(JSLP_ERR_ARG, c.records() ? "relax_batch_branch: after set_watched_variables (at most row_capacity of them)"
                                              : "relax_watched: after set_watched_variables (at most row_capacity of them)");
    if (c.checkpoint >= 0) JSLP_TRY(checkpoint_check(e, c.checkpoint, "relax_from"));
    if (!c.pinned && (c.rhs || c.var_index_by_row) && c.out_stride < e->cap_rows) return fail(JSLP_ERR_ARG, "relax_batch: out_stride < row capacity");
    if (c.cuts.n_nodes > 1 && !e->has_save && c.checkpoint < 0) return fail(JSLP_ERR_STATE, "relax_batch: several nodes need a saved root (save() first)");
    return JSLP_OK;
}

// ---- MIR node calls (include/jslpr_mir.h): where the kernels leave a node's MirRec, and what the host folds from it ------------------
// zero_copy: the pinned half as the device sees it (what a polled completion flag needs); else the device half, copied behind the kernels
static int mir_destination(jslp_engine* e, const NodeCall& c, size_t n_nodes, bool zero_copy, MirJob* mj) {
    if (sizeof(MirRec) * n_nodes > e->mir_rec.bytes()) {
        HIPC(hipStreamSynchronize(e->res.stream));
        HIPC(e->mir_rec.reserve(sizeof(MirRec) * std::max<size_t>(n_nodes, 16)));
    }
    mj->is_int = e->d_isint; mj->max_rounds = c.mir->max_rounds; mj->need_feasible = c.mir->need_feasible;
    mj->out = e->mir_rec.d.as<MirRec>();
    if (zero_copy) {
        void* p = nullptr;
        HIPC(hipHostGetDevicePointer(&p, e->mir_rec.h.p, 0));
        mj->out = static_cast<MirRec*>(p);
    }
    return JSLP_OK;
}
// node i's record -> its outcome, the evaluation folded over all its simplexes (fill_result knows the last one only), the host
// half of the work counters for the simplexes before the last
static void mir_fold(jslp_engine* e, const NodeCall& c, int i, const DevState& st, double prev_evaluation, jslp_simplex_result* out, double* evaluation_out) {
    const MirRec& r = e->mir_rec.h.as<MirRec>()[i];
    double ev = prev_evaluation;
    if (r.fold_kind == 1) {
        const double rc = js_round(1.0 / e->precision);
        ev = js_round((2.220446049250313e-16 + r.fold_obj) * rc) / rc;
    } else if (r.fold_kind == 2) {
        ev = -INFINITY;
    }
    out->evaluation = ev;
    *evaluation_out = ev;
    c.mir->outcomes[i] = jslpr_mir_outcome{r.rounds, r.rows_added, r.optimal_count, r.pivots, r.volume_before, r.volume_after};
    if (e->counting) {
        e->wc.simplex_calls += r.rounds;
        e->wc.pivots += (long long)r.pivots - ((long long)st.it1 + st.it2);
        e->wc.height_sum += r.height_sum - st.H;
    }
}

// ONE child of the saved root, slot 0 already in sync with the snapshot: one launch, one polled flag
static bool single_child_fast_path(const jslp_engine* e, const NodeCall& c) {
    return c.cuts.n_nodes == 1 && c.checkpoint < 0 && e->has_save && e->slot0_synced && !e->timing && e->force_path <= 1 &&
           e->one_launch_nodes && tableau_cells(e) <= wg_cells_child() && !c.shared.states && !c.to_device() && !c.records();
}
static int relax_single_child(jslp_engine* e, const NodeCall& c, bool dbg) {
    JSLP_TRY(upload_cuts(e, 1, c.cuts.offsets, c.cuts.type, c.cuts.var_index, c.cuts.value, false));
    JSLP_TRY(ensure_out(e, 1));
    void* out_dev = nullptr;  // the kernel writes the outcome straight into the pinned read-back buffer
    HIPC(hipHostGetDevicePointer(&out_dev, e->res.out.h.p, 0));
    char* ob = static_cast<char*>(out_dev);
    NodeArgs a{&e->s, root_snapshot(e), Cuts{e->d_cut_offs, e->d_cut_type, e->d_cut_var, e->d_cut_val}, c.check_cycles, iters_cap(e), (int)e->cap_rows};
    a.rhs = c.want_rhs ? reinterpret_cast<double*>(ob + ((char*)e->h_rhs - e->res.out.h.p)) : nullptr;
    a.rows = c.want_rows ? reinterpret_cast<int32_t*>(ob + ((char*)e->h_rows - e->res.out.h.p)) : nullptr;
    a.states = reinterpret_cast<DevState*>(ob);
    a.out_stride = c.compact() ? -e->n_watch : 0;
    e->last_path = "workgroup";
    DoneFlag flag;
    if (const hipError_t err = arm_done_flag(e, &flag); err != hipSuccess)
        return fail(JSLP_ERR_DEVICE, "%s: %s", "hipHostGetDevicePointer(&flag_dev, h_flag, 0)", hipGetErrorString(err));
    a.done_flag = flag.dev; a.done_seq = flag.seq;
    const size_t lds = wglds_smem(e);
    if (c.mir) JSLP_TRY(mir_destination(e, c, 1, true, &a.mj));
    JSLP_TRY(launch_node_kernel(single_node_kernel(e, lds, c.mir != nullptr), a, 1, lds, e->res.stream, dbg));
    unsigned spins;
    if (!wait_done_flag(flag.host, flag.seq, spins)) HIPC(hipStreamSynchronize(e->res.stream));
    const DevState st = e->h_states[0];
    int rc = state_error(st);
    if (rc) { e->slot0_synced = 0; return rc; }
    account(e, st, 1);
    if (e->counting) e->wc.cut_rows += c.cuts.offsets[1];
    double ev;
    JSLP_TRY(fill_result(e, st, 0, e->evaluation, &c.out[0], &ev));
    if (c.mir) mir_fold(e, c, 0, st, e->evaluation, &c.out[0], &ev);
    e->evaluation = ev;
    if (!c.pinned) {
        const size_t n_out = c.compact() ? (size_t)e->n_watch : (size_t)st.H;
        if (c.rhs) memcpy(c.rhs, e->h_rhs, sizeof(double) * n_out);
        if (c.var_index_by_row) memcpy(c.var_index_by_row, e->h_rows, sizeof(int32_t) * n_out);
    }
    return JSLP_OK;
}

struct NodePlan {
    bool wg;           // one workgroup per node (else: the chip-wide kernels on slot 0, node by node)
    int group;         // nodes per launch = tableau copies (slots) alive at once
    int n_grouped;     // the nodes [0, n_grouped) run in groups of `group`, the rest one by one in slot 0
    double prev_eval;  // what a node that reaches no optimum reports
};
static int plan_node_call(jslp_engine* e, const NodeCall& c, NodePlan* p) {
    const int n_nodes = c.cuts.n_nodes;
    const long long cells = tableau_cells(e);
    // branch-and-bound children (a saved root exists) need a handful of repair pivots each: one workgroup, one launch,
    // no host round trip.  A first solve / plain LP goes through the chip-wide path unless the tableau is tiny.
    p->wg = e->force_path == 1 ||
            (e->force_path == 0 && (((e->has_save || c.checkpoint >= 0) && cells <= (n_nodes > 1 ? WG_CELLS_BATCH : wg_cells_child())) || use_wg_single(e)));
    // a node that does not reach an optimum keeps the evaluation it started with: the checkpoint's (restoreCheckpoint,
    // incremental-branch-and-cut.ts:105) or the live one (restore() leaves it alone)
    p->prev_eval = c.checkpoint >= 0 ? e->ckpts[c.checkpoint].evaluation : e->evaluation;
    // group size: bounded by memory (<= 16 GiB of the 288 GB for tableau copies) and by what keeps every CU busy with several nodes
    p->group = 1;
    if (p->wg) {
        const long long max_slots = std::max<long long>(1, (16LL << 30) / (cells * 8));
        p->group = (int)std::min<long long>(std::min<long long>(n_nodes, group_max()), max_slots);
        if (const size_t lds = wglds_smem(e); lds && node_queue() && wg_batch_threads() == 512 && n_nodes > 1) {
            // the queue kernel wants exactly as many slots as the chip keeps workgroups resident
            if (e->queue_wgs == 0 || e->queue_wgs_lds != lds || e->queue_wgs_opt != (e->s.n_opt > 0)) {
                int per_cu = 0, cus = 0;
                // (the occupancy of the copy-on-write build whatever JSLP_NODE_COW says, of the OPT build with optional objectives)
                const NodeKernel& occ = e->s.n_opt > 0 ? NODE_QUEUE_OPT : NODE_QUEUE_COW;
                HIPC(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, occ.fn, occ.threads, lds));
                e->queue_wgs_opt = e->s.n_opt > 0;
                HIPC(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
                e->queue_wgs = std::max(1, per_cu * cus);
                e->queue_wgs_lds = lds;
            }
            p->group = (int)std::min<long long>(std::min<long long>(n_nodes, group_max_knob().set ? group_max() : e->queue_wgs), max_slots);
        }
        JSLP_TRY(ensure_slots(e, p->group));
    }
    // children of a checkpoint leave the live tableau (slot 0) holding the LAST of them (include/jslp_engine.h), as the sequential
    // reference does: the last of several nodes is a group of its own, in slot 0, behind the groups of the others
    p->n_grouped = (c.checkpoint >= 0 && p->wg && n_nodes > 1) ? n_nodes - 1 : n_nodes;
    return JSLP_OK;
}
static int ensure_records(jslp_engine* e, size_t n_nodes) {  // branch records of a batch: device + pinned
    if (sizeof(jslpx_branch_record) * n_nodes > e->rec.bytes()) HIPC(e->rec.reserve(sizeof(jslpx_branch_record) * std::max<size_t>(n_nodes, 16)));
    return JSLP_OK;
}

// where the kernels leave the outcomes: the device staging buffer (copied group by group on the copy stream), zero-copy the pinned host
// buffer itself - the stores cross PCIe while the other workgroups compute -, or the caller's device memory
struct NodeDest {
    DevState* states; double* rhs; int32_t* rows;
    bool zc;            // states / rhs / rows are the pinned host buffer as the device sees it
    bool copies;        // ... the staging buffer, and the call copies it to the pinned buffer itself (neither: the caller's device memory, or branch records)
    size_t row_stride;  // entries per node in rhs / rows
};
static int node_destination(jslp_engine* e, const NodeCall& c, NodeDest* d) {
    d->row_stride = c.compact() ? (size_t)e->n_watch : (c.to_device() ? (size_t)c.dev.stride : out_stride_of(e, c.shared));
    d->states = e->d_states; d->rhs = e->d_rhs; d->rows = e->d_rows;
    d->zc = zero_copy() != 0 && !c.records() && !c.to_device();  // (branch records: the compact read-back they are reduced from stays on the device)
    if (c.to_device()) { d->states = c.dev.states; d->rhs = c.dev.rhs; d->rows = c.dev.rows; }
    if (d->zc) {
        void *ps = nullptr, *pr = nullptr, *pw = nullptr;
        d->zc = hipHostGetDevicePointer(&ps, e->h_states, 0) == hipSuccess && hipHostGetDevicePointer(&pr, e->h_rhs, 0) == hipSuccess &&
                hipHostGetDevicePointer(&pw, e->h_rows, 0) == hipSuccess;
        if (d->zc) { d->states = static_cast<DevState*>(ps); d->rhs = static_cast<double*>(pr); d->rows = static_cast<int32_t*>(pw); }
        else (void)hipGetLastError();
    }
    d->copies = !d->zc && !c.to_device() && !c.records();
    if (d->copies && !e->res.copy_stream) {
        // created on first use, and only by the calls that copy their outcomes back (JSLP_ZERO_COPY=0, no mapped pinned memory): a stream costs a Solve of a
        // tiny model more than its pivots do
        HIPC(hipStreamCreateWithFlags(&e->res.copy_stream.h, hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&e->res.ev_group.h, hipEventDisableTiming));
    }
    return JSLP_OK;
}
// staging -> pinned for the nodes [first, first + g) (the three regions of the read-back buffer are laid out for all nodes, so a group
// is one contiguous slice of each)
static int copy_outcomes(jslp_engine* e, const NodeCall& c, const NodeDest& d, int first, int g, bool overlap) {
    hipStream_t on = e->res.stream;
    if (overlap) {  // a group's outcomes cross PCIe on the copy stream while the next group computes
        HIPC(hipEventRecord(e->res.ev_group, e->res.stream));
        HIPC(hipStreamWaitEvent(e->res.copy_stream, e->res.ev_group, 0));
        on = e->res.copy_stream;
    }
    const size_t off = (size_t)first * d.row_stride, len = (size_t)g * d.row_stride;
    HIPC(hipMemcpyAsync(e->h_states + first, e->d_states + first, sizeof(DevState) * (size_t)g, hipMemcpyDeviceToHost, on));
    if (c.want_rhs) HIPC(hipMemcpyAsync(e->h_rhs + off, e->d_rhs + off, sizeof(double) * len, hipMemcpyDeviceToHost, on));
    if (c.want_rows) HIPC(hipMemcpyAsync(e->h_rows + off, e->d_rows + off, sizeof(int32_t) * len, hipMemcpyDeviceToHost, on));
    return JSLP_OK;
}

// the slots [0, n) are in sync with the snapshot (the saved root except for their dirty rows) and nothing asks for the eager sequence: the node kernels may start from them
static bool node_kernels_fit(const jslp_engine* e, const NodeCall& c, int n) {
    return c.checkpoint < 0 && e->has_save && e->slot0_synced && n <= e->slots_synced && !e->timing && e->one_launch_nodes && wg_batch_threads() == 512;
}
// the whole batch in ONE launch of resident workgroups that pull nodes from a queue (more nodes than slots)
static int enqueue_queue(jslp_engine* e, const NodeCall& c, const NodePlan& p, const NodeDest& d, NodeArgs a, bool dbg) {
    const int n_nodes = c.cuts.n_nodes;
    e->last_path = "workgroup";
    e->node_queue_launches += 1;
    // (an order only where it can matter: more nodes than resident workgroups -- a batch that starts all at once pays the order array's trip per node
    //  for nothing: the four-member pool's 604-node shares lost 6 % to it; the full read-back stays in call order unless node_queue_order_full())
    const bool pcie_bound = d.zc && !c.compact() && (c.want_rhs || c.want_rows);
    a.n_nodes = n_nodes;
    a.order = (node_queue() == 2 && n_nodes > p.group && (node_queue_order_full() || !pcie_bound)) ? e->d_cut_order : (const int32_t*)nullptr;
    a.queue = e->d_queue;
    JSLP_TRY(launch_node_kernel(queue_kernel(e, c.mir != nullptr), a, p.group, wglds_smem(e), e->res.stream, dbg));
    return d.copies ? copy_outcomes(e, c, d, 0, n_nodes, false) : JSLP_OK;
}
// slots already in sync with the snapshot: restore of the dirty rows, cuts, simplex and gather in ONE launch per
// group (what a workgroup restores and cuts stays in its XCD's L2 for its own pivots)
static int enqueue_one_launch_group(jslp_engine* e, const NodeCall& c, const NodeDest& d, NodeArgs a, int first, int g, bool dbg, DoneFlag* polled) {
    e->last_path = "workgroup";
    const size_t lds = wglds_smem(e);
    a.first = first;
    // a batch that is ONE group, its outcomes written straight into pinned memory: the last workgroup raises the completion
    // flag the host polls instead of the two stream synchronisations that end the other shapes of this call
    if (small_batch_shape(e, lds, g) && g == c.cuts.n_nodes && d.zc && !c.shared.states && batch_poll_on()) {
        if (arm_done_flag(e, polled) == hipSuccess) { a.done_flag = polled->dev; a.done_seq = polled->seq; a.done_count = e->d_done_count; }
        else (void)hipGetLastError();
    }
    return launch_node_kernel(group_kernel(e, lds, g, c.mir != nullptr), a, g, lds, e->res.stream, dbg);
}
// restore, cuts, simplex and gather as launches of their own: any start, any tableau
static int enqueue_eager_group(jslp_engine* e, const NodeCall& c, const NodePlan& p, const NodeArgs& a, int first, int g, bool dbg) {
    hipStream_t s = e->res.stream;
    if (c.mir) return fail(JSLP_ERR_STATE, "internal: a MIR node call reached the eager sequence (mir_one_launch)");
    JSLP_TRY(enqueue_restore(e, 0, g, c.checkpoint));
    hipLaunchKernelGGL(k_add_cuts, dim3(g), dim3(256), 0, s, e->s, a.cu, 0, first, (int)e->cap_rows);
    HIPC(hipGetLastError());
    if (p.wg) {
        e->last_path = "workgroup";
        const size_t lds = wglds_smem(e);
        JSLP_TRY(launch_node_kernel(eager_kernel(e, lds, g), a, g, lds, s, dbg));
    } else {
        // big tableau: the chip-wide kernels on slot 0 (g == 1)
        if (dbg) debug_node_launch("restore+add_cuts+simplex+gather chip-wide", g, -1, 0);
        HIPC(hipMemcpyAsync(e->h_state, e->s.st, sizeof(DevState), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        JSLP_TRY(state_error(*e->h_state));
        JSLP_TRY(run_simplex(e, c.check_cycles));
    }
    hipLaunchKernelGGL(k_gather, dim3(g), dim3(256), 0, s, e->s, 0, a.rhs, a.rows, a.states, a.out_stride, first);
    HIPC(hipGetLastError());
    return JSLP_OK;
}
// the end of every shape but the single child's: the polled flag of a small batch, else both streams
static int wait_for_nodes(jslp_engine* e, int n_nodes, const DoneFlag& polled, std::chrono::steady_clock::time_point t_enter) {
    bool arrived = false;
    if (polled.host) {
        unsigned spins = 0;
        const auto t_poll = std::chrono::steady_clock::now();
        arrived = wait_done_flag(polled.host, polled.seq, spins);
        if (debug_stall_ms() > 0) report_stall(n_nodes, true, t_enter, t_poll, spins);
    }
    if (!arrived) {  // every other shape -- and a polled batch that did not show up in 5 s: let the runtime report the fault
        const auto t_sync = std::chrono::steady_clock::now();
        if (e->res.copy_stream) HIPC(hipStreamSynchronize(e->res.copy_stream));
        HIPC(hipStreamSynchronize(e->res.stream));
        if (debug_stall_ms() > 0) report_stall(n_nodes, false, t_enter, t_sync, 0);
    }
    return JSLP_OK;
}

// the 128-byte state of every node, in call order: the first error ends the call, the engine's evaluation is the last node's
static int decode_outcomes(jslp_engine* e, const NodeCall& c, const NodePlan& p, const NodeDest& d) {
    const int n_nodes = c.cuts.n_nodes;
    if (c.to_device()) {
        // the outcomes stay on the device (the caller converts the gathered records with jslp_engine_results_from_states), but the
        // engine's own bookkeeping must not depend on where they went: the 128-byte records of THIS call come back (n x 128 B) so
        // that a node that ended in an error clears the slot-sync flags (later one-launch / copy-on-write batches must not start
        // from slots it left dirty), the work counters see the pivots, and the engine's evaluation is the last node's
        HIPC(hipMemcpy(e->h_states, c.dev.states, sizeof(DevState) * (size_t)n_nodes, hipMemcpyDeviceToHost));
        e->dev_prev_evaluation = p.prev_eval;  // what results_from_states hands a node that reaches no optimum (as the host path does)
        e->dev_prev_valid = 1;
    }
    for (int i = 0; i < n_nodes; i++) {
        DevState st = e->h_states[i];
        int rc = state_error(st);
        if (rc) { e->slot0_synced = 0; e->slots_synced = 0; return rc; }
        account(e, st, 1);
        if (c.to_device()) {  // (a record carries no pivot history: results_from_states reports a cycle without its detail, and so does this)
            if (i < n_nodes - 1) continue;
            jslp_simplex_result last;
            st.hist_n = 0;
            JSLP_TRY(fill_result(e, st, 0, p.prev_eval, &last, &e->evaluation));
            continue;
        }
        if (st.cycle_phase && p.wg && (n_nodes > p.group || (p.n_grouped < n_nodes && i == 0))) {
            // the cycle message is rebuilt from the slot's history, which later groups have reused (of the children of a checkpoint in
            // one group only the first: the last child ran in its slot after it): report the hit (flags are exact) without the
            // [start, length] detail
            st.hist_n = 0;
        }
        double ev;
        JSLP_TRY(fill_result(e, st, p.wg && i < p.n_grouped ? i % p.group : 0, p.prev_eval, &c.out[i], &ev));
        if (c.mir) mir_fold(e, c, i, st, p.prev_eval, &c.out[i], &ev);
        if (i == n_nodes - 1) e->evaluation = ev;
        if (!c.pinned && !c.compact()) {
            const size_t n_out = (size_t)st.H;
            if (c.rhs) memcpy(c.rhs + (size_t)i * c.out_stride, e->h_rhs + (size_t)i * d.row_stride, sizeof(double) * n_out);
            if (c.var_index_by_row) memcpy(c.var_index_by_row + (size_t)i * c.out_stride, e->h_rows + (size_t)i * d.row_stride, sizeof(int32_t) * n_out);
        }
    }
    if (c.to_device()) return JSLP_OK;
    if (c.records()) { e->dev_prev_evaluation = p.prev_eval; e->dev_prev_valid = 1; }
    if (!c.pinned && c.compact()) {  // same layout on both sides: one copy each (per-node copies cost more than the kernel's share of a node)
        if (c.rhs) memcpy(c.rhs, e->h_rhs, sizeof(double) * (size_t)n_nodes * d.row_stride);
        if (c.var_index_by_row) memcpy(c.var_index_by_row, e->h_rows, sizeof(int32_t) * (size_t)n_nodes * d.row_stride);
    }
    return JSLP_OK;
}

// Every node entry point ends here.  Per-node-workgroup path: all groups are enqueued back to back, their outcomes accumulate in ONE
// buffer laid out for all n_nodes, one wait ends the call.
static int relax_batch_impl(jslp_engine* e, const NodeCall& c) {
    const auto t_enter = std::chrono::steady_clock::now();  // (JSLP_DEBUG_STALL)
    int rc = node_call_check(e, c);
    const int n_nodes = c.cuts.n_nodes;
    if (rc || n_nodes == 0) return rc;
    HIPC(hipSetDevice(e->device));
    hipStream_t s = e->res.stream;
    const bool dbg = debug_launch_on();  // (read per call, as run_simplex does: tests switch it inside one process)
    if (single_child_fast_path(e, c)) return relax_single_child(e, c, dbg);
    JSLP_TRY(upload_cuts(e, n_nodes, c.cuts.offsets, c.cuts.type, c.cuts.var_index, c.cuts.value));
    NodePlan p;
    JSLP_TRY(plan_node_call(e, c, &p));
    JSLP_TRY(ensure_out(e, (size_t)n_nodes, c.shared));  // laid out for ALL nodes: [states | rhs | rows]
    if (c.records()) JSLP_TRY(ensure_records(e, (size_t)n_nodes));
    if (e->timing) HIPC(hipEventRecord(e->res.ev_begin, s));
    NodeDest d;
    JSLP_TRY(node_destination(e, c, &d));
    NodeArgs a{&e->s, root_snapshot(e), Cuts{e->d_cut_offs, e->d_cut_type, e->d_cut_var, e->d_cut_val}, c.check_cycles, iters_cap(e), (int)e->cap_rows,
               c.want_rhs ? d.rhs : nullptr, c.want_rows ? d.rows : nullptr, d.states, c.compact() ? -e->n_watch : (int)d.row_stride};
    if (c.mir) JSLP_TRY(mir_destination(e, c, (size_t)n_nodes, d.zc, &a.mj));
    DoneFlag polled;  // armed when the call ends by polling a completion flag instead of synchronising the streams
    if (p.wg && wglds_smem(e) && node_queue() && n_nodes > p.group && node_kernels_fit(e, c, p.group)) {
        JSLP_TRY(enqueue_queue(e, c, p, d, a, dbg));
    } else {
        for (int first = 0, g = 0; first < n_nodes; first += g) {
            g = first < p.n_grouped ? std::min(p.group, p.n_grouped - first) : 1;
            JSLP_TRY(p.wg && g > 1 && node_kernels_fit(e, c, g) ? enqueue_one_launch_group(e, c, d, a, first, g, dbg, &polled) : enqueue_eager_group(e, c, p, a, first, g, dbg));
            if (d.copies) JSLP_TRY(copy_outcomes(e, c, d, first, g, true));
        }
    }
    if (c.records()) {  // the branch records of the whole batch, one workgroup per node, behind every node kernel on the stream
        hipLaunchKernelGGL(k_branch_record, dim3(n_nodes), dim3(256), 0, s, d.states, d.rows, d.rhs, e->s.watch, (int)e->n_watch, e->precision,
                           c.to_device() ? c.dev.rec : e->rec.d.as<double>());
        HIPC(hipGetLastError());
        if (!c.to_device()) {
            HIPC(hipMemcpyAsync(e->h_states, e->d_states, sizeof(DevState) * (size_t)n_nodes, hipMemcpyDeviceToHost, s));
            HIPC(hipMemcpyAsync(e->rec.h.p, e->rec.d.p, sizeof(jslpx_branch_record) * (size_t)n_nodes, hipMemcpyDeviceToHost, s));
        }
    }
    if (c.mir && !d.zc) HIPC(hipMemcpyAsync(e->mir_rec.h.p, e->mir_rec.d.p, sizeof(MirRec) * (size_t)n_nodes, hipMemcpyDeviceToHost, s));
    if (e->timing && p.wg) HIPC(hipEventRecord(e->res.ev_end, s));
    JSLP_TRY(wait_for_nodes(e, n_nodes, polled, t_enter));
    float ms = 0;
    if (p.wg && e->timing && hipEventElapsedTime(&ms, e->res.ev_begin, e->res.ev_end) == hipSuccess) e->total_ms += ms;
    if (e->counting) e->wc.cut_rows += c.cuts.offsets[n_nodes];
    return decode_outcomes(e, c, p, d);
}

extern "C" int jslp_engine_relax_batch(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                       const int32_t* var_index, const double* value, int check_cycles,
                                       jslp_simplex_result* out, double* rhs, int32_t* var_index_by_row,
                                       int32_t out_stride) {
    return jslp_engine_relax_from(e, -1, n_nodes, cut_offsets, type, var_index, value, check_cycles, out, rhs, var_index_by_row, out_stride);
}

// ---- outcomes left in DEVICE memory of the caller (the N > 1 process path: they are the input of an RCCL all-gather) -------------
extern "C" int32_t jslp_engine_state_record_bytes(void) { return (int32_t)sizeof(DevState); }

extern "C" int jslp_engine_relax_batch_device(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                              const int32_t* var_index, const double* value, int check_cycles, void* d_states,
                                              double* d_rhs, int32_t* d_rows, int32_t row_stride) {
    if (!e || !d_states || !d_rhs || !d_rows) return fail(JSLP_ERR_ARG, "relax_batch_device: null pointer");
    if (row_stride < e->cap_rows) return fail(JSLP_ERR_ARG, "relax_batch_device: row_stride < row capacity");
    return relax_batch_impl(e, NodeCall{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles, .want_rhs = true, .want_rows = true,
                                        .dev = {.states = static_cast<DevState*>(d_states), .rhs = d_rhs, .rows = d_rows, .stride = row_stride}});
}

// `states`: n_nodes raw records in HOST memory (wherever they were evaluated: this rank's own or another rank's, after the
// exchange) -> the result structs every other entry point returns.  A record carries no pivot history: the [start, length] detail of
// a detected cycle is reported as 0 (the flags and the phase are exact).
extern "C" int jslp_engine_results_from_states(jslp_engine* e, const void* states, int32_t n_nodes, jslp_simplex_result* out) {
    if (!e || !states || !out || n_nodes < 0) return fail(JSLP_ERR_ARG, "results_from_states: bad arguments");
    const DevState* st = static_cast<const DevState*>(states);
    for (int32_t i = 0; i < n_nodes; i++) {
        DevState rec = st[i];
        int rc = state_error(rec);
        if (rc) return rc;
        rec.hist_n = 0;
        double ev;
        rc = fill_result(e, rec, 0, e->dev_prev_valid ? e->dev_prev_evaluation : e->evaluation, &out[i], &ev);
        if (rc) return rc;
    }
    return JSLP_OK;
}

extern "C" int jslp_engine_relax_batch_pinned(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets,
                                              const int8_t* type, const int32_t* var_index, const double* value,
                                              int check_cycles, jslp_simplex_result* out, const double** rhs,
                                              const int32_t** var_index_by_row, int32_t* out_stride) {
    if (!e) return fail(JSLP_ERR_ARG, "relax_batch_pinned: null engine");
    JSLP_TRY(relax_batch_impl(e, NodeCall{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles,
                                          .want_rhs = rhs != nullptr, .want_rows = var_index_by_row != nullptr, .out = out, .pinned = true}));
    if (rhs) *rhs = n_nodes > 0 ? e->h_rhs : nullptr;
    if (var_index_by_row) *var_index_by_row = n_nodes > 0 ? e->h_rows : nullptr;
    if (out_stride) *out_stride = (int32_t)out_stride_of(e);
    return JSLP_OK;
}

extern "C" int jslp_engine_relax_from(jslp_engine* e, int32_t checkpoint, int32_t n_nodes, const int32_t* cut_offsets,
                                      const int8_t* type, const int32_t* var_index, const double* value, int check_cycles,
                                      jslp_simplex_result* out, double* rhs, int32_t* var_index_by_row,
                                      int32_t out_stride) {
    return relax_batch_impl(e, NodeCall{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles, .checkpoint = checkpoint < 0 ? -1 : checkpoint,
                                        .want_rhs = rhs != nullptr, .want_rows = var_index_by_row != nullptr,
                                        .out = out, .rhs = rhs, .var_index_by_row = var_index_by_row, .out_stride = out_stride});
}

extern "C" int jslp_engine_relax(jslp_engine* e, int32_t n_cuts, const int8_t* type, const int32_t* var_index,
                                 const double* value, int check_cycles, jslp_simplex_result* out, double* rhs,
                                 int32_t* var_index_by_row) {
    if (!e) return fail(JSLP_ERR_ARG, "relax: null engine");
    if (n_cuts < 0) return fail(JSLP_ERR_ARG, "relax: negative cut count");
    const int32_t offs[2] = {0, n_cuts};
    return jslp_engine_relax_batch(e, 1, offs, type, var_index, value, check_cycles, out, rhs, var_index_by_row,
                                   e->cap_rows);
}

// ---- a node with its MIR loop in one call (include/jslpr_mir.h) -------------------------------------------------------
static_assert(sizeof(jslpr_mir_outcome) == 32 && JSLPR_MAX_ROUNDS == JSLPR_MAX_ROUNDS_DEV, "include/jslpr_mir.h and jslp_mir.hip.h agree");
extern "C" int32_t jslpr_mir_outcome_bytes(void) { return (int32_t)sizeof(jslpr_mir_outcome); }

// every node of the call would go through ONE launch of an LDS node kernel: what relax_batch_impl decides, asked beforehand
static int mir_one_launch(jslp_engine* e, const NodeCall& c, bool* yes) {
    *yes = false;
    if (!wglds_smem(e) || c.checkpoint >= 0 || c.shared.states || !e->has_save) return JSLP_OK;
    const int n_nodes = c.cuts.n_nodes;
    NodePlan p;
    JSLP_TRY(plan_node_call(e, c, &p));
    // slots that are not in sync with the saved root yet are restored first -- what the eager sequence of a plain call begins with, and
    // what leaves them in sync for every later call: a tree's MIR batches reach the one-launch shapes from their second call on at the latest
    if (const int need = n_nodes == 1 ? 1 : p.group; p.wg && (!e->slot0_synced || need > e->slots_synced)) JSLP_TRY(enqueue_restore(e, 0, need));
    if (single_child_fast_path(e, c)) { *yes = true; return JSLP_OK; }
    if (!p.wg) return JSLP_OK;
    if (node_queue() && n_nodes > p.group && node_kernels_fit(e, c, p.group)) { *yes = true; return JSLP_OK; }
    for (int first = 0, g = 0; first < n_nodes; first += g) {
        g = first < p.n_grouped ? std::min(p.group, p.n_grouped - first) : 1;
        if (!(g > 1 && node_kernels_fit(e, c, g))) return JSLP_OK;
    }
    *yes = true;
    return JSLP_OK;
}
// computeFractionalVolume(true) of the live tableau, computed on the device: 8 bytes come back
static int device_volume(jslp_engine* e, double* volume) {
    if (e->mir_rec.bytes() < sizeof(MirRec)) {
        HIPC(hipStreamSynchronize(e->res.stream));
        HIPC(e->mir_rec.reserve(sizeof(MirRec) * 16));
    }
    MirLaunch m{};
    m.s = e->s; m.mj.is_int = e->d_isint; m.volume_out = e->mir_rec.d.as<double>();
    if (mir_launch(MIR_K_VOLUME, 1, 0, m, e->res.stream) == -1) return fail(JSLP_ERR_STATE, "internal: no k_fractional_volume in this build");
    HIPC(hipGetLastError());  // (the unit only peeked at the launch's error)
    HIPC(hipMemcpyAsync(e->mir_rec.h.p, e->mir_rec.d.p, sizeof(double), hipMemcpyDeviceToHost, e->res.stream));
    HIPC(hipStreamSynchronize(e->res.stream));
    *volume = *e->mir_rec.h.as<double>();
    return JSLP_OK;
}
// the same node through the engine's existing launches, one after the other: any start, any tableau (no saved root, a checkpoint,
// k_node_wg, the chip-wide kernels)
static int relax_mir_sequence(jslp_engine* e, const NodeCall& one, const MirCall& job, jslpr_mir_outcome* oc) {
    JSLP_TRY(relax_batch_impl(e, one));
    jslp_simplex_result& res = one.out[0];
    *oc = jslpr_mir_outcome{0, 0, res.optimal, res.pivots_phase1 + std::max(res.pivots_phase2, 0), 0.0, 0.0};
    if (job.need_feasible && !res.feasible) return JSLP_OK;
    const int limit = job.max_rounds < 0 ? JSLPR_MAX_ROUNDS : job.max_rounds;
    if (limit == 0) return JSLP_OK;
    bool stopped = false;
    double before = 0.0;
    JSLP_TRY(device_volume(e, &before));
    while (!stopped && oc->rounds < limit) {
        int32_t n = 0;
        JSLP_TRY(jslp_engine_apply_mir_cuts(e, &n));
        JSLP_TRY(jslp_engine_simplex(e, one.check_cycles, &res));
        oc->rounds += 1;
        oc->rows_added += n;
        oc->optimal_count += res.optimal;
        oc->pivots += res.pivots_phase1 + std::max(res.pivots_phase2, 0);
        double after = 0.0;
        JSLP_TRY(device_volume(e, &after));
        oc->volume_before = before;
        oc->volume_after = after;
        if (after >= 0.9 * before) stopped = true;
        before = after;
    }
    if (!stopped && job.max_rounds < 0) return fail(JSLP_ERR_CAPACITY, "relax_mir: the MIR loop reached JSLPR_MAX_ROUNDS without a stop");
    if (one.rhs || one.var_index_by_row) JSLP_TRY(jslp_engine_read_rhs(e, one.rhs, one.var_index_by_row));
    return JSLP_OK;
}

extern "C" int jslpr_engine_relax_mir(jslp_engine* e, int32_t checkpoint, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                      const int32_t* var_index, const double* value, int check_cycles, int32_t max_rounds, int32_t need_feasible,
                                      jslp_simplex_result* out, jslpr_mir_outcome* mir, double* rhs, int32_t* var_index_by_row, int32_t out_stride) {
    if (!e || !mir) return fail(JSLP_ERR_ARG, "relax_mir: null pointer");
    if (checkpoint >= 0 && n_nodes != 1) return fail(JSLP_ERR_ARG, "relax_mir: a checkpoint start takes exactly one node");
    if (max_rounds > JSLPR_MAX_ROUNDS) return fail(JSLP_ERR_ARG, "relax_mir: max_rounds > JSLPR_MAX_ROUNDS");
    const MirCall job{max_rounds < 0 ? -1 : max_rounds, need_feasible ? 1 : 0, mir};
    const NodeCall c{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles, .checkpoint = checkpoint < 0 ? -1 : checkpoint,
                     .want_rhs = rhs != nullptr, .want_rows = var_index_by_row != nullptr,
                     .out = out, .rhs = rhs, .var_index_by_row = var_index_by_row, .out_stride = out_stride, .mir = &job};
    JSLP_TRY(node_call_check(e, c));
    if (!e->has_int) return fail(JSLP_ERR_STATE, "relax_mir: after set_integer_variables");
    if (e->s.n_opt > 0) return fail(JSLP_ERR_UNSUPPORTED, "relax_mir: optional objectives are not supported");
    if (n_nodes == 0) return JSLP_OK;
    HIPC(hipSetDevice(e->device));
    bool one_launch = false;
    JSLP_TRY(mir_one_launch(e, c, &one_launch));
    if (one_launch) return relax_batch_impl(e, c);
    // every other shape: node by node.  Each node's folded evaluation starts from the one the call began with
    const double prev = e->evaluation;
    for (int32_t i = 0; i < n_nodes; i++) {
        const int32_t a = cut_offsets[i], offs[2] = {0, cut_offsets[i + 1] - a};
        NodeCall one = c;
        one.mir = nullptr;
        one.cuts = {1, offs, type ? type + a : nullptr, var_index ? var_index + a : nullptr, value ? value + a : nullptr};
        one.out = out + i;
        one.rhs = rhs ? rhs + (size_t)i * out_stride : nullptr;
        one.var_index_by_row = var_index_by_row ? var_index_by_row + (size_t)i * out_stride : nullptr;
        e->evaluation = prev;
        JSLP_TRY(relax_mir_sequence(e, one, job, &mir[i]));
    }
    return JSLP_OK;
}

// ---- compact read-back -----------------------------------------------------------------------------------------------
extern "C" int jslp_engine_set_watched_variables(jslp_engine* e, const int32_t* var_indexes, int32_t n) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "set_watched_variables before upload");
    if (n < 0 || (n > 0 && !var_indexes)) return fail(JSLP_ERR_ARG, "set_watched_variables: bad arguments");
    for (int32_t i = 0; i < n; i++)
        if (var_indexes[i] < 0 || var_indexes[i] >= e->n_idx) return fail(JSLP_ERR_ARG, "set_watched_variables: index out of range");
    HIPC(hipSetDevice(e->device));
    HIPC(hipStreamSynchronize(e->res.stream));
    e->d_watch.reset();
    e->n_watch = 0; e->s.watch = nullptr; e->s.n_watch = 0; e->s.watch_pos = nullptr;
    if (n > 0) {
        // [the list | variable index -> position in the list] (the second half only when no variable is listed twice)
        std::vector<int32_t> pos((size_t)e->n_idx, -1);
        bool unique = true;
        for (int32_t i = 0; i < n; i++) {
            if (pos[var_indexes[i]] >= 0) unique = false;
            pos[var_indexes[i]] = i;
        }
        HIPC(e->d_watch.reserve(sizeof(int32_t) * ((size_t)n + (size_t)e->n_idx)));
        int32_t* const watch = e->d_watch.as<int32_t>();
        HIPC(hipMemcpy(watch, var_indexes, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(watch + n, pos.data(), sizeof(int32_t) * (size_t)e->n_idx, hipMemcpyHostToDevice));
        e->n_watch = n; e->s.watch = watch; e->s.n_watch = n;
        e->s.watch_pos = unique ? watch + n : nullptr;
    }
    return JSLP_OK;
}

extern "C" int jslp_engine_relax_watched(jslp_engine* e, int32_t n_cuts, const int8_t* type, const int32_t* var_index,
                                         const double* value, int check_cycles, jslp_simplex_result* out,
                                         int32_t* watched_row, double* watched_value) {
    if (!e) return fail(JSLP_ERR_ARG, "relax_watched: null engine");
    if (n_cuts < 0) return fail(JSLP_ERR_ARG, "relax_watched: negative cut count");
    const int32_t offs[2] = {0, n_cuts};
    return jslp_engine_relax_batch_watched(e, 1, offs, type, var_index, value, check_cycles, out, watched_row, watched_value);
}

extern "C" int jslp_engine_relax_batch_watched(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                               const int32_t* var_index, const double* value, int check_cycles,
                                               jslp_simplex_result* out, int32_t* watched_row, double* watched_value) {
    if (!e) return fail(JSLP_ERR_ARG, "relax_batch_watched: null engine");
    return relax_batch_impl(e, NodeCall{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles, .read_back = ReadBack::Watched,
                                        .want_rhs = watched_value != nullptr, .want_rows = watched_row != nullptr,
                                        .out = out, .rhs = watched_value, .var_index_by_row = watched_row, .out_stride = e->cap_rows});
}

extern "C" int jslp_engine_relax_batch_watched_pinned(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                                      const int32_t* var_index, const double* value, int check_cycles,
                                                      jslp_simplex_result* out, const int32_t** watched_row,
                                                      const double** watched_value) {
    if (!e) return fail(JSLP_ERR_ARG, "relax_batch_watched_pinned: null engine");
    JSLP_TRY(relax_batch_impl(e, NodeCall{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles, .read_back = ReadBack::Watched,
                                          .want_rhs = watched_value != nullptr, .want_rows = watched_row != nullptr, .out = out, .pinned = true}));
    if (watched_row) *watched_row = n_nodes > 0 ? e->h_rows : nullptr;
    if (watched_value) *watched_value = n_nodes > 0 ? e->h_rhs : nullptr;
    return JSLP_OK;
}

// ---- work counters ---------------------------------------------------------------------------------------------------
// the compact read-back left in the caller's DEVICE memory: the exchange payload of the multi-process path (sharding.py)
extern "C" int jslp_engine_relax_batch_watched_device(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                                      const int32_t* var_index, const double* value, int check_cycles, void* d_states,
                                                      int32_t* d_watched_row, double* d_watched_value) {
    if (!e || !d_states || !d_watched_row || !d_watched_value) return fail(JSLP_ERR_ARG, "relax_batch_watched_device: null pointer");
    return relax_batch_impl(e, NodeCall{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles, .read_back = ReadBack::Watched, .want_rhs = true, .want_rows = true,
                                        .dev = {.states = static_cast<DevState*>(d_states), .rhs = d_watched_value, .rows = d_watched_row, .stride = e->n_watch}});
}

extern "C" int32_t jslp_engine_watched_count(const jslp_engine* e) { return e ? e->n_watch : 0; }

// ---- branch records (include/jslpx_branch.h) --------------------------------------------------------------------------------------
static_assert(sizeof(jslpx_branch_record) == 32, "jslpx_branch_record is 32 bytes");
static_assert(BREC_FEASIBLE == JSLPX_BRANCH_FEASIBLE && BREC_BOUNDED == JSLPX_BRANCH_BOUNDED && BREC_OPTIMAL == JSLPX_BRANCH_OPTIMAL &&
              BREC_INTEGRAL == JSLPX_BRANCH_INTEGRAL, "branch record flags");
extern "C" int32_t jslpx_branch_record_bytes(void) { return (int32_t)sizeof(jslpx_branch_record); }

// where relax_batch_impl leaves the per-node results of a record call (the engine's bookkeeping; the caller gets the records)
static jslp_simplex_result* branch_results_scratch(jslp_engine* e, int32_t n_nodes) {
    if ((int32_t)e->rec_results.size() < std::max(n_nodes, 1)) e->rec_results.resize((size_t)std::max(n_nodes, 1));
    return e->rec_results.data();
}

extern "C" int jslpx_engine_relax_batch_branch(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                               const int32_t* var_index, const double* value, int check_cycles, jslpx_branch_record* out) {
    if (!e || !out) return fail(JSLP_ERR_ARG, "relax_batch_branch: null pointer");
    jslp_simplex_result* res = branch_results_scratch(e, std::max(n_nodes, 0));
    JSLP_TRY(relax_batch_impl(e, NodeCall{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles, .read_back = ReadBack::BranchRecord,
                                          .want_rhs = true, .want_rows = true, .out = res, .pinned = true}));
    if (n_nodes > 0) memcpy(out, e->rec.h.p, sizeof(jslpx_branch_record) * (size_t)n_nodes);
    return JSLP_OK;
}

extern "C" int jslpx_engine_relax_batch_branch_pinned(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                                      const int32_t* var_index, const double* value, int check_cycles,
                                                      const jslpx_branch_record** out) {
    if (!e || !out) return fail(JSLP_ERR_ARG, "relax_batch_branch_pinned: null pointer");
    jslp_simplex_result* res = branch_results_scratch(e, std::max(n_nodes, 0));
    JSLP_TRY(relax_batch_impl(e, NodeCall{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles, .read_back = ReadBack::BranchRecord,
                                          .want_rhs = true, .want_rows = true, .out = res, .pinned = true}));
    *out = n_nodes > 0 ? e->rec.h.as<jslpx_branch_record>() : nullptr;
    return JSLP_OK;
}

// the records in the caller's device memory; the compact read-back they are reduced from and the 128-byte states the engine checks every
// node with stay in its own staging buffers
extern "C" int jslpx_engine_relax_batch_branch_device(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                                      const int32_t* var_index, const double* value, int check_cycles, void* d_records) {
    if (!e || !d_records) return fail(JSLP_ERR_ARG, "relax_batch_branch_device: null pointer");
    if ((reinterpret_cast<uintptr_t>(d_records) & 15) != 0) return fail(JSLP_ERR_ARG, "relax_batch_branch_device: records must be 16-byte aligned");
    if (!e->uploaded) return fail(JSLP_ERR_STATE, "relax before upload");
    if (e->n_watch <= 0 || e->n_watch > e->cap_rows)
        return fail(JSLP_ERR_ARG, "relax_batch_branch: after set_watched_variables (at most row_capacity of them)");
    HIPC(hipSetDevice(e->device));
    JSLP_TRY(ensure_out(e, (size_t)std::max(n_nodes, 1)));
    // (the compact read-back stays in the engine's own staging buffers, which ensure_out has just laid out)
    return relax_batch_impl(e, NodeCall{.cuts = {n_nodes, cut_offsets, type, var_index, value}, .check_cycles = check_cycles, .read_back = ReadBack::BranchRecord, .want_rhs = true, .want_rows = true,
                                        .dev = {.states = e->d_states, .rhs = e->d_rhs, .rows = e->d_rows, .stride = e->n_watch, .rec = static_cast<double*>(d_records)}});
}

// records (host memory: this rank's or, after the exchange, another rank's) -> result structs, evaluation as fill_result derives it
extern "C" int jslpx_engine_results_from_branch_records(jslp_engine* e, const void* records, int32_t n, jslp_simplex_result* out) {
    if (!e || n < 0 || (n > 0 && (!records || !out))) return fail(JSLP_ERR_ARG, "results_from_branch_records: bad arguments");
    const jslpx_branch_record* rec = static_cast<const jslpx_branch_record*>(records);
    const double prev = e->dev_prev_valid ? e->dev_prev_evaluation : e->evaluation;
    const double rc = js_round(1.0 / e->precision);
    for (int32_t i = 0; i < n; i++) {
        jslpx_branch_record r;
        memcpy(&r, rec + i, sizeof r);
        jslp_simplex_result& o = out[i];
        memset(&o, 0, sizeof o);
        o.feasible = (r.flags & JSLPX_BRANCH_FEASIBLE) != 0;
        o.bounded = (r.flags & JSLPX_BRANCH_BOUNDED) != 0;
        o.optimal = (r.flags & JSLPX_BRANCH_OPTIMAL) != 0;
        o.unbounded_var_index = r.unbounded_var_index;
        o.height = r.height;
        o.obj_cell = r.obj_cell;
        o.evaluation = o.optimal ? js_round((2.220446049250313e-16 + r.obj_cell) * rc) / rc : (!o.bounded ? -INFINITY : prev);
    }
    return JSLP_OK;
}

// ---- many independent LPs in one launch (include/jslpm_many.h) ------------------------------------------------------------------
// Per device, kept from call to call: the descriptor table and the final states of a batch, [ManyLp x n | DevState x n] on the
// device and its pinned twin.  One call at a time holds them (g_many_mu); jslp_release_pooled_resources frees them.
struct ManyRes {
    int device = -1;
    StagePair buf;
};
static std::mutex g_many_mu;
static std::vector<ManyRes>& g_many = *new std::vector<ManyRes>();  // (never destroyed: see g_pool)

static void release_many_resources() {
    std::lock_guard<std::mutex> lk(g_many_mu);
    for (auto& r : g_many) {
        hipSetDevice(r.device);
        r.buf = StagePair();
    }
    g_many.clear();
}

static int many_buffers(int device, size_t bytes, ManyRes** out) {  // (caller holds g_many_mu)
    ManyRes* r = nullptr;
    for (auto& x : g_many) if (x.device == device) r = &x;
    if (!r) { g_many.emplace_back(); r = &g_many.back(); r->device = device; }
    if (r->buf.bytes() < bytes) HIPC(r->buf.reserve(std::max<size_t>(bytes, 64 * 1024)));
    *out = r;
    return JSLP_OK;
}

extern "C" int jslpm_simplex_many(jslp_engine* const* engines, int32_t n, const int32_t* check_cycles, jslp_simplex_result* out,
                                  int32_t* status) {
    if (n < 0 || (n > 0 && (!engines || !out))) return fail(JSLP_ERR_ARG, "simplex_many: bad arguments");
    if (n == 0) return JSLP_OK;
    char idx[32];
    for (int32_t i = 0; i < n; i++) {
        snprintf(idx, sizeof idx, "%d", (int)i);
        if (!engines[i]) return fail(JSLP_ERR_STATE, "simplex_many: engine %s is null", idx);
        if (!engines[i]->uploaded) return fail(JSLP_ERR_STATE, "simplex_many: engine %s: simplex before upload", idx);
    }
    {
        std::vector<const jslp_engine*> sorted(engines, engines + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(JSLP_ERR_ARG, "simplex_many: an engine is listed twice");
    }
    const int device = engines[0]->device;
    for (int32_t i = 1; i < n; i++)
        if (engines[i]->device != device) return fail(JSLP_ERR_ARG, "simplex_many: engines on different devices");
    HIPC(hipSetDevice(device));
    if (status) for (int32_t i = 0; i < n; i++) status[i] = JSLP_OK;
    int32_t first_bad = -1; int first_rc = JSLP_OK; char first_msg[sizeof g_err];
    auto note = [&](int32_t i, int rc) {
        if (status) status[i] = rc;
        if (first_bad < 0 || i < first_bad) { first_bad = i; first_rc = rc; snprintf(first_msg, sizeof first_msg, "%s", g_err); }
    };
    // routing: the engines whose own policy runs simplex() in one workgroup with LDS selection state go into the batch
    // (plain first, then optional objectives); every other engine afterwards, through its own path
    std::vector<int32_t> plain, opt, rest;
    size_t lds_plain = 0, lds_opt = 0;
    for (int32_t i = 0; i < n; i++) {
        const jslp_engine* e = engines[i];
        const size_t lds = use_wg_single(e) ? wglds_smem(e) : 0;
        if (!lds) rest.push_back(i);
        else if (e->s.n_opt > 0) { opt.push_back(i); lds_opt = std::max(lds_opt, lds); }
        else { plain.push_back(i); lds_plain = std::max(lds_plain, lds); }
    }
    const size_t nb = plain.size() + opt.size();
    if (nb) {
        std::lock_guard<std::mutex> lk(g_many_mu);
        ManyRes* res = nullptr;
        const size_t table_bytes = (sizeof(ManyLp) * nb + 255) & ~(size_t)255;
        int rc = many_buffers(device, table_bytes + sizeof(DevState) * nb, &res);
        if (rc) return rc;
        ManyLp* h_lps = res->buf.h.as<ManyLp>();
        ManyLp* d_lps = res->buf.d.as<ManyLp>();
        DevState* h_st = reinterpret_cast<DevState*>(res->buf.h.p + table_bytes);
        DevState* d_st = reinterpret_cast<DevState*>(res->buf.d.p + table_bytes);
        std::vector<int32_t> order(plain);
        order.insert(order.end(), opt.begin(), opt.end());
        jslp_engine* const lead = engines[order[0]];
        hipStream_t s = lead->res.stream;
        for (size_t k = 0; k < nb; k++) {
            jslp_engine* e = engines[order[k]];
            e->slot0_synced = 0;
            e->abort_injected = 0;
            e->last_path = "workgroup-many";
            ManyLp& m = h_lps[k];
            m.s = e->s;
            m.check_cycles = check_cycles ? check_cycles[order[k]] : 1;
            m.iters_cap = iters_cap(e);
            m.cap_rows = e->cap_rows;
            m.pad = 0;
            if (e != lead) {  // the launch runs after whatever the member's stream holds
                HIPC(hipEventRecord(e->res.ev_end, e->res.stream));
                HIPC(hipStreamWaitEvent(s, e->res.ev_end, 0));
            }
        }
        HIPC(hipMemcpyAsync(d_lps, h_lps, sizeof(ManyLp) * nb, hipMemcpyHostToDevice, s));
        HIPC(hipEventRecord(lead->res.ev_begin, s));
        const bool dbg = debug_launch_on();
        for (int variant = 0; variant < 2; variant++) {
            const size_t cnt = variant ? opt.size() : plain.size();
            if (!cnt) continue;
            const size_t lds = variant ? lds_opt : lds_plain;
            const ManyLp* lps = d_lps + (variant ? plain.size() : 0);
            DevState* sts = d_st + (variant ? plain.size() : 0);
            // one LP: the 1024-thread latency shape; a batch: the node batches' workgroup size (LDS builds exist for 512 and 1024)
            const int shape = cnt == 1 || wg_batch_threads() == 1024 ? 1024 : 512;
            if (shape == 1024 && variant)
                hipLaunchKernelGGL((k_simplex_lds_many<1024, true>), dim3(cnt), dim3(1024), lds, s, lps, sts);
            else if (shape == 1024)
                hipLaunchKernelGGL((k_simplex_lds_many<1024, false>), dim3(cnt), dim3(1024), lds, s, lps, sts);
            else if (variant)
                hipLaunchKernelGGL((k_simplex_lds_many<512, true>), dim3(cnt), dim3(512), lds, s, lps, sts);
            else
                hipLaunchKernelGGL((k_simplex_lds_many<512, false>), dim3(cnt), dim3(512), lds, s, lps, sts);
            HIPC(hipGetLastError());
            if (dbg) fprintf(stderr, "[jslp] launch k_simplex_lds_many<%d,opt %d> n %zu lds %zu\n", shape, variant, cnt, lds);
        }
        HIPC(hipMemcpyAsync(h_st, d_st, sizeof(DevState) * nb, hipMemcpyDeviceToHost, s));
        HIPC(hipEventRecord(lead->res.ev_end, s));
        for (size_t k = 0; k < nb; k++) {  // every member's stream continues after the launch
            jslp_engine* e = engines[order[k]];
            if (e != lead) HIPC(hipStreamWaitEvent(e->res.stream, lead->res.ev_end, 0));
        }
        HIPC(hipStreamSynchronize(s));
        float ms = 0;
        if (hipEventElapsedTime(&ms, lead->res.ev_begin, lead->res.ev_end) != hipSuccess) ms = 0;
        for (size_t k = 0; k < nb; k++) {  // what jslp_engine_simplex does after run_simplex, per member
            const int32_t i = order[k];
            jslp_engine* e = engines[i];
            if (e->timing) e->total_ms += ms;
            *e->h_state = h_st[k];
            rc = state_error(*e->h_state);
            if (!rc) {
                account(e, *e->h_state, 0);
                rc = fill_result(e, *e->h_state, 0, e->evaluation, &out[i], &e->evaluation);
            }
            if (rc) note(i, rc);
        }
    }
    for (int32_t i : rest) {  // only once the batch has completed: a cooperative chip-wide launch must not meet its workgroups
        const int rc = jslp_engine_simplex(engines[i], check_cycles ? check_cycles[i] : 1, &out[i]);
        if (rc) note(i, rc);
    }
    if (first_bad >= 0) {
        snprintf(g_err, sizeof g_err, "simplex_many: LP %d: %s", (int)first_bad, first_msg);
        return first_rc;
    }
    return JSLP_OK;
}

extern "C" int jslp_engine_set_counting(jslp_engine* e, int enabled) {
    if (!e) return fail(JSLP_ERR_ARG, "set_counting: null engine");
    HIPC(hipSetDevice(e->device));
    HIPC(hipStreamSynchronize(e->res.stream));
    HIPC(e->d_cnt.reserve(sizeof(cnt_t) * CNT_ALLOC));
    HIPC(hipMemset(e->d_cnt.p, 0, sizeof(cnt_t) * CNT_ALLOC));
    e->counting = enabled ? 1 : 0;
    e->s.cnt = enabled ? e->d_cnt.as<cnt_t>() : nullptr;
    e->wc = jslp_work_counters{};
    e->resident_fallbacks = e->resident_handovers = e->resident_launches = e->resident_refusals = e->node_queue_launches = 0;
    e->resident_fetch_retries = 0;
    return JSLP_OK;
}

extern "C" int jslp_engine_get_counters(jslp_engine* e, jslp_work_counters* out) {
    if (!e || !out) return fail(JSLP_ERR_ARG, "get_counters: null pointer");
    *out = e->wc;
    out->resident_aborts = e->resident_fallbacks;
    out->resident_handovers = e->resident_handovers;
    out->resident_launches = e->resident_launches;
    out->resident_refusals = e->resident_refusals;
    out->node_queue_launches = e->node_queue_launches;
    out->resident_fetch_retries = e->resident_fetch_retries;
    if (e->d_cnt.p) {
        HIPC(hipSetDevice(e->device));
        HIPC(hipStreamSynchronize(e->res.stream));
        cnt_t c[CNT_ALLOC];
        HIPC(hipMemcpy(c, e->d_cnt.p, sizeof c, hipMemcpyDeviceToHost));
#ifdef JSLP_DEBUG_WGLDS
        {   // cycle accumulators of the LDS one-workgroup kernels (thread 0 of every workgroup, s_memtime), per section
            static const char* names[] = {"restore rows", "restore maps", "cuts", "begin + LDS load", "phase-1 row", "pricing", "column gather + ratio test",
                                          "cycle check", "gate + pivot row", "map swap + compaction", "row updates", "epilogue", "read-back", "phase-1 column"};
            const double piv = (double)std::max<long long>(1, out->pivots), nodes = (double)std::max<long long>(1, out->simplex_calls);
            fprintf(stderr, "[wglds cycles] per node (%lld nodes, %lld pivots):", (long long)out->simplex_calls, (long long)out->pivots);
            double tot = 0;
            for (int i = 0; i < 14; i++) tot += (double)c[CNT_DBG + i];
            for (int i = 0; i < 14; i++)
                fprintf(stderr, "\n  %-28s %10.0f cycles/node %9.0f cycles/pivot %5.1f %%", names[i], c[CNT_DBG + i] / nodes, c[CNT_DBG + i] / piv, 100.0 * c[CNT_DBG + i] / std::max(1.0, tot));
            fprintf(stderr, "\n  total %.0f cycles/node\n", tot / nodes);
            static const char* micro[] = {"block_min_ki", "__syncthreads", "LDS scan of H + barrier", "strided column gather + barrier", "coalesced row load + barrier",
                                          "coalesced row store + barrier"};
            for (int i = 0; i < 6; i++) fprintf(stderr, "  micro: %-34s %8.0f cycles each\n", micro[i], c[CNT_DBG + 14 + i] / nodes / 16.0);
        }
#endif
        out->gated_cells += (int64_t)c[CNT_CELLS];
        out->gated_rows += (int64_t)c[CNT_ROWS];
        out->restored_rows += (int64_t)c[CNT_RESTORED];
    }
    return JSLP_OK;
}

// ---- device pool -------------------------------------------------------------------------------------------
// One host thread per additional member: the caller stays single-threaded and synchronous, the fan-out lives in here.
// One host thread per further pool member.  A batch call hands every member its share and waits for all of them; with a condition variable
// on both sides the hand-off cost ~250 us per call on the bench box (four members: three wake-ups to start, three to finish) -- most of what a
// 0.6 ms batch call takes.  Round 5: both sides SPIN first (a worker for ~0.2 ms after its last job, the caller while its members run) and fall
// back to the condition variable only when nothing arrives: calls that follow one another -- a tree's batches, the bench's repeated batch --
// never sleep.
struct PoolWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> job;
    std::atomic<unsigned> submitted{0}, done{0};
    std::atomic<int> asleep{0}, quit{0};
    int rc = 0;
    char err[512] = {0};
    static void relax_cpu() {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    // (the sleep / wake handshake is a Dekker pattern -- the worker stores `asleep` and then loads `submitted`, submit() bumps
    //  `submitted` and then loads `asleep` -- so every access that takes part in it is seq_cst: with acquire loads in the predicate the
    //  C++ memory model allows the store and the load to pass each other and a wake-up to be lost; both sides spin for a bounded TIME
    //  -- ~0.5 ms in the worker, ~0.2 ms in the caller -- not for a number of iterations, before they give the core back)
    static bool spin_for_us(const std::chrono::steady_clock::time_point& t0, unsigned& spins, double us) {
        relax_cpu();
        return (++spins & 0xffu) != 0 || std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() < us;
    }
    void loop() {
        unsigned seen = 0;
        for (;;) {
            unsigned spins = 0;
            auto t0 = std::chrono::steady_clock::now();
            while (submitted.load(std::memory_order_seq_cst) == seen && !quit.load(std::memory_order_seq_cst)) {
                if (spin_for_us(t0, spins, 500.0)) continue;
                std::unique_lock<std::mutex> lk(mu);
                asleep.store(1, std::memory_order_seq_cst);
                cv.wait(lk, [&] { return submitted.load(std::memory_order_seq_cst) != seen || quit.load(std::memory_order_seq_cst) != 0; });
                asleep.store(0, std::memory_order_seq_cst);
                spins = 0;
                t0 = std::chrono::steady_clock::now();
            }
            if (quit.load(std::memory_order_acquire)) return;
            seen = submitted.load(std::memory_order_acquire);
            g_err[0] = 0;
            const int r = job();
            rc = r;
            snprintf(err, sizeof err, "%s", g_err);
            done.store(seen, std::memory_order_release);
        }
    }
    void submit(std::function<int()> j) {
        job = std::move(j);  // (the worker reads it only behind the acquire of `submitted`; the previous job is done: wait() returned)
        submitted.fetch_add(1, std::memory_order_seq_cst);
        if (asleep.load(std::memory_order_seq_cst)) {
            std::lock_guard<std::mutex> lk(mu);
            cv.notify_all();
        }
    }
    int wait() {
        unsigned spins = 0;
        const auto t0 = std::chrono::steady_clock::now();
        while (done.load(std::memory_order_acquire) != submitted.load(std::memory_order_acquire)) {
            if (spin_for_us(t0, spins, 200.0)) continue;
            std::this_thread::sleep_for(std::chrono::microseconds(20));  // (a long job -- a big batch, a root fan-out over a slow link: stop burning the core)
        }
        return rc;
    }
    void stop() {
        wait();
        quit.store(1, std::memory_order_seq_cst);
        {
            std::lock_guard<std::mutex> lk(mu);
            cv.notify_all();
        }
        if (th.joinable()) th.join();
    }
};

struct jslp_pool {
    std::vector<jslp_engine*> members;  // members[0] = the primary (not owned)
    std::vector<PoolWorker*> workers;   // workers[i] drives members[i] (i >= 1); the primary runs on the calling thread
    unsigned long long synced_seq = ~0ull;
    int synced = 0;
    PinBuf h_out;  // ONE pinned (portable) read-back buffer: [states | rhs | rows] for all nodes
    std::vector<std::vector<int32_t>> offs;         // per member: its cut offsets rebased to 0
};

extern "C" int jslp_pool_size(const jslp_pool* p) { return p ? (int)p->members.size() : 0; }

extern "C" void jslp_pool_destroy(jslp_pool* p) {
    if (!p) return;
    for (size_t i = 1; i < p->workers.size(); i++) {
        PoolWorker* w = p->workers[i];
        if (!w) continue;
        w->stop();
        delete w;
    }
    for (size_t i = 1; i < p->members.size(); i++) jslp_engine_destroy(p->members[i]);
    delete p;
}

extern "C" int jslp_pool_create(jslp_pool** out, jslp_engine* primary, const int32_t* devices, int32_t n_devices) {
    if (!out || !primary || !devices || n_devices < 1) return fail(JSLP_ERR_ARG, "pool_create: bad arguments");
    if (devices[0] != primary->device) return fail(JSLP_ERR_ARG, "pool_create: devices[0] must be the primary engine's device");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(JSLP_ERR_DEVICE, "pool_create: no HIP device visible");
    for (int32_t i = 0; i < n_devices; i++)
        if (devices[i] < 0 || devices[i] >= ndev) return fail(JSLP_ERR_ARG, "pool_create: device ordinal out of range");
    jslp_pool* p = new jslp_pool();
    p->members.push_back(primary);
    p->workers.push_back(nullptr);
    for (int32_t i = 1; i < n_devices; i++) {
        jslp_engine* m = nullptr;
        int rc = jslp_engine_create(&m, devices[i], primary->H0, primary->W, primary->cap_rows, primary->precision);
        if (rc) { jslp_pool_destroy(p); return rc; }
        p->members.push_back(m);
        // The root fan-out (pool_adopt_root) is a set of peer copies primary -> member: direct xGMI transfers need peer access.
        // A platform that refuses it would still run -- the runtime stages peer copies through host memory -- at a fraction of
        // the bandwidth and silently: the pool fails LOUDLY instead (JSLP_POOL_ALLOW_STAGED=1 accepts the staged copies).
        // JSLP_TEST_PEER_REFUSED=1 (tests) makes every member look refused, virtual devices included.
        static const bool test_refused = getenv("JSLP_TEST_PEER_REFUSED") && atoi(getenv("JSLP_TEST_PEER_REFUSED")) != 0;
        static const bool allow_staged = getenv("JSLP_POOL_ALLOW_STAGED") && atoi(getenv("JSLP_POOL_ALLOW_STAGED")) != 0;
        if (devices[i] != primary->device || test_refused) {
            int can = 0;
            bool ok = !test_refused && hipDeviceCanAccessPeer(&can, devices[i], primary->device) == hipSuccess && can;
            if (ok) {
                hipSetDevice(devices[i]);
                const hipError_t pe = hipDeviceEnablePeerAccess(primary->device, 0);
                ok = pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled;
            }
            (void)hipGetLastError();
            if (!ok && !allow_staged) {
                hipSetDevice(primary->device);
                jslp_pool_destroy(p);  // members created so far, their worker threads; never the primary
                char msg[160];
                snprintf(msg, sizeof msg, "pool_create: device %d cannot access device %d's memory (peer access refused); "
                         "JSLP_POOL_ALLOW_STAGED=1 accepts host-staged copies", (int)devices[i], (int)primary->device);
                return fail(JSLP_ERR_DEVICE, msg);
            }
        }
        PoolWorker* w = new PoolWorker();
        w->th = std::thread([w] { w->loop(); });
        p->workers.push_back(w);
    }
    hipSetDevice(primary->device);
    p->offs.resize(p->members.size());
    *out = p;
    return JSLP_OK;
}

// one member adopts the primary's saved root: peer copies of the snapshot + a state fix-up + restore()
static int pool_adopt_root(jslp_engine* m, const jslp_engine* src, int s_H, int s_lei) {
    HIPC(hipSetDevice(m->device));
    hipStream_t s = m->res.stream;
    if (m->n_opt != src->n_opt) {  // optional objectives travel with the root (backup.ts:37-43)
        HIPC(hipStreamSynchronize(s));
        JSLP_TRY(resize_optional_objectives(m, src->n_opt));
    }
    const int sd = src->device, dd = m->device;
    HIPC(hipMemcpyPeerAsync(m->snap_A, dd, src->snap_A, sd, sizeof(double) * (size_t)s_H * m->ld, s));
    HIPC(hipMemcpyPeerAsync(m->snap_rhs, dd, src->snap_rhs, sd, sizeof(double) * (size_t)s_H, s));
    HIPC(hipMemcpyPeerAsync(m->snap_vibr, dd, src->snap_vibr, sd, sizeof(int32_t) * (size_t)s_H, s));
    HIPC(hipMemcpyPeerAsync(m->snap_vibc, dd, src->snap_vibc, sd, sizeof(int32_t) * (size_t)m->W, s));
    HIPC(hipMemcpyPeerAsync(m->snap_rbv, dd, src->snap_rbv, sd, sizeof(int32_t) * (size_t)m->n_idx, s));
    HIPC(hipMemcpyPeerAsync(m->snap_cbv, dd, src->snap_cbv, sd, sizeof(int32_t) * (size_t)m->n_idx, s));
    HIPC(hipMemcpyPeerAsync(m->d_unr, dd, src->d_unr, sd, (size_t)m->n_idx, s));
    HIPC(hipMemcpyPeerAsync(m->d_isint, dd, src->d_isint, sd, (size_t)m->n_idx, s));
    if (src->n_opt > 0) HIPC(hipMemcpyPeerAsync(m->snap_oo, dd, src->snap_oo, sd, sizeof(double) * (size_t)m->s.oo_stride, s));
    hipLaunchKernelGGL(k_adopt_root, dim3(1), dim3(1), 0, s, m->s, s_H, s_lei);
    launch_snapshot_transpose(m);
    HIPC(hipGetLastError());
    m->uploaded = 1;
    m->has_save = 1;
    m->root_seq += 1;
    m->n_unr = src->n_unr;
    m->s.has_unr = src->n_unr > 0 ? 1 : 0;
    m->evaluation = src->evaluation;
    m->nnz = src->nnz;
    m->max_uploaded_idx = src->max_uploaded_idx;
    m->slot0_synced = 0;
    m->slots_synced = 0;
    drop_checkpoints(m);
    int rc = enqueue_restore(m, 0, 1);  // the member's live tableau = the root
    if (rc) return rc;
    HIPC(hipStreamSynchronize(s));
    return JSLP_OK;
}

static int pool_join(jslp_pool* p, int rc0) {  // wait for every worker; the first failure wins (its text becomes ours)
    int rc = rc0;
    for (size_t i = 1; i < p->workers.size(); i++) {
        const int r = p->workers[i]->wait();
        if (r && !rc) { rc = r; snprintf(g_err, sizeof g_err, "%s", p->workers[i]->err); }
    }
    return rc;
}

extern "C" int jslp_pool_sync_root(jslp_pool* p) {
    if (!p) return fail(JSLP_ERR_ARG, "pool_sync_root: null pool");
    jslp_engine* e = p->members[0];
    if (!e->uploaded || !e->has_save) return fail(JSLP_ERR_STATE, "pool_sync_root: the primary has no saved root (save() first)");
    HIPC(hipSetDevice(e->device));
    HIPC(hipStreamSynchronize(e->res.stream));
    DevState st;
    HIPC(hipMemcpy(&st, e->s.st, sizeof st, hipMemcpyDeviceToHost));
    const int s_H = st.s_H, s_lei = st.s_last_element_index;
    for (size_t i = 1; i < p->members.size(); i++) {
        jslp_engine* m = p->members[i];
        p->workers[i]->submit([m, e, s_H, s_lei] { return pool_adopt_root(m, e, s_H, s_lei); });
    }
    int rc = pool_join(p, JSLP_OK);
    hipSetDevice(e->device);
    if (rc) return rc;
    p->synced_seq = e->root_seq;
    p->synced = 1;
    return JSLP_OK;
}

// compact = 1: the watched variables' rows / RHS cells only (rhs / vibr then hold n_watch entries per node, out_stride is ignored)
static int pool_relax(jslp_pool* p, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type, const int32_t* var_index,
                      const double* value, int check_cycles, jslp_simplex_result* out, double* rhs, int32_t* vibr,
                      int32_t out_stride, int want_rhs, int want_rows, int compact = 0) {
    if (!p || n_nodes < 0 || !cut_offsets || !out) return fail(JSLP_ERR_ARG, "pool_relax_batch: null pointer");
    jslp_engine* e = p->members[0];
    if (!e->uploaded || !e->has_save) return fail(JSLP_ERR_STATE, "pool_relax_batch: the primary has no saved root (save() first)");
    if (!compact && (rhs || vibr) && out_stride < e->cap_rows) return fail(JSLP_ERR_ARG, "pool_relax_batch: out_stride < row capacity");
    if (compact) {
        if (e->n_watch <= 0) return fail(JSLP_ERR_ARG, "pool_relax_batch_watched: after jslp_pool_set_watched_variables");
        for (jslp_engine* m : p->members)
            if (m->n_watch != e->n_watch) return fail(JSLP_ERR_STATE, "pool_relax_batch_watched: the members' watched variables differ from the primary's (jslp_pool_set_watched_variables sets them all)");
    }
    if (n_nodes == 0) return JSLP_OK;
    if (cut_offsets[0] != 0) return fail(JSLP_ERR_ARG, "cuts: cut_offsets[0] must be 0");
    for (int32_t i = 0; i < n_nodes; i++)
        if (cut_offsets[i + 1] < cut_offsets[i]) return fail(JSLP_ERR_ARG, "cuts: cut_offsets must not decrease");
    int rc;
    if (!p->synced || p->synced_seq != e->root_seq) {  // the primary saved a new root since the last fan-out
        rc = jslp_pool_sync_root(p);
        if (rc) return rc;
    }
    // ONE pinned buffer for every member's outcomes, laid out for all nodes: [states | rhs | rows]
    const size_t cap = compact ? (size_t)e->n_watch : (size_t)e->cap_rows;  // entries per node in the shared buffer
    const size_t need = (size_t)n_nodes * (sizeof(DevState) + cap * 12);
    if (need > p->h_out.bytes) HIPC(p->h_out.reserve(std::max<size_t>(need, (size_t)16 * (sizeof(DevState) + cap * 12)), hipHostMallocPortable));
    DevState* g_states = p->h_out.as<DevState>();
    double* g_rhs = reinterpret_cast<double*>(p->h_out.p + (size_t)n_nodes * sizeof(DevState));
    int32_t* g_rows = reinterpret_cast<int32_t*>(p->h_out.p + (size_t)n_nodes * (sizeof(DevState) + cap * 8));
    const int M = (int)p->members.size();
    // JSLP_DEBUG_POOL=1 (diagnosis, tools/pool_handoff.py): per call, when every member's job started and ended relative to the call's entry -- what of a
    // pool call is thread hand-off (the start delays, the join after the last end) and what is the members' own work
    static const int dbg_pool = [] { const char* t = getenv("JSLP_DEBUG_POOL"); return t ? atoi(t) : 0; }();
    const auto t_call = std::chrono::steady_clock::now();
    static double dbg_t[2][64];
    auto job = [=](int mi) -> int {
        jslp_engine* m = p->members[mi];
        const int first = (int)((long long)n_nodes * mi / M), last = (int)((long long)n_nodes * (mi + 1) / M), cnt = last - first;
        struct Stamp {
            int on, mi; std::chrono::steady_clock::time_point t0;
            Stamp(int on_, int mi_, std::chrono::steady_clock::time_point t) : on(on_), mi(mi_), t0(t) { if (on && mi < 64) dbg_t[0][mi] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
            ~Stamp() { if (on && mi < 64) dbg_t[1][mi] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
        } stamp(dbg_pool, mi, t_call);
        if (cnt <= 0) return JSLP_OK;
        std::vector<int32_t>& o = p->offs[mi];
        o.resize((size_t)cnt + 1);
        const int32_t base = cut_offsets[first];
        for (int i = 0; i <= cnt; i++) o[i] = cut_offsets[first + i] - base;
        // (pinned: the member's buffers ARE this range of the pool's, through `shared`)
        const int r = relax_batch_impl(m, NodeCall{.cuts = {cnt, o.data(), type ? type + base : nullptr, var_index ? var_index + base : nullptr, value ? value + base : nullptr},
                                                   .check_cycles = check_cycles, .read_back = compact ? ReadBack::Watched : ReadBack::Full,
                                                   .want_rhs = want_rhs != 0, .want_rows = want_rows != 0, .out = out + first, .pinned = true,
                                                   .shared = {g_states + first, g_rhs + (size_t)first * cap, g_rows + (size_t)first * cap}});
        if (r) return r;
        if (compact) {  // same layout on both sides: one copy per member
            if (rhs) memcpy(rhs + (size_t)first * cap, g_rhs + (size_t)first * cap, sizeof(double) * (size_t)cnt * cap);
            if (vibr) memcpy(vibr + (size_t)first * cap, g_rows + (size_t)first * cap, sizeof(int32_t) * (size_t)cnt * cap);
            return JSLP_OK;
        }
        for (int i = first; i < last && (rhs || vibr); i++) {  // caller-owned arrays: every member copies its own range
            const size_t H = (size_t)out[i].height;
            if (rhs) memcpy(rhs + (size_t)i * out_stride, g_rhs + (size_t)i * cap, sizeof(double) * H);
            if (vibr) memcpy(vibr + (size_t)i * out_stride, g_rows + (size_t)i * cap, sizeof(int32_t) * H);
        }
        return JSLP_OK;
    };
    for (int mi = 1; mi < M; mi++) p->workers[mi]->submit([job, mi] { return job(mi); });
    rc = job(0);
    rc = pool_join(p, rc);
    if (dbg_pool) {
        const double t_join = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_call).count();
        fprintf(stderr, "[jslp] pool call, %d nodes: joined at %.1f us; members (start -> end, us):", (int)n_nodes, t_join);
        for (int mi = 0; mi < M && mi < 64; mi++) fprintf(stderr, " %.1f -> %.1f", dbg_t[0][mi], dbg_t[1][mi]);
        fprintf(stderr, "\n");
    }
    hipSetDevice(e->device);
    return rc;
}

extern "C" int jslp_pool_relax_batch(jslp_pool* p, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                     const int32_t* var_index, const double* value, int check_cycles,
                                     jslp_simplex_result* out, double* rhs, int32_t* var_index_by_row, int32_t out_stride) {
    return pool_relax(p, n_nodes, cut_offsets, type, var_index, value, check_cycles, out, rhs, var_index_by_row, out_stride,
                      rhs != nullptr, var_index_by_row != nullptr);
}

extern "C" int jslp_pool_relax_batch_pinned(jslp_pool* p, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                            const int32_t* var_index, const double* value, int check_cycles,
                                            jslp_simplex_result* out, const double** rhs, const int32_t** var_index_by_row,
                                            int32_t* out_stride) {
    int rc = pool_relax(p, n_nodes, cut_offsets, type, var_index, value, check_cycles, out, nullptr, nullptr, 0, rhs != nullptr,
                        var_index_by_row != nullptr);
    if (rc) return rc;
    const size_t cap = (size_t)p->members[0]->cap_rows;
    if (rhs) *rhs = n_nodes > 0 ? reinterpret_cast<const double*>(p->h_out.p + (size_t)n_nodes * sizeof(DevState)) : nullptr;
    if (var_index_by_row)
        *var_index_by_row = n_nodes > 0 ? reinterpret_cast<const int32_t*>(p->h_out.p + (size_t)n_nodes * (sizeof(DevState) + cap * 8)) : nullptr;
    if (out_stride) *out_stride = (int32_t)cap;
    return JSLP_OK;
}

extern "C" int jslp_pool_set_watched_variables(jslp_pool* p, const int32_t* var_indexes, int32_t n) {
    if (!p) return fail(JSLP_ERR_ARG, "pool_set_watched_variables: null pool");
    jslp_engine* e = p->members[0];
    // the members learn their dimensions' worth of state with the root: make sure they have it before they are handed index lists
    if (e->uploaded && e->has_save && (!p->synced || p->synced_seq != e->root_seq)) {
        int rc = jslp_pool_sync_root(p);
        if (rc) return rc;
    }
    for (jslp_engine* m : p->members) {
        int rc = jslp_engine_set_watched_variables(m, var_indexes, n);
        if (rc) { hipSetDevice(e->device); return rc; }
    }
    hipSetDevice(e->device);
    return JSLP_OK;
}

extern "C" int jslp_pool_relax_batch_watched(jslp_pool* p, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                             const int32_t* var_index, const double* value, int check_cycles,
                                             jslp_simplex_result* out, int32_t* watched_row, double* watched_value) {
    return pool_relax(p, n_nodes, cut_offsets, type, var_index, value, check_cycles, out, watched_value, watched_row, 0,
                      watched_value != nullptr, watched_row != nullptr, 1);
}

extern "C" int jslp_pool_relax_batch_watched_pinned(jslp_pool* p, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                                    const int32_t* var_index, const double* value, int check_cycles,
                                                    jslp_simplex_result* out, const int32_t** watched_row, const double** watched_value) {
    int rc = pool_relax(p, n_nodes, cut_offsets, type, var_index, value, check_cycles, out, nullptr, nullptr, 0, watched_value != nullptr,
                        watched_row != nullptr, 1);
    if (rc) return rc;
    const size_t nw = p && !p->members.empty() ? (size_t)p->members[0]->n_watch : 0;
    if (watched_value) *watched_value = n_nodes > 0 ? reinterpret_cast<const double*>(p->h_out.p + (size_t)n_nodes * sizeof(DevState)) : nullptr;
    if (watched_row)
        *watched_row = n_nodes > 0 ? reinterpret_cast<const int32_t*>(p->h_out.p + (size_t)n_nodes * (sizeof(DevState) + nw * 8)) : nullptr;
    return JSLP_OK;
}

extern "C" int32_t jslp_pool_watched_count(const jslp_pool* p) {
    if (!p || p->members.empty()) return 0;
    const int32_t n = p->members[0]->n_watch;
    for (const jslp_engine* m : p->members)
        if (m->n_watch != n) return -1;
    return n;
}

extern "C" int jslp_pool_set_counting(jslp_pool* p, int enabled) {
    if (!p) return fail(JSLP_ERR_ARG, "pool_set_counting: null pool");
    for (jslp_engine* m : p->members) {
        int rc = jslp_engine_set_counting(m, enabled);
        if (rc) return rc;
    }
    hipSetDevice(p->members[0]->device);
    return JSLP_OK;
}

extern "C" int jslp_pool_get_counters(jslp_pool* p, jslp_work_counters* out) {
    if (!p || !out) return fail(JSLP_ERR_ARG, "pool_get_counters: null pointer");
    jslp_work_counters sum{};
    for (jslp_engine* m : p->members) {
        jslp_work_counters c;
        int rc = jslp_engine_get_counters(m, &c);
        if (rc) return rc;
        sum.relaxations += c.relaxations; sum.simplex_calls += c.simplex_calls; sum.pivots += c.pivots;
        sum.gated_cells += c.gated_cells; sum.gated_rows += c.gated_rows; sum.restored_rows += c.restored_rows;
        sum.cut_rows += c.cut_rows; sum.height_sum += c.height_sum;
        sum.resident_aborts += c.resident_aborts; sum.resident_handovers += c.resident_handovers; sum.resident_launches += c.resident_launches;
        sum.resident_refusals += c.resident_refusals; sum.node_queue_launches += c.node_queue_launches; sum.resident_fetch_retries += c.resident_fetch_retries;
    }
    hipSetDevice(p->members[0]->device);
    *out = sum;
    return JSLP_OK;
}

extern "C" int jslp_engine_dims(const jslp_engine* e, int32_t* height, int32_t* width, int32_t* n_var_indexes) {
    if (!e) return fail(JSLP_ERR_ARG, "dims: null engine");
    if (height) {
        if (hipSetDevice(e->device) != hipSuccess) return fail(JSLP_ERR_DEVICE, "dims: hipSetDevice failed");
        if (hipStreamSynchronize(e->res.stream) != hipSuccess) return fail(JSLP_ERR_DEVICE, "dims: stream synchronisation failed");
        DevState st;
        if (hipMemcpy(&st, e->s.st, sizeof st, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(JSLP_ERR_DEVICE, "dims: state read-back failed");
        *height = e->uploaded ? st.H : e->H0;
    }
    if (width) *width = e->W;
    if (n_var_indexes) *n_var_indexes = e->n_idx;
    return JSLP_OK;
}

extern "C" int jslp_engine_download(jslp_engine* e, double* matrix, int32_t* var_index_by_row, int32_t* var_index_by_col,
                                    int32_t* row_by_var_index, int32_t* col_by_var_index) {
    if (!e || !e->uploaded) return fail(JSLP_ERR_STATE, "download before upload");
    HIPC(hipSetDevice(e->device));
    HIPC(hipStreamSynchronize(e->res.stream));
    DevState st;
    HIPC(hipMemcpy(&st, e->s.st, sizeof st, hipMemcpyDeviceToHost));
    const int H = st.H, W = e->W;
    if (matrix)
        HIPC(hipMemcpy2D(matrix, sizeof(double) * W, e->s.A, sizeof(double) * e->ld, sizeof(double) * W, H, hipMemcpyDeviceToHost));
    if (var_index_by_row) HIPC(hipMemcpy(var_index_by_row, e->s.vibr, sizeof(int32_t) * H, hipMemcpyDeviceToHost));
    if (var_index_by_col) HIPC(hipMemcpy(var_index_by_col, e->s.vibc, sizeof(int32_t) * W, hipMemcpyDeviceToHost));
    if (row_by_var_index) HIPC(hipMemcpy(row_by_var_index, e->s.rbv, sizeof(int32_t) * e->n_idx, hipMemcpyDeviceToHost));
    if (col_by_var_index) HIPC(hipMemcpy(col_by_var_index, e->s.cbv, sizeof(int32_t) * e->n_idx, hipMemcpyDeviceToHost));
    return JSLP_OK;
}

extern "C" int jslp_engine_pivot_trace(jslp_engine* e, int32_t* row_col, int64_t max_pairs, int64_t* n_pivots) {
    if (!e || !n_pivots) return fail(JSLP_ERR_ARG, "pivot_trace: null pointer");
    HIPC(hipSetDevice(e->device));
    HIPC(hipStreamSynchronize(e->res.stream));
    DevState st;
    HIPC(hipMemcpy(&st, e->s.st, sizeof st, hipMemcpyDeviceToHost));
    *n_pivots = st.trace_n;
    if (row_col && max_pairs > 0 && st.trace_n > e->s.trace_cap)
        return fail(JSLP_ERR_CAPACITY, "pivot_trace: more pivots since upload than the trace holds (2^20): the recorded prefix is not handed out as if it were complete");
    if (row_col && max_pairs > 0) {
        const long long n = std::min<long long>(std::min<long long>(st.trace_n, max_pairs), e->s.trace_cap);
        if (n > 0) HIPC(hipMemcpy(row_col, e->s.trace, sizeof(int2) * n, hipMemcpyDeviceToHost));
    }
    return JSLP_OK;
}

extern "C" const char* jslp_engine_last_path(const jslp_engine* e) { return e ? e->last_path : "none"; }

extern "C" int jslp_engine_set_timing(jslp_engine* e, int enabled) {
    if (!e) return fail(JSLP_ERR_ARG, "set_timing: null engine");
    e->timing = enabled ? 1 : 0;
    e->upd_ms = 0; e->upd_launches = 0; e->total_ms = 0;
    return JSLP_OK;
}

extern "C" int jslp_engine_get_timing(jslp_engine* e, double* update_kernel_ms, int64_t* update_kernel_launches,
                                      double* total_device_ms) {
    if (!e) return fail(JSLP_ERR_ARG, "get_timing: null engine");
    if (update_kernel_ms) *update_kernel_ms = e->upd_ms;
    if (update_kernel_launches) *update_kernel_launches = e->upd_launches;
    if (total_device_ms) *total_device_ms = e->total_ms;
    return JSLP_OK;
}

// ---- the fp32 twin as a sweep (include/jslpf_f32.h) -----------------------------------------------------------------------------
// Behind every other kernel of this translation unit: k32_simplex_lds is instantiated last.
#include "jslp_f32_lds.hip.h"

// dynamic LDS of k32_simplex_lds for this engine; 0 = its fp32 LDS state does not fit
static size_t f32lds_smem(const jslp_engine* e) {
    const size_t b = f32lds_bytes(e->ld, e->cap_rows);
    return b <= WGLDS_MAX_BYTES ? b : 0;
}
// JSLPF_PATH_AUTO: use_wg_single's rule restated for k32_simplex_lds, without the force-path knobs (the bounds were measured for
// the fp64 kernels; what the fp32 kernel measured against them: DESIGN.md section 4, profiles/f32_one_launch_times.md)
static bool f32_auto_one_launch(const jslp_engine* e) {
    if (!f32lds_smem(e)) return false;
    const long long cells = (long long)e->cap_rows * e->ld;
    if (cells <= WG_CELLS_SINGLE) return true;
    return cells <= WG_CELLS_SPARSE && e->nnz >= 0 && (double)e->nnz <= WG_SPARSE_DENSITY * (double)e->H0 * (double)e->W;
}
// what jslp_engine_simplex_f32 makes of a finished fp32 state
static void fill_f32_result(const jslp_engine* e, const DevState& st, double precision, jslp_simplex_result* out) {
    memset(out, 0, sizeof *out);
    out->feasible = st.feasible;
    out->bounded = st.bounded;
    out->optimal = st.optimal;
    out->unbounded_var_index = st.bounded ? -1 : st.unbounded_var;
    out->pivots_phase1 = st.it1;
    out->pivots_phase2 = st.entered_phase2 ? st.it2 : -1;
    out->cycle_phase = st.cycle_phase;
    out->height = st.H;
    out->obj_cell = st.obj_cell;
    out->evaluation = e->evaluation;
    if (st.optimal) {
        const double rcoef = js_round(1.0 / precision);
        out->evaluation = js_round((2.220446049250313e-16 + st.obj_cell) * rcoef) / rcoef;
    } else if (!st.bounded) {
        out->evaluation = -INFINITY;
    }
}

extern "C" int jslpf_simplex_f32_sweep(jslp_engine* e, const double* precisions, int32_t n, int check_cycles, int32_t path,
                                       jslp_simplex_result* out, double* rhs, int32_t* var_index_by_row, int32_t stride,
                                       int32_t* status, int32_t* path_taken, double* device_ms) {
    if (n < 0 || n > JSLPF_MAX_RUNS) return fail(JSLP_ERR_ARG, "simplex_f32_sweep: the number of runs must be in [0, 64]");
    if (n > 0 && (!precisions || !out)) return fail(JSLP_ERR_ARG, "simplex_f32_sweep: null pointer");
    if (path != JSLPF_PATH_AUTO && path != JSLPF_PATH_SELECT_UPDATE && path != JSLPF_PATH_ONE_LAUNCH)
        return fail(JSLP_ERR_ARG, "simplex_f32_sweep: unknown path");
    char idx[32];
    for (int32_t i = 0; i < n; i++)
        if (!(precisions[i] > 0)) {
            snprintf(idx, sizeof idx, "%d", (int)i);
            return fail(JSLP_ERR_ARG, "simplex_f32_sweep: run %s: precision must be positive", idx);
        }
    if (n == 0) return JSLP_OK;
    if (!e) return fail(JSLP_ERR_STATE, "simplex_f32_sweep: null engine");
    if (!e->uploaded) return fail(JSLP_ERR_STATE, "simplex_f32_sweep before upload");
    if (e->n_opt > 0) return fail(JSLP_ERR_UNSUPPORTED, "simplex_f32_sweep: optional objectives are not part of the fp32 experiment");
    const size_t lds = f32lds_smem(e);
    if (path == JSLPF_PATH_ONE_LAUNCH && !lds)
        return fail(JSLP_ERR_UNSUPPORTED, "simplex_f32_sweep: the tableau's fp32 LDS state does not fit one workgroup (k32_simplex_lds)");
    HIPC(hipSetDevice(e->device));
    hipStream_t s = e->res.stream;
    if (rhs || var_index_by_row) {  // the live height decides whether the caller's arrays hold a run
        HIPC(hipMemcpyAsync(e->h_state, e->s.st, sizeof(DevState), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        if (stride < e->h_state->H) return fail(JSLP_ERR_ARG, "simplex_f32_sweep: stride below the live height");
    }
    const bool one_launch = path == JSLPF_PATH_ONE_LAUNCH || (path == JSLPF_PATH_AUTO && f32_auto_one_launch(e));
    if (path_taken) *path_taken = one_launch ? JSLPF_PATH_ONE_LAUNCH : JSLPF_PATH_SELECT_UPDATE;
    if (status) for (int32_t i = 0; i < n; i++) status[i] = JSLP_OK;
    int32_t first_bad = -1; int first_rc = JSLP_OK; char first_msg[sizeof g_err];
    auto note = [&](int32_t i, int rc) {
        if (status) status[i] = rc;
        if (first_bad < 0) { first_bad = i; first_rc = rc; snprintf(first_msg, sizeof first_msg, "%s", g_err); }
    };
    double total_ms = 0;
    if (!one_launch) {
        for (int32_t i = 0; i < n; i++) {
            jslp_simplex_result r;
            double ms = 0;
            const int rc = jslp_engine_simplex_f32(e, precisions[i], check_cycles, &r, rhs ? rhs + (size_t)i * stride : nullptr,
                                                   var_index_by_row ? var_index_by_row + (size_t)i * stride : nullptr, &ms);
            if (rc) { note(i, rc); continue; }
            out[i] = r;
            total_ms = ms < 0 || total_ms < 0 ? -1.0 : total_ms + ms;
        }
    } else {
        JSLP_TRY(ensure_f32(e, n));
        JSLP_TRY(ensure_out(e, (size_t)n));
        f32::Slots& d = e->s32;
        d.unr = e->d_unr;
        d.has_unr = e->n_unr > 0 ? 1 : 0;
        F32Precisions precs{};
        for (int32_t i = 0; i < n; i++) precs.v[i] = (float)precisions[i];
        const int out_stride = (int)out_stride_of(e);
        HIPC(hipEventRecord(e->res.ev_begin, s));
        hipLaunchKernelGGL((k32_simplex_lds<JSLP_WG_THREADS>), dim3(n), dim3(JSLP_WG_THREADS), lds, s, e->s, d, precs, check_cycles ? 1 : 0,
                           iters_cap(e), (int)e->cap_rows, e->d_rhs, e->d_rows, e->d_states, out_stride);
        HIPC(hipGetLastError());
        HIPC(hipEventRecord(e->res.ev_end, s));
        if (debug_launch_on()) fprintf(stderr, "[jslp] launch k32_simplex_lds<%d> n %d lds %zu\n", JSLP_WG_THREADS, (int)n, lds);
        HIPC(hipMemcpyAsync(e->res.out.h.p, e->res.out.d.p, out_bytes(e, (size_t)n), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        float ms = 0;
        total_ms = hipEventElapsedTime(&ms, e->res.ev_begin, e->res.ev_end) == hipSuccess ? ms : -1.0;
        for (int32_t i = 0; i < n; i++) {
            const DevState st = e->h_states[i];
            const int rc = state_error(st);
            if (rc) { note(i, rc); continue; }
            fill_f32_result(e, st, precisions[i], &out[i]);
            if (rhs) memcpy(rhs + (size_t)i * stride, e->h_rhs + (size_t)i * out_stride, sizeof(double) * st.H);
            if (var_index_by_row) memcpy(var_index_by_row + (size_t)i * stride, e->h_rows + (size_t)i * out_stride, sizeof(int32_t) * st.H);
        }
    }
    if (device_ms) *device_ms = total_ms;
    if (first_bad >= 0) {
        snprintf(idx, sizeof idx, "%d", (int)first_bad);
        snprintf(g_err, sizeof g_err, "simplex_f32_sweep: run %s: %s", idx, first_msg);
        return first_rc;
    }
    return JSLP_OK;
}

// ---- a pack of small LPs solved in LDS (include/jslpp_packed.h) ---------------------------------------------------------------------
// One object, one arena: [LP images | descriptor table | launch order | per-LP checkForCycles | histories | traces].  The images have a
// pinned twin (the ONE H2D copy of upload); the result block [states | RHS columns | row maps | (tree records) | optional rows] has another
// (the ONE D2H copy of simplex).  An LP with optional objectives (include/jslps_soft.h) carries their rows in its image behind the matrix and
// runs in the OPT build of its kernel: up to four launches per call, 64 or 256 threads, each with or without OPT -- six in a pack made with
// big_lds (include/jslpb_big_lds.h), whose LPs above 64 KiB of LDS run in the large builds.
// A pack call holds no jslp_engine and takes no g_many_mu.  The kernels live in jslp_tu_packed.hip (jslp_packed.hip.h).
#include "jslp_packed.hip.h"
#include "jslp_tree.hip.h"  // (the layout of a pack with cut rows and a heap per LP, include/jslpt_tree.h)
// The units that hold the builds of the pack kernels: each launches the build (a.tree, threads, a.build) names, or answers -1 for one that is
// not its own (pack_dispatch, jslp_tree.hip.h).  The product has seven (jslp_tu_packed.hip, jslp_tu_tree_mir.hip, _enh, _inc, the two parts of
// jslp_tu_tree_tol.hip, and jslp_tu_packed_big.hip with the large builds of include/jslpb_big_lds.h); a single-unit build has this file, the
// kernels at its end.
typedef int (*PackUnit)(int threads, unsigned grid, size_t lds, const void* args, void* stream);
#ifdef JSLP_SPLIT_TU
extern "C" __attribute__((visibility("hidden"))) int jslpp_packed_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int jslpc_tree_mir_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int jslpe_tree_enh_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int jslpi_tree_inc_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int jslpg_tree_tol1_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int jslpg_tree_tol2_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int jslpb_packed_big_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream);
static constexpr PackUnit PACK_UNITS[] = {jslpp_packed_launch_tu, jslpc_tree_mir_launch_tu, jslpe_tree_enh_launch_tu, jslpi_tree_inc_launch_tu,
                                          jslpg_tree_tol1_launch_tu, jslpg_tree_tol2_launch_tu, jslpb_packed_big_launch_tu};
#else
static int pack_dispatch(int threads, unsigned grid, size_t lds, const void* bytes, void* stream);  // (jslp_tree.hip.h, at the end of this file)
static constexpr PackUnit PACK_UNITS[] = {pack_dispatch};
#endif
static int packed_launch(int threads, unsigned grid, size_t lds, const PackLaunch& a, hipStream_t s) {
    for (PackUnit unit : PACK_UNITS) {
        const int le = unit(threads, grid, lds, &a, s);
        if (le != -1) return le;
    }
    return -1;
}

// THE launch groups of a pack, in launch order: the LPs of one kind that run with one thread count, and what the launch line says behind the
// thread count.  pack_init sorts the LPs into them, pack_run launches them.  (A plain simplex has the plain and the OPT build only: it runs a
// group of MIR, enhanced or incremental LPs in the plain build of the group's thread count, and says so.)
struct PackGroup { PackKind kind; int threads; const char* suffix; bool big = false; };  // (big: the large class, whatever its thread count)
static constexpr PackGroup PACK_GROUPS[] = {{PACK_PLAIN, 64, ""},      {PACK_PLAIN, 256, ""},      {PACK_OPT, 64, ",opt 1"}, {PACK_OPT, 256, ",opt 1"},
                                            {PACK_MIR, 64, ",mir 1"},  {PACK_MIR, 256, ",mir 1"},  {PACK_ENH, 64, ",enh 1"}, {PACK_ENH, 256, ",enh 1"},
                                            {PACK_INC, 64, ",inc 1"},  {PACK_INC, 256, ",inc 1"},
                                            // (the large LPs of a pack with big_lds, include/jslpb_big_lds.h: an image above 64 KiB is a plain LP's or an OPT LP's)
                                            {PACK_PLAIN, JSLP_PACK_BIG_THREADS, "", true}, {PACK_OPT, JSLP_PACK_BIG_THREADS, ",opt 1", true}};
// The result block [states | RHS columns | row maps | (a TreeRec per LP | (a TreeMirRec per LP) | (a TreeEnhRec per LP, an incremental pack's with
// the LP's TreeIncRec behind it)) | optional rows]: the byte offset of every piece, each at a 256-byte boundary, computed ONCE at create
// (a pack with a tolerance table, include/jslpg_tree_tolerance.h: a TreeTolRec per LP behind everything else)
struct PackLayout { size_t rhs, rows, tree, mir, enh, enh_stride, opt, tol, bytes; };
static PackLayout pack_layout(size_t n, size_t n_rows, size_t opt_doubles, bool tree, bool has_mir, bool has_enh, bool has_inc, bool has_tol) {
    PackLayout l{};
    l.rhs = (sizeof(DevState) * n + 255) & ~(size_t)255;
    l.rows = (l.rhs + sizeof(double) * n_rows + 255) & ~(size_t)255;
    l.tree = (l.rows + sizeof(int32_t) * n_rows + 255) & ~(size_t)255;
    l.mir = (l.tree + sizeof(TreeRec) * n + 255) & ~(size_t)255;  // (has_mir: a TreeMirRec per LP)
    // (has_enh: a TreeEnhRec per LP, behind the MIR records when the pack has them; has_inc: LP i's TreeIncRec follows its TreeEnhRec)
    l.enh = ((has_mir ? l.mir + sizeof(TreeMirRec) * n : l.tree + sizeof(TreeRec) * n) + 255) & ~(size_t)255;
    l.enh_stride = has_inc ? sizeof(TreeEnhRec) + sizeof(TreeIncRec) : sizeof(TreeEnhRec);
    const size_t plain_bytes = has_enh ? l.enh + l.enh_stride * n
                               : has_mir ? l.mir + sizeof(TreeMirRec) * n
                               : tree  ? l.tree + sizeof(TreeRec) * n
                                       : l.rows + sizeof(int32_t) * n_rows;
    l.opt = (plain_bytes + 255) & ~(size_t)255;
    l.bytes = opt_doubles ? l.opt + sizeof(double) * opt_doubles : plain_bytes;
    l.tol = (l.bytes + 255) & ~(size_t)255;
    if (has_tol) l.bytes = l.tol + sizeof(TreeTolRec) * n;
    return l;
}
// LP i's share of d_tree_mem, from byte `heap` on: the heap, (an enhanced LP's pseudocost table behind the heap array, (an incremental LP's
// checkpoint arena behind the table,) where the kernel looks for them,) the cut-list pool, the free stack, best_opt
struct TreeCarve { size_t heap, pool, free_list, best_opt, end; };

struct jslpp_pack {
    int device = 0;
    int32_t n = 0, trace_cap = 0, hist_cap = 0;
    // stream and events: a bundle of the resource pool when it had one (handed back intact at destroy), else the pack's own
    PooledRes res;
    bool pooled = false;
    Stream own_stream;
    Event own_begin, own_end;
    hipStream_t stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    std::vector<int32_t> H, W;
    std::vector<int32_t> RC;        // rows LP i's image, LDS layout and result block are sized for: H[i], or H[i] + cut_rows[i] (jslpt_pack_create)
    // every LP's ONE kind: plain; with optional objectives (include/jslps_soft.h); a MIR LP (include/jslpc_tree_mir.h: row capacity height +
    // row_extra, a TreeMirRec in the result block); an enhanced LP (include/jslpe_tree_enhanced.h: a pseudocost table behind its heap, a
    // TreeEnhRec in the result block); an incremental LP (include/jslpi_tree_incremental.h: an enhanced LP in everything but its kernel build,
    // its row capacity height + row_extra, the checkpoint arena behind its pseudocost table and the TreeIncRec behind its TreeEnhRec)
    std::vector<PackKind> kind;
    // a pack made by jslpt_pack_create: per LP a heap and a pool of cut lists (jslp_tree.hip.h); tree_ran: the arena holds saved roots
    bool tree = false, tree_ran = false;
    int32_t max_nodes = 0;
    std::vector<int32_t> cut_rows, heap_cap;
    std::vector<int32_t> tree_status;  // the status of every LP after the last tree call (jslpc_pack_read_mir and its like)
    std::vector<int32_t> policy;       // an enhanced or incremental LP's node selection | branching << 4; 0 for every other LP
    std::vector<int32_t> max_ckpt;     // an incremental LP's max_checkpoints; 0 for every other LP
    // options.tolerance (include/jslpg_tree_tolerance.h): which LPs have one, and their 1 + tolerance or 1 - tolerance; empty: a pack without the table
    std::vector<uint8_t> has_tol;
    std::vector<double> tol_factor;
    TreeLp* d_trees = nullptr;
    char* d_tree_mem = nullptr;
    size_t tree_mem_bytes = 0;
    std::vector<double> precision, evaluation;
    std::vector<size_t> image_off;  // LP i's image in the arena / the pinned twin
    std::vector<int64_t> offs;      // LP i's RHS column / row map in the result block, n + 1 entries
    std::vector<uint8_t> is_set;
    size_t image_bytes = 0;
    DevBuf arena;
    PinBuf h_image, h_cc;
    StagePair result;
    PackLayout at;  // where the pieces of the result block lie
    char* d_image = nullptr;
    PackLp* d_lps = nullptr;
    int32_t *d_order = nullptr, *d_cc = nullptr;
    int2 *d_hist = nullptr, *d_trace = nullptr;
    // (every group twice: its LPs without a tolerance, then those with one -- slot 2 g and 2 g + 1; a tree call launches the two in the
    // build and the TOL build of the group's kind, a plain simplex launches them as one)
    static constexpr int N_GROUPS = 2 * (int)(sizeof PACK_GROUPS / sizeof PACK_GROUPS[0]);
    int32_t n_group[N_GROUPS] = {};  // LPs per launch group (d_order holds them group after group), and the largest LDS image of each
    size_t lds_group[N_GROUPS] = {};
    // optional objectives (include/jslps_soft.h): rows per LP, whether they were set, and where they lie in the result block (in doubles)
    std::vector<int32_t> n_opt;
    std::vector<uint8_t> opt_set;
    std::vector<int64_t> opt_offs;  // n + 1 entries
    bool solved = false;            // a solve since the last upload: the result block holds its rows
    int uploaded = 0;
    int32_t launches = 0;
    DevState* h_states() const { return result.h.as<DevState>(); }
    double* h_rhs() const { return reinterpret_cast<double*>(result.h.p + at.rhs); }
    int32_t* h_rows() const { return reinterpret_cast<int32_t*>(result.h.p + at.rows); }
    TreeRec* h_tree() const { return reinterpret_cast<TreeRec*>(result.h.p + at.tree); }
    TreeMirRec* h_mir() const { return reinterpret_cast<TreeMirRec*>(result.h.p + at.mir); }
    TreeTolRec* h_tol() const { return reinterpret_cast<TreeTolRec*>(result.h.p + at.tol); }
    bool is_tol(size_t i) const { return !has_tol.empty() && has_tol[i]; }
    TreeEnhRec* h_enh(size_t i) const { return reinterpret_cast<TreeEnhRec*>(result.h.p + at.enh + at.enh_stride * i); }
    bool is_mir(size_t i) const { return kind[i] == PACK_MIR; }
    bool is_enh(size_t i) const { return kind[i] == PACK_ENH || kind[i] == PACK_INC; }  // (an incremental LP is one too)
    bool is_inc(size_t i) const { return kind[i] == PACK_INC; }
    bool is_big(size_t i) const { return lds_bytes(i) > (size_t)PACK_SMALL_LDS; }  // a large LP (include/jslpb_big_lds.h; create lets none into a pack without big_lds)
    int threads(size_t i) const {  // (tableau cells at the row capacity, optional rows or not)
        return is_big(i) ? JSLP_PACK_BIG_THREADS : (long long)RC[i] * W[i] <= PACK_CELLS_WAVE ? 64 : 256;
    }
    size_t ckpt_arena_bytes(size_t i) const { return is_inc(i) ? (size_t)tree_ckpt_bytes(RC[i], W[i]) * (size_t)max_ckpt[i] : 0; }
    TreeCarve tree_carve(size_t i, size_t off) const {
        const size_t slots = (size_t)heap_cap[i] + 3;
        TreeCarve c;
        c.heap = off;
        off += sizeof(TreeEntry) * (size_t)heap_cap[i];
        if (is_enh(i)) off += (size_t)tree_pseudo_bytes(RC[i], W[i]);
        off += ckpt_arena_bytes(i);
        c.pool = off;
        off += (size_t)tree_slot_bytes(cut_rows[i]) * slots;
        c.free_list = off;
        off += (sizeof(int32_t) * slots + 15) & ~(size_t)15;
        c.best_opt = off;
        off += (sizeof(double) * (size_t)n_opt[i] + 15) & ~(size_t)15;
        c.end = off;
        return c;
    }
    size_t lds_bytes(size_t i) const { return is_mir(i) ? (size_t)tree_mir_lds_bytes(RC[i], W[i]) : (size_t)pk_lds_bytes(RC[i], W[i], n_opt[i]); }
    size_t ints_off(int32_t i) const { return sizeof(DevState) + 8 * (size_t)pk_image_doubles(RC[i], W[i], n_opt[i]); }
    size_t opt_rows_off(int32_t i) const { return sizeof(DevState) + 8 * (size_t)pk_opt_image_off(RC[i], W[i]); }
    size_t ivars_off(int32_t i) const { return ints_off(i) + 4 * (size_t)pk_ints(RC[i], W[i]).total; }
};
// An LP with a tolerance (include/jslpg_tree_tolerance.h): the three spare words of its image's integer-variable header, as jslp_tree.hip.h
// reads them -- where the TreeTolRec array lies behind the TreeRec array, in units of 256 bytes, and the factor
static void pack_write_tol_head(jslpp_pack* p, int32_t i) {
    if (!p->is_tol((size_t)i)) return;
    int32_t* v = reinterpret_cast<int32_t*>(p->h_image.p + p->image_off[i] + p->ivars_off(i));
    v[1] = (int32_t)((p->at.tol - p->at.tree) / 256);
    memcpy(v + 2, &p->tol_factor[i], sizeof(double));
}
static int pack_fail(int code, const char* what, int32_t i, const char* why) {
    snprintf(g_err, sizeof g_err, "%s: LP %d: %s", what, (int)i, why);
    return code;
}
// (H: the rows the image is sized for -- an LP's row capacity)
static size_t pack_image_bytes(int32_t H, int32_t W, int32_t n_opt) {
    return sizeof(DevState) + 8 * (size_t)pk_image_doubles(H, W, n_opt) + 4 * (size_t)pk_ints(H, W).total;
}
static_assert(sizeof(DevState) % 16 == 0, "an LP's matrix follows its DevState at a 16-byte boundary");

extern "C" int64_t jslpp_lds_bytes(int32_t height, int32_t width) {
    if (height < 2 || width < 2) return 0;
    return (int64_t)pk_lds_bytes(height, width);
}
extern "C" int64_t jslps_lds_bytes(int32_t height, int32_t width, int32_t n_optional) {
    if (height < 2 || width < 2 || n_optional < 0) return 0;
    return (int64_t)pk_lds_bytes(height, width, n_optional);
}

static void pack_carve(jslpp_pack* p, Carver& cv) {
    p->d_image = cv.take<char>(p->image_bytes);
    p->d_lps = cv.take<PackLp>((size_t)p->n);
    p->d_order = cv.take<int32_t>((size_t)p->n);
    p->d_cc = cv.take<int32_t>((size_t)p->n);
    p->d_hist = cv.take<int2>((size_t)p->n * p->hist_cap);
    p->d_trace = cv.take<int2>((size_t)p->n * p->trace_cap);
    if (p->tree) {
        p->d_trees = cv.take<TreeLp>((size_t)p->n);
        p->d_tree_mem = cv.take<char>(p->tree_mem_bytes);
    }
}
// the device side of create(): stream, events, the arena, the pinned twins, the descriptor table and the launch order (built ONCE)
static int pack_init(jslpp_pack* p, int32_t max_pivots) {
    p->pooled = pool_take(p->device, &p->res);
    if (p->pooled) {
        p->stream = p->res.stream; p->ev_begin = p->res.ev_begin; p->ev_end = p->res.ev_end;
    } else {
        HIPC(hipStreamCreateWithFlags(&p->own_stream.h, hipStreamNonBlocking));
        HIPC(hipEventCreate(&p->own_begin.h));
        HIPC(hipEventCreate(&p->own_end.h));
        p->stream = p->own_stream; p->ev_begin = p->own_begin; p->ev_end = p->own_end;
    }
    const size_t n = (size_t)p->n;
    HIPC_CARVE(p->arena, [&](Carver& cv) { pack_carve(p, cv); });
    HIPC(p->h_image.reserve(std::max<size_t>(p->image_bytes, 256)));
    memset(p->h_image.p, 0, p->image_bytes);
    if (p->tree) for (int32_t i = 0; i < p->n; i++) pack_write_tol_head(p, i);
    HIPC(p->h_cc.reserve(std::max<size_t>(sizeof(int32_t) * n, 256)));
    HIPC(p->result.reserve(std::max<size_t>(p->at.bytes, 256)));
    std::vector<PackLp> lps(n);
    std::vector<int32_t> order(n);
    int32_t k = 0;
    for (int g = 0; g < jslpp_pack::N_GROUPS; g++)  // group after group (PACK_GROUPS), each in pack order
        for (size_t i = 0; i < n; i++) {
            if (p->kind[i] != PACK_GROUPS[g / 2].kind || p->threads(i) != PACK_GROUPS[g / 2].threads || p->is_big(i) != PACK_GROUPS[g / 2].big || p->is_tol(i) != ((g & 1) != 0)) continue;
            order[k++] = (int32_t)i;
            p->n_group[g] += 1;
            p->lds_group[g] = std::max(p->lds_group[g], p->lds_bytes(i));
        }
    for (size_t i = 0; i < n; i++) {
        PackLp& m = lps[i];
        m.image = p->d_image + p->image_off[i];
        m.hist = p->d_hist + i * p->hist_cap;
        m.trace = p->d_trace + i * p->trace_cap;
        m.precision = p->precision[i];
        m.out_off = p->offs[i];
        m.H = p->H[i]; m.W = p->W[i];
        m.hist_cap = p->hist_cap; m.trace_cap = p->trace_cap;
        // the engine's iters_cap formula with its row_capacity
        m.iters_cap = max_pivots > 0 ? max_pivots : (int32_t)std::min<long long>(2000000LL + 200LL * ((long long)p->RC[i] + m.W), 2000000000LL);
        // partial pricing parameters (simplex.ts:118-127), as jslp_engine_create derives them
        const int32_t n_columns = m.W - 1;
        m.batch = std::min(500, std::max(50, (int32_t)floor(sqrt((double)n_columns))));
        m.use_partial = n_columns > m.batch * 2;
        m.RC = p->RC[i];
        m.n_opt = p->n_opt[i];
        m.opt_out = p->n_opt[i] ? reinterpret_cast<double*>(p->result.d.p + p->at.opt) + p->opt_offs[i] : nullptr;
    }
    if (p->tree && n) {  // every LP's heap, cut-list pool and free stack, carved out of one block
        std::vector<TreeLp> trees(n);
        size_t off = 0;
        for (size_t i = 0; i < n; i++) {
            TreeLp& t = trees[i];
            const TreeCarve c = p->tree_carve(i, off);
            off = c.end;
            t.heap = reinterpret_cast<TreeEntry*>(p->d_tree_mem + c.heap);
            t.pool = p->d_tree_mem + c.pool;
            t.free_list = reinterpret_cast<int32_t*>(p->d_tree_mem + c.free_list);
            t.best_opt = reinterpret_cast<double*>(p->d_tree_mem + c.best_opt);
            if (p->is_mir(i)) t.mir_out = reinterpret_cast<TreeMirRec*>(p->result.d.p + p->at.mir) + i;  // (never with optional objectives)
            t.rcoef = js_round(1.0 / p->precision[i]);
            if (p->is_enh(i)) t.enh_out = reinterpret_cast<TreeEnhRec*>(p->result.d.p + p->at.enh + p->at.enh_stride * i);  // (never with optional objectives or MIR)
            t.cut_rows = p->cut_rows[i]; t.heap_cap = p->heap_cap[i]; t.max_nodes = p->max_nodes;
            t.policy = p->is_enh(i) ? p->policy[i] | (p->is_inc(i) ? p->max_ckpt[i] << 8 : 0) : 0;
        }
        HIPC(hipMemcpyAsync(p->d_trees, trees.data(), sizeof(TreeLp) * n, hipMemcpyHostToDevice, p->stream));
        HIPC(hipStreamSynchronize(p->stream));
    }
    if (n) {
        HIPC(hipMemcpyAsync(p->d_lps, lps.data(), sizeof(PackLp) * n, hipMemcpyHostToDevice, p->stream));
        HIPC(hipMemcpyAsync(p->d_order, order.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, p->stream));
        HIPC(hipStreamSynchronize(p->stream));  // (both vectors die with this function)
    }
    return JSLP_OK;
}

// What a create entry point asks for.  tree / mir / enh / inc say which tables the entry point takes (each then non-null unless n is 0):
// cut_rows and heap_cap (include/jslpt_tree.h); row_extra (jslpc_tree_pack_create); node_selection and branching
// (include/jslpe_tree_enhanced.h); incremental and max_checkpoints (include/jslpi_tree_incremental.h).  n_optional is null for no optional
// objectives; row_extra of an entry point with enh is null for no MIR LP; an incremental LP's row_extra is its row capacity and makes no
// MIR LP of it.
struct PackSpec {
    jslpp_pack** out;
    int device;
    int32_t n;
    const int32_t *height, *width;
    const double* precision;
    int32_t trace_cap, max_pivots, max_nodes;
    bool tree, mir, enh, inc;
    const int32_t *cut_rows, *heap_cap, *n_optional, *row_extra, *node_selection, *branching, *incremental, *max_checkpoints;
    const double* tolerance;  // (include/jslpg_tree_tolerance.h; either may be null)
    const int32_t* minimize;
    bool big_lds;  // (include/jslpb_big_lds.h) the pack's limit is JSLPB_LDS_LIMIT
};
static PackSpec pack_spec(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision, int32_t trace_cap,
                          int32_t max_pivots, int32_t max_nodes) {
    PackSpec s{};
    s.out = out; s.device = device; s.n = n;
    s.height = height; s.width = width; s.precision = precision;
    s.trace_cap = trace_cap; s.max_pivots = max_pivots; s.max_nodes = max_nodes;
    return s;
}
static int pack_create(const PackSpec& s) {
    const int32_t n = s.n;
    const bool tree = s.tree;
    // ---- every refusal, before any HIP call: the entry point's own tables, `a MIR LP has no optional objectives`, the common arguments,
    // then LP after LP
    if (n > 0 && ((tree && (!s.cut_rows || !s.heap_cap)) || (s.mir && !s.row_extra) || (s.enh && (!s.node_selection || !s.branching)) ||
                  (s.inc && (!s.incremental || !s.max_checkpoints))))
        return fail(JSLP_ERR_ARG, "pack_create: bad arguments");
    if (s.n_optional && s.row_extra)
        for (int32_t i = 0; i < n; i++)
            if (s.row_extra[i] >= 0 && s.n_optional[i] > 0 && !(s.incremental && s.incremental[i])) return pack_fail(JSLP_ERR_ARG, "pack_create", i, "a MIR LP has no optional objectives");
    if (!s.out || n < 0 || (n > 0 && (!s.height || !s.width || !s.precision))) return fail(JSLP_ERR_ARG, "pack_create: bad arguments");
    if (s.trace_cap < 0 || s.max_pivots < 0 || s.max_nodes < 0) return fail(JSLP_ERR_ARG, "pack_create: negative trace_cap, max_pivots or max_nodes");
    for (int32_t i = 0; i < n; i++) {
        if (s.height[i] < 2 || s.width[i] < 2) return pack_fail(JSLP_ERR_ARG, "pack_create", i, "a tableau has at least 2 rows and 2 columns");
        if (!(s.precision[i] == s.precision[i])) return pack_fail(JSLP_ERR_ARG, "pack_create", i, "precision is not a number");
        if (tree && (s.cut_rows[i] < 0 || s.heap_cap[i] < 1 || s.heap_cap[i] > (1 << 24)))
            return pack_fail(JSLP_ERR_ARG, "pack_create", i, "cut_rows is at least 0 and heap_cap between 1 and 2^24");
        if (s.n_optional && s.n_optional[i] < 0) return pack_fail(JSLP_ERR_ARG, "pack_create", i, "n_optional is at least 0");
        if (s.incremental && (s.incremental[i] < 0 || s.incremental[i] > 1)) return pack_fail(JSLP_ERR_ARG, "pack_create", i, "incremental is 0 or 1");
        if (s.minimize && (s.minimize[i] < 0 || s.minimize[i] > 1)) return pack_fail(JSLP_ERR_ARG, "pack_create", i, "minimize is 0 (the model maximises) or 1");
        const bool inc = s.incremental && s.incremental[i];
        if (inc) {
            if (s.max_checkpoints[i] < 0 || s.max_checkpoints[i] > JSLPI_MAX_CHECKPOINTS)
                return pack_fail(JSLP_ERR_ARG, "pack_create", i, "max_checkpoints of an incremental LP is between 0 and JSLPI_MAX_CHECKPOINTS (64)");
            if (!s.row_extra || s.row_extra[i] < s.cut_rows[i])
                return pack_fail(JSLP_ERR_ARG, "pack_create", i, "row_extra of an incremental LP is its row capacity beyond height: at least its cut_rows");
            if (s.n_optional && s.n_optional[i] > 0)
                return pack_fail(JSLP_ERR_ARG, "pack_create", i, "an incremental LP has no optional objectives (a checkpoint carries none) and no MIR cuts");
        }
        const bool mir = !inc && s.row_extra && s.row_extra[i] >= 0;
        if (s.node_selection) {
            if (s.node_selection[i] < 0 || s.node_selection[i] > 3) return pack_fail(JSLP_ERR_ARG, "pack_create", i, "node_selection is 0 (the default service), 1 best-first, 2 depth-first or 3 hybrid");
            if (s.branching[i] < 0 || s.branching[i] > 3) return pack_fail(JSLP_ERR_ARG, "pack_create", i, "branching is 0 (the default service), 1 most-fractional, 2 pseudocost or 3 strong");
            if ((s.node_selection[i] || s.branching[i]) && (mir || (s.n_optional && s.n_optional[i] > 0)))
                return pack_fail(JSLP_ERR_ARG, "pack_create", i, "an enhanced LP (node_selection / branching) has neither MIR cuts (row_extra) nor optional objectives");
        }
        if (mir && s.row_extra[i] < s.cut_rows[i])
            return pack_fail(JSLP_ERR_ARG, "pack_create", i, "row_extra of a MIR LP is at least its cut_rows (a negative one makes a plain tree LP)");
        const long long rc = (long long)s.height[i] + (mir || inc ? s.row_extra[i] : tree ? s.cut_rows[i] : 0);
        const long long no = s.n_optional ? s.n_optional[i] : 0;
        if (s.big_lds) {  // (include/jslpb_big_lds.h) the large builds are the default service's: every other kind keeps the 64 KiB rule
            const bool enh = s.node_selection && (s.node_selection[i] || s.branching[i]);
            const bool tol = s.tolerance && s.tolerance[i] > 0;
            const bool own = mir || inc || enh || tol;  // (its kind has no large build)
            const long long limit = own ? JSLPP_LDS_LIMIT : JSLPB_LDS_LIMIT;
            if ((rc + no) * s.width[i] > limit / 8 ||
                (mir ? tree_mir_lds_bytes((int32_t)rc, s.width[i]) : pk_lds_bytes((int32_t)rc, s.width[i], (int32_t)no)) > limit)
                return pack_fail(JSLP_ERR_UNSUPPORTED, "pack_create", i,
                                 mir ? "the MIR LP's LDS image at its row capacity exceeds 64 KiB (jslpc_tree_lds_bytes; the large builds of jslpb_big_lds.h hold no MIR LP): a smaller row_extra, or solve it through a jslp_engine" :
                                 inc ? "the incremental LP's LDS image at its row capacity exceeds 64 KiB (jslpi_tree_lds_bytes; the large builds of jslpb_big_lds.h hold no incremental LP): a smaller row_extra, or solve it through a jslp_engine" :
                                 enh ? "the enhanced LP's LDS image at its row capacity exceeds 64 KiB (jslpt_lds_bytes; the large builds of jslpb_big_lds.h hold no enhanced LP): fewer cut rows, or solve it through a jslp_engine" :
                                 tol ? "the LDS image of the LP with a tolerance exceeds 64 KiB at its row capacity (the large builds of jslpb_big_lds.h hold no LP with a tolerance): fewer cut rows, or solve it through a jslp_engine" :
                                 tree ? "the tableau's LDS image at its row capacity exceeds JSLPB_LDS_LIMIT, 156 KiB (jslpt_lds_bytes): fewer cut rows, or solve it through a jslp_engine"
                                      : "the tableau's LDS image exceeds JSLPB_LDS_LIMIT, 156 KiB (jslpp_lds_bytes): solve it through a jslp_engine");
            continue;
        }
        // (cells beyond the limit first: the byte count of an absurd shape must not overflow before it is compared)
        if (mir && ((rc + no) * s.width[i] > JSLPP_LDS_LIMIT / 8 || tree_mir_lds_bytes((int32_t)rc, s.width[i]) > (long long)WGLDS_MAX_BYTES))
            return pack_fail(JSLP_ERR_UNSUPPORTED, "pack_create", i,
                             "the MIR LP's LDS image at its row capacity exceeds 64 KiB (jslpc_tree_lds_bytes): a smaller row_extra, or solve it through a jslp_engine");
        if ((rc + no) * s.width[i] > JSLPP_LDS_LIMIT / 8 || pk_lds_bytes((int32_t)rc, s.width[i], (int32_t)no) > (long long)WGLDS_MAX_BYTES)
            return pack_fail(JSLP_ERR_UNSUPPORTED, "pack_create", i,
                             inc ? "the incremental LP's LDS image at its row capacity exceeds 64 KiB (jslpi_tree_lds_bytes): a smaller row_extra, or solve it through a jslp_engine" :
                             tree ? "the tableau's LDS image at its row capacity exceeds 64 KiB (jslpt_lds_bytes): fewer cut rows, or solve it through a jslp_engine"
                                  : "the tableau's LDS image exceeds 64 KiB (jslpp_lds_bytes): solve it through a jslp_engine");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(JSLP_ERR_DEVICE, "pack_create: no HIP device visible (this engine has no CPU fallback)");
    if (s.device < 0 || s.device >= ndev) return fail(JSLP_ERR_ARG, "pack_create: device ordinal out of range");
    HIPC(hipSetDevice(s.device));
    if (s.big_lds) {  // a large LP's workgroup takes (nearly) all of a compute unit's LDS: the device must have 160 KiB per workgroup
        int per_block = 0;
        HIPC(hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, s.device));
        if (per_block < PACK_CU_LDS) {
            snprintf(g_err, sizeof g_err, "pack_create: device %d offers %d bytes of LDS to a workgroup: big_lds needs 163840 (include/jslpb_big_lds.h)", s.device, per_block);
            return JSLP_ERR_UNSUPPORTED;
        }
    }
    jslpp_pack* p = new jslpp_pack();
    p->device = s.device; p->n = n; p->trace_cap = s.trace_cap;
    p->hist_cap = s.max_pivots > 0 ? std::min<int32_t>(s.max_pivots, JSLPP_HIST_CAP) : JSLPP_HIST_CAP;
    p->H.assign(s.height, s.height + n); p->W.assign(s.width, s.width + n); p->precision.assign(s.precision, s.precision + n);
    p->RC = p->H;
    p->tree = tree;
    if (s.n_optional) p->n_opt.assign(s.n_optional, s.n_optional + n); else p->n_opt.assign((size_t)n, 0);
    p->opt_set.assign((size_t)n, 0);
    p->opt_offs.assign((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; i++) p->opt_offs[i + 1] = p->opt_offs[i] + (int64_t)p->n_opt[i] * s.width[i];
    p->kind.resize((size_t)n);
    for (int32_t i = 0; i < n; i++)  // (the refusals above leave an LP at most one of the four)
        p->kind[i] = tree && s.incremental && s.incremental[i]                             ? PACK_INC
                     : tree && s.node_selection && (s.node_selection[i] || s.branching[i]) ? PACK_ENH
                     : tree && s.row_extra && s.row_extra[i] >= 0                          ? PACK_MIR
                     : p->n_opt[i] > 0                                                     ? PACK_OPT
                                                                                           : PACK_PLAIN;
    if (tree) {
        p->cut_rows.assign(s.cut_rows, s.cut_rows + n); p->heap_cap.assign(s.heap_cap, s.heap_cap + n);
        p->max_nodes = s.max_nodes > 0 ? s.max_nodes : JSLPT_MAX_NODES_DEFAULT;
        p->policy.assign((size_t)n, 0);
        p->max_ckpt.assign((size_t)n, 0);
        for (int32_t i = 0; i < n; i++) {
            if (p->is_inc((size_t)i)) p->max_ckpt[i] = s.max_checkpoints[i];
            if (p->is_enh((size_t)i))  // an LP with exactly one of the two set gets the other's default, hybrid / pseudocost (main.ts:76-77)
                p->policy[i] = (s.node_selection[i] ? s.node_selection[i] : (int32_t)ENH_HYBRID) | (s.branching[i] ? s.branching[i] : (int32_t)ENH_PSEUDOCOST) << 4;
            p->RC[i] = s.height[i] + (p->is_mir((size_t)i) || p->is_inc((size_t)i) ? s.row_extra[i] : s.cut_rows[i]);
            p->tree_mem_bytes = p->tree_carve((size_t)i, p->tree_mem_bytes).end;
        }
        if (s.tolerance) {  // `tolerance > 0` decides (false for NaN); the factor as branch-and-cut.ts:77-81 computes it
            p->has_tol.assign((size_t)n, 0);
            p->tol_factor.assign((size_t)n, 0.0);
            for (int32_t i = 0; i < n; i++) {
                if (!(s.tolerance[i] > 0)) continue;
                p->has_tol[i] = 1;
                p->tol_factor[i] = (!s.minimize || s.minimize[i]) ? 1 + s.tolerance[i] : 1 - s.tolerance[i];
            }
        }
    }
    p->evaluation.assign((size_t)n, 0.0);
    p->is_set.assign((size_t)n, 0);
    p->image_off.resize((size_t)n);
    p->offs.resize((size_t)n + 1);
    p->offs[0] = 0;
    for (int32_t i = 0; i < n; i++) {
        p->image_off[i] = p->image_bytes;
        p->image_bytes += pack_image_bytes(p->RC[i], s.width[i], p->n_opt[i]) + (tree ? (size_t)tree_ivars_bytes(p->RC[i], s.width[i]) : 0);
        p->offs[i + 1] = p->offs[i] + p->RC[i];
    }
    // (a pack whose entry point takes the table has the records, whichever LPs use them)
    p->at = pack_layout((size_t)n, (size_t)p->offs[n], (size_t)p->opt_offs[n], tree, tree && (s.mir || s.row_extra), tree && s.enh, tree && s.inc, tree && s.tolerance);
    const int rc = pack_init(p, s.max_pivots);
    if (rc) { jslpp_pack_destroy(p); return rc; }
    *s.out = p;
    return JSLP_OK;
}
extern "C" int jslpp_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                 int32_t trace_cap, int32_t max_pivots) {
    return jslps_pack_create(out, device, n, height, width, precision, nullptr, trace_cap, max_pivots);
}
extern "C" int jslps_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                 const int32_t* n_optional, int32_t trace_cap, int32_t max_pivots) {
    PackSpec s = pack_spec(out, device, n, height, width, precision, trace_cap, max_pivots, 0);
    s.n_optional = n_optional;
    return pack_create(s);
}
extern "C" int jslpt_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                 const int32_t* cut_rows, const int32_t* heap_cap, int32_t trace_cap, int32_t max_pivots, int32_t max_nodes) {
    return jslps_tree_pack_create(out, device, n, height, width, precision, cut_rows, heap_cap, nullptr, trace_cap, max_pivots, max_nodes);
}
extern "C" int jslps_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                      const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, int32_t trace_cap,
                                      int32_t max_pivots, int32_t max_nodes) {
    PackSpec s = pack_spec(out, device, n, height, width, precision, trace_cap, max_pivots, max_nodes);
    s.tree = true; s.cut_rows = cut_rows; s.heap_cap = heap_cap;
    s.n_optional = n_optional;
    return pack_create(s);
}
extern "C" int jslpc_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                      const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* row_extra, int32_t trace_cap,
                                      int32_t max_pivots, int32_t max_nodes) {
    PackSpec s = pack_spec(out, device, n, height, width, precision, trace_cap, max_pivots, max_nodes);
    s.tree = true; s.cut_rows = cut_rows; s.heap_cap = heap_cap;
    s.mir = true; s.row_extra = row_extra;
    return pack_create(s);
}
// include/jslpe_tree_enhanced.h
extern "C" int jslpe_tree_pack_create_mixed(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                            const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, const int32_t* row_extra,
                                            const int32_t* node_selection, const int32_t* branching, int32_t trace_cap, int32_t max_pivots,
                                            int32_t max_nodes) {
    PackSpec s = pack_spec(out, device, n, height, width, precision, trace_cap, max_pivots, max_nodes);
    s.tree = true; s.cut_rows = cut_rows; s.heap_cap = heap_cap;
    s.n_optional = n_optional; s.row_extra = row_extra;
    s.enh = true; s.node_selection = node_selection; s.branching = branching;
    return pack_create(s);
}
extern "C" int jslpe_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                      const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* node_selection, const int32_t* branching,
                                      int32_t trace_cap, int32_t max_pivots, int32_t max_nodes) {
    return jslpe_tree_pack_create_mixed(out, device, n, height, width, precision, cut_rows, heap_cap, nullptr, nullptr, node_selection, branching, trace_cap,
                                        max_pivots, max_nodes);
}
// include/jslpi_tree_incremental.h
extern "C" int jslpi_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                      const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, const int32_t* row_extra,
                                      const int32_t* node_selection, const int32_t* branching, const int32_t* incremental,
                                      const int32_t* max_checkpoints, int32_t trace_cap, int32_t max_pivots, int32_t max_nodes) {
    PackSpec s = pack_spec(out, device, n, height, width, precision, trace_cap, max_pivots, max_nodes);
    s.tree = true; s.cut_rows = cut_rows; s.heap_cap = heap_cap;
    s.n_optional = n_optional; s.row_extra = row_extra;
    s.enh = true; s.node_selection = node_selection; s.branching = branching;
    s.inc = true; s.incremental = incremental; s.max_checkpoints = max_checkpoints;
    return pack_create(s);
}
// include/jslpg_tree_tolerance.h
extern "C" int jslpg_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                      const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, const int32_t* row_extra,
                                      const int32_t* node_selection, const int32_t* branching, const int32_t* incremental,
                                      const int32_t* max_checkpoints, const double* tolerance, const int32_t* minimize, int32_t trace_cap,
                                      int32_t max_pivots, int32_t max_nodes) {
    PackSpec s = pack_spec(out, device, n, height, width, precision, trace_cap, max_pivots, max_nodes);
    s.tree = true; s.cut_rows = cut_rows; s.heap_cap = heap_cap;
    s.n_optional = n_optional; s.row_extra = row_extra;
    s.enh = true; s.node_selection = node_selection; s.branching = branching;
    s.inc = true; s.incremental = incremental; s.max_checkpoints = max_checkpoints;
    s.tolerance = tolerance; s.minimize = minimize;
    return pack_create(s);
}
// include/jslpb_big_lds.h
static_assert(JSLPB_LDS_LIMIT == PACK_BIG_LDS && JSLPP_LDS_LIMIT == PACK_SMALL_LDS, "the headers' limits are the kernels' (jslp_packed.hip.h)");
extern "C" int jslpb_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                 const int32_t* n_optional, int32_t trace_cap, int32_t max_pivots, int32_t big_lds) {
    if (big_lds == 0) return jslps_pack_create(out, device, n, height, width, precision, n_optional, trace_cap, max_pivots);
    if (big_lds != 1) return fail(JSLP_ERR_ARG, "pack_create: big_lds is 0 or 1");
    PackSpec s = pack_spec(out, device, n, height, width, precision, trace_cap, max_pivots, 0);
    s.n_optional = n_optional;
    s.big_lds = true;
    return pack_create(s);
}
extern "C" int jslpb_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                      const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, const int32_t* row_extra,
                                      const int32_t* node_selection, const int32_t* branching, const int32_t* incremental,
                                      const int32_t* max_checkpoints, const double* tolerance, const int32_t* minimize, int32_t trace_cap,
                                      int32_t max_pivots, int32_t max_nodes, int32_t big_lds) {
    if (big_lds == 0)
        return jslpg_tree_pack_create(out, device, n, height, width, precision, cut_rows, heap_cap, n_optional, row_extra, node_selection, branching, incremental,
                                      max_checkpoints, tolerance, minimize, trace_cap, max_pivots, max_nodes);
    if (big_lds != 1) return fail(JSLP_ERR_ARG, "pack_create: big_lds is 0 or 1");
    PackSpec s = pack_spec(out, device, n, height, width, precision, trace_cap, max_pivots, max_nodes);
    s.tree = true; s.cut_rows = cut_rows; s.heap_cap = heap_cap;
    s.n_optional = n_optional; s.row_extra = row_extra;
    s.enh = true; s.node_selection = node_selection; s.branching = branching;
    s.inc = true; s.incremental = incremental; s.max_checkpoints = max_checkpoints;
    s.tolerance = tolerance; s.minimize = minimize;
    s.big_lds = true;
    return pack_create(s);
}
extern "C" int32_t jslpb_pack_big_threads(void) { return JSLP_PACK_BIG_THREADS; }
extern "C" int64_t jslpi_tree_lds_bytes(int32_t height, int32_t width, int32_t row_capacity) { return jslpt_lds_bytes(height, width, row_capacity); }
extern "C" int64_t jslpi_checkpoint_bytes(int32_t height, int32_t width, int32_t row_capacity) {
    if (height < 2 || width < 2 || row_capacity < height) return 0;
    return (int64_t)tree_ckpt_bytes(row_capacity, width);
}
// what the three record read-backs ask first (`what`: the function, as its messages name it)
static int pack_read_check(const jslpp_pack* p, const void* out, const char* what, const char* not_a_tree_pack) {
    if (!p || (p->n > 0 && !out)) return fail(JSLP_ERR_ARG, "%s: bad arguments", what);
    if (!p->tree) return fail(JSLP_ERR_STATE, "%s: %s", what, not_a_tree_pack);
    if (!p->uploaded || !p->tree_ran) return fail(JSLP_ERR_STATE, "%s before jslpt_pack_branch_and_cut", what);
    if ((int32_t)p->tree_status.size() != p->n) return fail(JSLP_ERR_STATE, "%s: the last jslpt_pack_branch_and_cut did not finish", what);
    return JSLP_OK;
}
extern "C" int jslpg_pack_read_tolerance(jslpp_pack* p, jslpg_tolerance_result* out) {
    JSLP_TRY(pack_read_check(p, out, "pack_read_tolerance", "not a pack with trees (jslpg_tree_pack_create, jslpt_pack_create)"));
    static_assert(sizeof(jslpg_tolerance_result) == 32 && sizeof(TreeTolRec) == 32, "jslpg_tolerance_result is a TreeTolRec");
    for (int32_t i = 0; i < p->n; i++) {
        if (p->tree_status[(size_t)i] != JSLP_OK) continue;  // (left as it was)
        memset(&out[i], 0, sizeof out[i]);
        if (p->is_tol((size_t)i)) memcpy(&out[i], &p->h_tol()[i], sizeof out[i]);
        if (out[i].threshold != out[i].threshold) out[i].threshold = std::numeric_limits<double>::quiet_NaN();  // (0 * Infinity: THE quiet NaN, whatever sign the multiplier gave it)
    }
    return JSLP_OK;
}
extern "C" int jslpi_pack_read_incremental(jslpp_pack* p, jslpi_tree_result* out) {
    JSLP_TRY(pack_read_check(p, out, "pack_read_incremental", "not a pack with trees (jslpi_tree_pack_create, jslpt_pack_create)"));
    static_assert(sizeof(jslpi_tree_result) == 32 && sizeof(TreeIncRec) == 32 && sizeof(TreeCkptHead) == 16, "jslpi_tree_result is a TreeIncRec");
    static_assert(JSLPI_MAX_CHECKPOINTS == TREE_MAX_CHECKPOINTS, "include/jslpi_tree_incremental.h and jslp_tree.hip.h agree");
    for (int32_t i = 0; i < p->n; i++) {
        if (p->tree_status[(size_t)i] != JSLP_OK) continue;  // (left as it was)
        memset(&out[i], 0, sizeof out[i]);
        if (p->is_inc((size_t)i)) memcpy(&out[i], p->h_enh((size_t)i) + 1, sizeof out[i]);  // (the TreeIncRec behind the LP's TreeEnhRec)
    }
    return JSLP_OK;
}
extern "C" int jslpe_pack_read_enhanced(jslpp_pack* p, jslpe_tree_result* out) {
    JSLP_TRY(pack_read_check(p, out, "pack_read_enhanced", "not a pack with trees (jslpe_tree_pack_create, jslpt_pack_create)"));
    static_assert(sizeof(jslpe_tree_result) == 32 && sizeof(TreeEnhRec) == 32 && sizeof(TreePseudo) == 32, "jslpe_tree_result is a TreeEnhRec");
    static_assert(JSLPE_BEST_FIRST == ENH_BEST_FIRST && JSLPE_DEPTH_FIRST == ENH_DEPTH_FIRST && JSLPE_HYBRID == ENH_HYBRID && JSLPE_MOST_FRACTIONAL == ENH_MOST_FRACTIONAL &&
                      JSLPE_PSEUDOCOST == ENH_PSEUDOCOST && JSLPE_STRONG == ENH_STRONG,
                  "include/jslpe_tree_enhanced.h and jslp_tree.hip.h agree");
    for (int32_t i = 0; i < p->n; i++) {
        if (p->tree_status[(size_t)i] != JSLP_OK) continue;  // (left as it was)
        memset(&out[i], 0, sizeof out[i]);
        if (p->is_enh((size_t)i)) memcpy(&out[i], p->h_enh((size_t)i), sizeof out[i]);
    }
    return JSLP_OK;
}
extern "C" int64_t jslpc_tree_lds_bytes(int32_t height, int32_t width, int32_t row_capacity) {
    if (height < 2 || width < 2 || row_capacity < height) return 0;
    return (int64_t)tree_mir_lds_bytes(row_capacity, width);
}
extern "C" int jslpc_pack_read_mir(jslpp_pack* p, jslpc_mir_result* out) {
    JSLP_TRY(pack_read_check(p, out, "pack_read_mir", "not a pack made by jslpc_tree_pack_create or jslpt_pack_create"));
    static_assert(sizeof(jslpc_mir_result) == 20 && sizeof(TreeMirRec) == 32, "jslpc_mir_result is the head of a TreeMirRec");
    static_assert(TMIR_MAX_ROUNDS == JSLPR_MAX_ROUNDS, "include/jslpr_mir.h and jslp_tree.hip.h agree");
    for (int32_t i = 0; i < p->n; i++) {
        if (p->tree_status[(size_t)i] != JSLP_OK) continue;  // (left as it was)
        memset(&out[i], 0, sizeof out[i]);
        if (p->is_mir((size_t)i)) memcpy(&out[i], &p->h_mir()[i], sizeof out[i]);
    }
    return JSLP_OK;
}
extern "C" int64_t jslpt_lds_bytes(int32_t height, int32_t width, int32_t row_capacity) {
    if (height < 2 || width < 2 || row_capacity < height) return 0;
    return (int64_t)pk_lds_bytes(row_capacity, width);
}
extern "C" int64_t jslps_tree_lds_bytes(int32_t height, int32_t width, int32_t row_capacity, int32_t n_optional) {
    if (height < 2 || width < 2 || row_capacity < height || n_optional < 0) return 0;
    return (int64_t)pk_lds_bytes(row_capacity, width, n_optional);
}
extern "C" int jslps_pack_set_optional_objectives(jslpp_pack* p, int32_t i, const double* rows) {
    if (!p) return fail(JSLP_ERR_ARG, "pack_set_optional_objectives: null pack");
    if (i < 0 || i >= p->n) return fail(JSLP_ERR_ARG, "pack_set_optional_objectives: no such LP");
    if (p->n_opt[i] == 0) return pack_fail(JSLP_ERR_ARG, "pack_set_optional_objectives", i, "created without optional objectives (n_optional)");
    if (!rows) return pack_fail(JSLP_ERR_ARG, "pack_set_optional_objectives", i, "null rows");
    memcpy(p->h_image.p + p->image_off[i] + p->opt_rows_off(i), rows, sizeof(double) * (size_t)p->n_opt[i] * p->W[i]);
    p->opt_set[i] = 1;
    p->uploaded = 0;  // (the device copy is stale until the next upload)
    return JSLP_OK;
}
extern "C" int jslps_pack_get_optional_objectives(jslpp_pack* p, int32_t i, double* rows, int32_t* n_out) {
    if (!p) return fail(JSLP_ERR_ARG, "pack_get_optional_objectives: null pack");
    if (i < 0 || i >= p->n) return fail(JSLP_ERR_ARG, "pack_get_optional_objectives: no such LP");
    if (!p->uploaded || !p->solved) return fail(JSLP_ERR_STATE, "pack_get_optional_objectives before a solve: the result block holds no rows yet");
    if (n_out) *n_out = p->n_opt[i];
    if (rows && p->n_opt[i])
        memcpy(rows, reinterpret_cast<const double*>(p->result.h.p + p->at.opt) + p->opt_offs[i], sizeof(double) * (size_t)p->n_opt[i] * p->W[i]);
    return JSLP_OK;
}
extern "C" int jslpt_pack_set_integers(jslpp_pack* p, int32_t i, const int32_t* var_indexes, int32_t n) {
    if (!p) return fail(JSLP_ERR_ARG, "pack_set_integers: null pack");
    if (!p->tree) return fail(JSLP_ERR_STATE, "pack_set_integers: not a pack made by jslpt_pack_create");
    if (i < 0 || i >= p->n) return fail(JSLP_ERR_ARG, "pack_set_integers: no such LP");
    const int32_t n_idx = pk_n_idx(p->RC[i], p->W[i]);
    if (n < 0 || n > n_idx || (n > 0 && !var_indexes)) return pack_fail(JSLP_ERR_ARG, "pack_set_integers", i, "bad integer variable list");
    for (int32_t k = 0; k < n; k++)
        if (var_indexes[k] < 0 || var_indexes[k] >= n_idx) return pack_fail(JSLP_ERR_ARG, "pack_set_integers", i, "integer variable index out of range");
    if (p->is_enh((size_t)i)) {  // (the pseudocost table has one entry per list position: the reference's has one per variable index)
        std::vector<int32_t> sorted(var_indexes, var_indexes + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return pack_fail(JSLP_ERR_ARG, "pack_set_integers", i, "the integer variables of an enhanced LP are distinct");
    }
    int32_t* v = reinterpret_cast<int32_t*>(p->h_image.p + p->image_off[i] + p->ivars_off(i));
    memset(v, 0, (size_t)tree_ivars_bytes(p->RC[i], p->W[i]));
    v[0] = n;
    if (n) memcpy(v + 4, var_indexes, sizeof(int32_t) * (size_t)n);
    pack_write_tol_head(p, i);
    p->uploaded = 0;  // (the device copy is stale until the next upload)
    return JSLP_OK;
}

extern "C" void jslpp_pack_destroy(jslpp_pack* p) {
    if (!p) return;
    hipSetDevice(p->device);
    if (p->stream) hipStreamSynchronize(p->stream);
    if (p->pooled && p->res.complete()) pool_give(std::move(p->res));  // the bundle goes back as it came
    delete p;
}

extern "C" int32_t jslpp_pack_size(const jslpp_pack* p) { return p ? p->n : 0; }
extern "C" int32_t jslpp_pack_launches(const jslpp_pack* p) { return p ? p->launches : 0; }

extern "C" int jslpp_pack_host_matrix(jslpp_pack* p, int32_t i, double** matrix, int64_t* n_doubles) {
    if (!p || !matrix) return fail(JSLP_ERR_ARG, "pack_host_matrix: null pointer");
    if (i < 0 || i >= p->n) return fail(JSLP_ERR_ARG, "pack_host_matrix: no such LP");
    double* m = reinterpret_cast<double*>(p->h_image.p + p->image_off[i] + sizeof(DevState));
    memset(m, 0, sizeof(double) * (size_t)p->H[i] * p->W[i]);  // a fresh Float64Array is zero-filled (tableau.ts:304)
    *matrix = m;
    if (n_doubles) *n_doubles = (int64_t)p->H[i] * p->W[i];
    return JSLP_OK;
}

extern "C" int jslpp_pack_set(jslpp_pack* p, int32_t i, const double* matrix, const int32_t* var_index_by_row, const int32_t* var_index_by_col,
                              const int32_t* unrestricted_var_indexes, int32_t n_unrestricted) {
    if (!p || !var_index_by_row || !var_index_by_col) return fail(JSLP_ERR_ARG, "pack_set: null pointer");
    if (i < 0 || i >= p->n) return fail(JSLP_ERR_ARG, "pack_set: no such LP");
    if (n_unrestricted < 0 || (n_unrestricted > 0 && !unrestricted_var_indexes)) return pack_fail(JSLP_ERR_ARG, "pack_set", i, "bad unrestricted list");
    const int32_t H = p->H[i], W = p->W[i], RC = p->RC[i], n_idx = pk_n_idx(RC, W);
    for (int32_t r = 1; r < H; r++)
        if (var_index_by_row[r] < 0 || var_index_by_row[r] >= n_idx) return pack_fail(JSLP_ERR_ARG, "pack_set", i, "row variable index out of range");
    for (int32_t c = 1; c < W; c++)
        if (var_index_by_col[c] < 0 || var_index_by_col[c] >= n_idx) return pack_fail(JSLP_ERR_ARG, "pack_set", i, "column variable index out of range");
    for (int32_t k = 0; k < n_unrestricted; k++)
        if (unrestricted_var_indexes[k] < 0 || unrestricted_var_indexes[k] >= n_idx)
            return pack_fail(JSLP_ERR_ARG, "pack_set", i, "unrestricted variable index out of range");
    char* img = p->h_image.p + p->image_off[i];
    double* m = reinterpret_cast<double*>(img + sizeof(DevState));
    if (matrix && matrix != m) memcpy(m, matrix, sizeof(double) * (size_t)H * W);
    // the integer block, as k_upload_finish builds an engine's: the maps, their inverses, the unrestricted flags
    const PackInts io = pk_ints(RC, W);
    int32_t* ints = reinterpret_cast<int32_t*>(img + p->ints_off(i));
    memset(ints, 0, 4 * (size_t)io.total);
    int32_t *vibr = ints + io.vibr, *vibc = ints + io.vibc, *rbv = ints + io.rbv, *cbv = ints + io.cbv;
    uint8_t* unr = reinterpret_cast<uint8_t*>(ints + io.unr);
    for (int32_t k = 0; k < n_idx; k++) { rbv[k] = -1; cbv[k] = -1; }
    vibr[0] = -1; vibc[0] = -1;
    for (int32_t r = 1; r < H; r++) { vibr[r] = var_index_by_row[r]; rbv[vibr[r]] = r; }
    for (int32_t c = 1; c < W; c++) { vibc[c] = var_index_by_col[c]; cbv[vibc[c]] = c; }
    for (int32_t k = 0; k < n_unrestricted; k++) unr[unrestricted_var_indexes[k]] = 1;
    p->is_set[i] = 1;
    return JSLP_OK;
}

extern "C" int jslpp_pack_upload(jslpp_pack* p) {
    if (!p) return fail(JSLP_ERR_ARG, "pack_upload: null pack");
    for (int32_t i = 0; i < p->n; i++)
        if (!p->is_set[i]) return pack_fail(JSLP_ERR_STATE, "pack_upload", i, "never set (jslpp_pack_set)");
    for (int32_t i = 0; i < p->n; i++)
        if (p->n_opt[i] && !p->opt_set[i])
            return pack_fail(JSLP_ERR_STATE, "pack_upload", i, "optional objectives reserved and never set (jslps_pack_set_optional_objectives)");
    HIPC(hipSetDevice(p->device));
    for (int32_t i = 0; i < p->n; i++) {  // the state an upload leaves (k_upload_finish)
        DevState st;
        memset(&st, 0, sizeof st);
        st.H = p->H[i];
        st.last_element_index = p->W[i] + p->H[i] - 2;  // tableau.ts:312-316
        st.status = ST_DONE;
        st.phase = 1;
        st.feasible = 1;
        st.bounded = 1;
        st.unbounded_var = -1;
        memcpy(p->h_image.p + p->image_off[i], &st, sizeof st);
        p->evaluation[i] = 0;
    }
    if (p->image_bytes) HIPC(hipMemcpyAsync(p->d_image, p->h_image.p, p->image_bytes, hipMemcpyHostToDevice, p->stream));
    HIPC(hipStreamSynchronize(p->stream));
    p->uploaded = 1;
    p->tree_ran = false;
    p->solved = false;
    return JSLP_OK;
}

static int tree_error(const TreeRec& r) {
    switch (r.err) {
        case TREE_OK: return JSLP_OK;
        case TREE_ERR_NODES: return fail(JSLP_ERR_CAPACITY, "branch_and_cut: max_nodes reached before the tree was done");
        case TREE_ERR_HEAP: return fail(JSLP_ERR_CAPACITY, "branch_and_cut: heap_cap reached (the heap is full)");
        case TREE_ERR_CUTS: return fail(JSLP_ERR_CAPACITY, "branch_and_cut: cut_rows reached (a node's cut list is longer)");
        case TREE_ERR_BRANCH: return fail(JSLP_ERR_ARG, "branch_and_cut: a node is not integral and has no fractional variable (negative precision?)");
        case TREE_ERR_MIR_ROWS: return fail(JSLP_ERR_CAPACITY, "branch_and_cut: row_extra reached (the rows of a MIR round or of a cut list do not fit the row capacity)");
        case TREE_ERR_MIR_ROUNDS: return fail(JSLP_ERR_CAPACITY, "branch_and_cut: mir rounds: JSLPR_MAX_ROUNDS rounds of one node without a stop");
        case TREE_ERR_INC_ROWS: return fail(JSLP_ERR_CAPACITY, "branch_and_cut: row_extra reached (the new cut row of a node that starts from a checkpoint does not fit the row capacity)");
    }
    return fail(JSLP_ERR_DEVICE, "unknown tree error code");
}

// One call on every LP of an uploaded pack -- simplex(), or with `tree` the whole branch-and-cut tree (include/jslpt_tree.h): the flags, one
// launch per launch group that has LPs, the ONE D2H copy, then LP after LP what jslp_engine_simplex does after its solve.  An LP that failed
// keeps its entries of out / tree_out and gets its code in `status`; the call's error names the first such LP.
static int pack_run(jslpp_pack* p, bool tree, const int32_t* check_cycles, jslp_simplex_result* out, jslpt_tree_result* tree_out, int32_t* status,
                    double* device_ms) {
    if (device_ms) *device_ms = 0;
    p->launches = 0;
    const int32_t n = p->n;
    if (n == 0) return JSLP_OK;
    HIPC(hipSetDevice(p->device));
    hipStream_t s = p->stream;
    PackLaunch a{};
    a.tree = tree;
    a.lps = p->d_lps;
    a.trees = tree ? p->d_trees : nullptr;
    a.cc = nullptr;
    a.cc_all = check_cycles ? (check_cycles[0] != 0) : 1;
    if (check_cycles) {  // one flag for all is an argument; a mixed list is a small copy of its own
        bool mixed = false;
        for (int32_t i = 1; i < n && !mixed; i++) mixed = (check_cycles[i] != 0) != (a.cc_all != 0);
        if (mixed) {
            int32_t* h = p->h_cc.as<int32_t>();
            for (int32_t i = 0; i < n; i++) h[i] = check_cycles[i] != 0;
            HIPC(hipMemcpyAsync(p->d_cc, h, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
            a.cc = p->d_cc;
        }
    }
    a.states = p->result.d.p;
    a.rhs = reinterpret_cast<double*>(p->result.d.p + p->at.rhs);
    a.rows = reinterpret_cast<int32_t*>(p->result.d.p + p->at.rows);
    a.tree_out = tree ? p->result.d.p + p->at.tree : nullptr;
    const bool dbg = debug_launch_on();
    if (tree) p->tree_ran = true;
    HIPC(hipEventRecord(p->ev_begin, s));
    int32_t first = 0;
    for (int g = 0; g < jslpp_pack::N_GROUPS; g++) {  // one launch per group that has LPs
        int32_t cnt = p->n_group[g];
        size_t lds = p->lds_group[g];
        const int32_t begin = first;
        first += cnt;
        const bool tol = tree && (g & 1);
        if (!tree) {  // (k_simplex_packed knows no tolerance: the two halves of a group are ONE launch, made at the first)
            if (g & 1) continue;
            cnt += p->n_group[g + 1];
            lds = std::max(lds, p->lds_group[g + 1]);
        }
        if (!cnt) continue;
        const PackGroup& grp = PACK_GROUPS[g / 2];
        const bool own = tree || grp.kind == PACK_OPT;  // (k_simplex_packed: MIR, enhanced and incremental LPs in the plain build)
        a.order = p->d_order + begin;
        a.build = own ? grp.kind : PACK_PLAIN;
        a.tol = tol ? 1 : 0;
        const int le = packed_launch(grp.threads, (unsigned)cnt, lds, a, s);
        HIPC(hipGetLastError());
        // (a large build says what forbade its launch -- the LDS attribute refused, static plus dynamic LDS beyond the compute unit's -- and
        // a group no unit holds a build for is an error, never a launch skipped in silence)
        if (grp.big && le != (int)hipSuccess) {
            snprintf(g_err, sizeof g_err, "pack launch %s<%d%s> lds %zu: %s", tree ? "k_tree_packed" : "k_simplex_packed", grp.threads, own ? grp.suffix : "", lds,
                     le == -1 ? "no unit holds this build" : hipGetErrorString((hipError_t)le));
            return JSLP_ERR_DEVICE;
        }
        p->launches += 1;
        if (dbg) fprintf(stderr, "[jslp] launch %s<%d%s%s> n %d lds %zu\n", tree ? "k_tree_packed" : "k_simplex_packed", grp.threads, own ? grp.suffix : "", tol ? ",tol 1" : "", (int)cnt, lds);
    }
    HIPC(hipEventRecord(p->ev_end, s));
    HIPC(hipMemcpyAsync(p->result.h.p, p->result.d.p, p->at.bytes, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    p->solved = true;
    float ms = 0;
    if (device_ms && hipEventElapsedTime(&ms, p->ev_begin, p->ev_end) == hipSuccess) *device_ms = ms;
    if (status) for (int32_t i = 0; i < n; i++) status[i] = JSLP_OK;
    int32_t first_bad = -1; int first_rc = JSLP_OK; char first_msg[sizeof g_err];
    const DevState* sts = p->h_states();
    const TreeRec* recs = p->h_tree();  // (read with `tree` only)
    if (tree) p->tree_status.assign((size_t)n, JSLP_OK);
    for (int32_t i = 0; i < n; i++) {
        const DevState& st = sts[i];
        int rc = state_error(st);
        if (!rc && tree) rc = tree_error(recs[i]);
        if (!rc) {
            if (tree) {
                const double evaluation = recs[i].evaluation;  // folded on the device, node after node (a node without an optimum keeps the one before)
                decode_state(st, p->precision[i], evaluation, &out[i], nullptr);
                out[i].evaluation = evaluation;
                p->evaluation[i] = evaluation;
            } else {
                decode_state(st, p->precision[i], p->evaluation[i], &out[i], &p->evaluation[i]);
            }
            if (st.cycle_phase && st.hist_n > 0) {  // the reference's [start, length] message from the LP's history (rare: one small copy)
                std::vector<int2> h(st.hist_n);
                if (hipMemcpy(h.data(), p->d_hist + (size_t)i * p->hist_cap, sizeof(int2) * st.hist_n, hipMemcpyDeviceToHost) != hipSuccess)
                    rc = fail(JSLP_ERR_DEVICE, "cycle history read-back failed");
                else
                    cycle_message(h, &out[i].cycle_start, &out[i].cycle_length);
            }
            if (!rc && tree && tree_out) {
                const TreeRec& r = recs[i];
                jslpt_tree_result& o = tree_out[i];
                o.iterations = r.iterations; o.is_integral = r.is_integral; o.final_height = r.final_height;
                o.nodes_pushed = r.nodes_pushed; o.heap_high_water = r.heap_high_water; o.cuts_high_water = r.cuts_high_water;
            }
        }
        if (rc) {
            if (tree) p->tree_status[(size_t)i] = rc;
            if (status) status[i] = rc;
            if (first_bad < 0) { first_bad = i; first_rc = rc; snprintf(first_msg, sizeof first_msg, "%s", g_err); }
        }
    }
    if (first_bad >= 0) {
        snprintf(g_err, sizeof g_err, "%s: LP %d: %s", tree ? "pack_branch_and_cut" : "pack_simplex", (int)first_bad, first_msg);
        return first_rc;
    }
    return JSLP_OK;
}

extern "C" int jslpp_pack_simplex(jslpp_pack* p, const int32_t* check_cycles, jslp_simplex_result* out, int32_t* status, double* device_ms) {
    if (!p || (p->n > 0 && !out)) return fail(JSLP_ERR_ARG, "pack_simplex: bad arguments");
    if (!p->uploaded) return fail(JSLP_ERR_STATE, "pack_simplex before upload");
    if (p->tree_ran) return fail(JSLP_ERR_STATE, "pack_simplex: after jslpt_pack_branch_and_cut the arena holds the saved roots; upload first");
    return pack_run(p, false, check_cycles, out, nullptr, status, device_ms);
}

extern "C" int jslpp_pack_read_rhs(jslpp_pack* p, const double** rhs, const int32_t** var_index_by_row, const int64_t** offsets) {
    if (!p) return fail(JSLP_ERR_ARG, "pack_read_rhs: null pack");
    if (!p->uploaded) return fail(JSLP_ERR_STATE, "pack_read_rhs before upload");
    if (rhs) *rhs = p->h_rhs();
    if (var_index_by_row) *var_index_by_row = p->h_rows();
    if (offsets) *offsets = p->offs.data();
    return JSLP_OK;
}

extern "C" int jslpp_pack_download(jslpp_pack* p, int32_t i, double* matrix, int32_t* var_index_by_row, int32_t* var_index_by_col,
                                   int32_t* row_by_var_index, int32_t* col_by_var_index) {
    if (!p) return fail(JSLP_ERR_ARG, "pack_download: null pack");
    if (i < 0 || i >= p->n) return fail(JSLP_ERR_ARG, "pack_download: no such LP");
    if (!p->uploaded) return fail(JSLP_ERR_STATE, "pack_download before upload");
    if (p->tree_ran) return fail(JSLP_ERR_STATE, "pack_download: after jslpt_pack_branch_and_cut the arena holds the saved roots, not the final tableaus");
    HIPC(hipSetDevice(p->device));
    HIPC(hipStreamSynchronize(p->stream));
    const int32_t H = p->H[i], W = p->W[i], RC = p->RC[i], n_idx = pk_n_idx(RC, W);
    std::vector<char> img(pack_image_bytes(RC, W, p->n_opt[i]));
    HIPC(hipMemcpy(img.data(), p->d_image + p->image_off[i], img.size(), hipMemcpyDeviceToHost));
    const PackInts io = pk_ints(RC, W);
    const int32_t* ints = reinterpret_cast<const int32_t*>(img.data() + p->ints_off(i));
    if (matrix) memcpy(matrix, img.data() + sizeof(DevState), sizeof(double) * (size_t)H * W);
    if (var_index_by_row) memcpy(var_index_by_row, ints + io.vibr, sizeof(int32_t) * (size_t)H);
    if (var_index_by_col) memcpy(var_index_by_col, ints + io.vibc, sizeof(int32_t) * (size_t)W);
    if (row_by_var_index) memcpy(row_by_var_index, ints + io.rbv, sizeof(int32_t) * (size_t)n_idx);
    if (col_by_var_index) memcpy(col_by_var_index, ints + io.cbv, sizeof(int32_t) * (size_t)n_idx);
    return JSLP_OK;
}

extern "C" int jslpp_pack_pivot_trace(jslpp_pack* p, int32_t i, int32_t* row_col, int64_t max_pairs, int64_t* n_pivots) {
    if (!p || !n_pivots) return fail(JSLP_ERR_ARG, "pack_pivot_trace: null pointer");
    if (i < 0 || i >= p->n) return fail(JSLP_ERR_ARG, "pack_pivot_trace: no such LP");
    if (!p->uploaded) return fail(JSLP_ERR_STATE, "pack_pivot_trace before upload");
    HIPC(hipSetDevice(p->device));
    HIPC(hipStreamSynchronize(p->stream));
    DevState st;
    HIPC(hipMemcpy(&st, p->d_image + p->image_off[i], sizeof st, hipMemcpyDeviceToHost));
    *n_pivots = st.trace_n;
    if (row_col && max_pairs > 0 && st.trace_n > p->trace_cap)
        return pack_fail(JSLP_ERR_CAPACITY, "pack_pivot_trace", i, "more pivots since upload than the pack's trace_cap: the recorded prefix is not handed out as if it were complete");
    if (row_col && max_pairs > 0) {
        const long long n = std::min<long long>(st.trace_n, max_pairs);
        if (n > 0) HIPC(hipMemcpy(row_col, p->d_trace + (size_t)i * p->trace_cap, sizeof(int2) * n, hipMemcpyDeviceToHost));
    }
    return JSLP_OK;
}

// ---- the trees of a pack, each walked by its LP's workgroup (include/jslpt_tree.h) ---------------------------------------------------
extern "C" int jslpt_pack_branch_and_cut(jslpp_pack* p, const int32_t* check_cycles, jslp_simplex_result* out, jslpt_tree_result* tree_out,
                                         int32_t* status, double* device_ms) {
    if (!p || (p->n > 0 && !out)) return fail(JSLP_ERR_ARG, "pack_branch_and_cut: bad arguments");
    if (!p->tree) return fail(JSLP_ERR_STATE, "pack_branch_and_cut: not a pack made by jslpt_pack_create");
    if (!p->uploaded) return fail(JSLP_ERR_STATE, "pack_branch_and_cut before upload");
    if (p->tree_ran) return fail(JSLP_ERR_STATE, "pack_branch_and_cut: the arena holds the saved roots of an earlier call; upload first");
    return pack_run(p, true, check_cycles, out, tree_out, status, device_ms);
}

extern "C" int jslpt_pack_read_rhs(jslpp_pack* p, const double** rhs, const int32_t** var_index_by_row, const int64_t** offsets) {
    if (!p) return fail(JSLP_ERR_ARG, "pack_read_rhs: null pack");
    if (!p->tree) return fail(JSLP_ERR_STATE, "pack_read_rhs: not a pack made by jslpt_pack_create");
    return jslpp_pack_read_rhs(p, rhs, var_index_by_row, offsets);
}

#if !defined(JSLP_SPLIT_TU)
#include "jslp_mir_kernels.hip.h"  // single-unit build: the MIR kernels behind everything else (the product: jslp_tu_mir.hip)
#define JSLP_PACKED_KERNELS 1
#include "jslp_packed.hip.h"       // ... and the pack's two (the product: jslp_tu_packed.hip)
#include "jslp_tree.hip.h"         // ... with the tree kernels behind them, every build (the product: jslp_tu_tree_mir.hip, _enh, _inc too)
#endif
