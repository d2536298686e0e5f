// jslp_mir.hip.h -- the MIR-cut loop of a branch-and-bound node INSIDE the LDS node kernels (include/jslpr_mir.h).
// Included by jslp_wglds.hip.h in front of node_lds_run (needs WgLds / SmemL / simplex_wg_lds, Slots / Ctx / DevState, js_max0 / js_min0).
//
// Between two simplex_wg_lds runs the workgroup, alone on its slot, does what the host loop does with three engine calls per round
// (branch-and-cut.ts:38-52): computeFractionalVolume(true) from the LDS copies of column 0 and the row map, applyMIRCuts (up to ten
// lower-bound MIR rows appended to the slot, as k_mir_cuts builds them), and simplex() again.  No workgroup talks to another.
// Only device functions live here: the kernels built on them are instantiated in a translation unit of their own
// (jslp_mir_kernels.hip.h / jslp_tu_mir.hip), so no kernel of the other units changes.
#pragma once

#define JSLPR_MAX_ROUNDS_DEV 64  // JSLPR_MAX_ROUNDS of include/jslpr_mir.h (static_assert in jslp_hip.hip)
#define MIR_MAX_CUTS 10         // applyMIRCuts' default maxCuts (cutting-strategies.ts:199)

// what a node's loop did: jslpr_mir_outcome field for field, then what the host needs to fold the evaluation and the work counters
// over ALL the node's simplexes (the node's DevState record describes the last one only)
struct MirRec {
    int32_t rounds, rows_added, optimal_count, pivots;
    double volume_before, volume_after;
    int32_t fold_kind, pad;  // 0: no simplex set the evaluation; 1: the last one that did was optimal, with fold_obj in A[0,0]; 2: ... unbounded
    double fold_obj;
    long long height_sum;    // heights of all the simplexes (jslp_work_counters::height_sum)
};
struct MirJob {
    const uint8_t* is_int;  // variable.isInteger per variable index
    MirRec* out;            // one record per node, at the index of the node's outcome
    int32_t max_rounds;     // < 0: until the volume rule stops the loop (JSLPR_MAX_ROUNDS rounds without a stop are an error)
    int32_t need_feasible;  // the loop only starts on a feasible tableau (the incremental service)
};
struct MirSm {
    unsigned long long masks[16];  // one ballot per wave of an ordered compaction
    int32_t sel[MIR_MAX_CUTS];     // source rows of this round's cuts
    double volume;
    MirRec rec;                    // the node's record while its loop runs (thread 0's)
};

// one step of an ordered compaction over the workgroup: how many threads before mine hold `ok`, and how many in all (uniform)
__device__ __forceinline__ int mir_rank(bool ok, MirSm& ms, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long m = __ballot(ok);
    if (lane == 0) ms.masks[wave] = m;
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1)), all = 0;
    for (int k = 0; k < nw; k++) {
        const int n = __popcll(ms.masks[k]);
        if (k < wave) before += n;
        all += n;
    }
    __syncthreads();  // (the masks are free for the next step)
    *total = all;
    return before;
}

// computeFractionalVolume(ignoreIntegerValues = true) (mip-utils.ts:67-92) of rows [1, H): the ORDERED product of |value| over the
// basic integer variables that are not at an integer value.  The contributing rows are compacted in row order into `scratch`
// (>= H doubles of LDS) and ONE lane multiplies them in that order: a tree reduction would round differently.  JavaScript's NaN
// rules: Math.min(NaN, x) is NaN and NaN < precision is false, so a NaN (or infinite) row multiplies in.
__device__ __forceinline__ double mir_volume_wg(const double* rhs, const int32_t* vibr, int H, const uint8_t* is_int, double precision, double* scratch, MirSm& ms) {
    int base = 0;
    for (int r0 = 1; r0 < H; r0 += blockDim.x) {
        const int r = r0 + (int)threadIdx.x;
        bool ok = false;
        double distance = 0.0;
        if (r < H) {
            const int v = vibr[r];
            if (v >= 0 && is_int[v]) {
                distance = fabs(rhs[r]);
                const double a = distance - floor(distance), b = floor(distance + 1);
                const bool nan = a != a || b != b;
                ok = nan || !((a < b ? a : b) < precision);
            }
        }
        int total;
        const int before = mir_rank(ok, ms, &total);
        if (ok) scratch[base + before] = distance;
        base += total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double volume = -1.0;
        for (int i = 0; i < base; i++) volume = volume == -1.0 ? scratch[i] : volume * scratch[i];
        ms.volume = volume == -1.0 ? 0.0 : volume;
    }
    __syncthreads();
    return ms.volume;
}

// applyMIRCuts (cutting-strategies.ts:199-212) on the tableau of context c, whose rows are all current in c.A (an eager slot): the
// arithmetic of k_mir_cuts, with the scan reading the LDS copies of column 0 and the maps.  Rows H .. H+n-1 of the slot are written
// with their RHS mirror, row map, index maps and dirty flags, and the state's height; the next simplex_wg_lds reloads its LDS
// copies from there.  Returns n (uniform), or -1 with st->err = ERR_CAPACITY when the rows or the slack indexes do not fit.
__device__ __forceinline__ int mir_append_wg(const Ctx& c, const WgLds& L, int H, int lei, int idx_cap, const uint8_t* is_int, int cap_rows, MirSm& ms) {
    const double precision = c.precision;
    const int W = c.W, ld = c.ld;
    int base = 0;
    for (int r0 = 1; r0 < H && base < MIR_MAX_CUTS; r0 += blockDim.x) {
        const int r = r0 + (int)threadIdx.x;
        bool ok = false;
        if (r < H) {
            const int v = L.vibr[r];
            if (v >= 0 && is_int[v]) {  // :82-85
                const double rhs = L.rhs[r];
                const double f = rhs - floor(rhs);
                ok = !(f < precision || f > 1 - precision);  // :88-90
            }
        }
        int total;
        const int before = mir_rank(ok, ms, &total);
        if (ok && base + before < MIR_MAX_CUTS) ms.sel[base + before] = r;
        base += total;
    }
    __syncthreads();
    const int n = base < MIR_MAX_CUTS ? base : MIR_MAX_CUTS;
    if (H + n > cap_rows || lei + n > idx_cap) {
        if (threadIdx.x == 0) { c.st->err = ERR_CAPACITY; c.st->mir_added = 0; }
        __syncthreads();
        return -1;
    }
    for (int k = 0; k < n; k++) {
        const double* src = c.A + (long long)ms.sel[k] * ld;
        double* dst = c.A + (long long)(H + k) * ld;
        const double rhs = src[0];
        const double f = rhs - floor(rhs);
        for (int col = threadIdx.x; col < ld; col += blockDim.x) {
            double out = 0.0;
            if (col == 0) {
                out = floor(rhs) - rhs;  // :112 then :128-130
            } else if (col < W) {
                const double a = src[col];
                const int v = L.vibc[col];
                double cut;
                if (v >= 0 && is_int[v]) {  // :117-123
                    const double fl = floor(a);
                    cut = fl + js_max0(a - fl - f) / (1 - f);
                } else {
                    cut = js_min0(a / (1 - f));  // :124-125
                }
                out = cut - a;  // :128-130
            }
            dst[col] = out;
            if (col == 0 && c.rhs) c.rhs[H + k] = out;
        }
    }
    if (threadIdx.x == 0) {
        for (int k = 0; k < n; k++) {  // :104-109
            const int slack = lei + k;
            c.vibr[H + k] = slack;
            c.rbv[slack] = H + k;
            c.cbv[slack] = -1;
            c.dirty[H + k] = 1;
        }
        c.st->last_element_index = lei + n;
        c.st->H = H + n;
        c.st->mir_added = n;
    }
    __syncthreads();
    return n;
}

// The loop itself, entered behind the node's first simplex_wg_lds (whose final barrier made the state visible to the workgroup).
// Every value the loop branches on is read from the slot's state or from LDS behind a barrier: uniform.  The record is thread 0's,
// kept in LDS (as registers of every thread it would be live across the simplexes, which the 512-thread builds have no room for).
template <int UN, bool PF>
__device__ __forceinline__ void mir_node_loop(const Ctx& c, int idx_cap, SmemL& sm, const WgLds& L, const MirJob& mj, int o, int iters_cap, int cap_rows) {
    __shared__ MirSm ms;
    DevState* st = c.st;
    const bool t0 = threadIdx.x == 0;
    auto absorb = [&]() {  // thread 0: one finished simplex()
        MirRec& rec = ms.rec;
        if (st->optimal) { rec.fold_kind = 1; rec.fold_obj = st->obj_cell; rec.optimal_count += 1; }
        else if (!st->bounded) rec.fold_kind = 2;
        rec.pivots += st->it1 + st->it2;
        rec.height_sum += st->H;
    };
    if (t0) {
        MirRec& rec = ms.rec;
        rec.rounds = 0; rec.rows_added = 0; rec.optimal_count = 0; rec.pivots = 0; rec.volume_before = 0.0; rec.volume_after = 0.0;
        rec.fold_kind = 0; rec.pad = 0; rec.fold_obj = 0.0; rec.height_sum = 0;
        absorb();
    }
    int err = st->err, rounds = 0;
    const bool run = err == ERR_NONE && !(mj.need_feasible && !st->feasible);
    const int limit = mj.max_rounds < 0 ? JSLPR_MAX_ROUNDS_DEV : (mj.max_rounds < JSLPR_MAX_ROUNDS_DEV ? mj.max_rounds : JSLPR_MAX_ROUNDS_DEV);
    bool stopped = !run || limit == 0;
    double before = 0.0;
    if (!stopped) before = mir_volume_wg(L.rhs, L.vibr, st->H, mj.is_int, c.precision, L.pcol, ms);
    while (!stopped && rounds < limit) {
        const int n = mir_append_wg(c, L, st->H, st->last_element_index, idx_cap, mj.is_int, cap_rows, ms);
        if (n < 0) { err = ERR_CAPACITY; break; }
        err = simplex_wg_lds<UN, false, PF>(c, sm, L, iters_cap);  // (not preloaded: column 0, the cost row and the maps come back from the slot)
        rounds += 1;
        if (t0) { absorb(); ms.rec.rounds = rounds; ms.rec.rows_added += n; }
        if (err == ERR_NONE) err = st->err;
        if (err != ERR_NONE) break;
        const double after = mir_volume_wg(L.rhs, L.vibr, st->H, mj.is_int, c.precision, L.pcol, ms);
        if (t0) { ms.rec.volume_before = before; ms.rec.volume_after = after; }
        if (after >= 0.9 * before) stopped = true;  // (false for NaN: the loop goes on, as the reference's does)
        before = after;
    }
    if (!stopped && err == ERR_NONE && mj.max_rounds < 0) {  // the unbounded loop must end whatever the data: a loud failure
        if (t0) st->err = ERR_MIR_ROUNDS;  // (a code of its own: the host names the round limit, as the sequenced form does, not a row capacity)
    }
    if (t0) mj.out[o] = ms.rec;
    __syncthreads();
}

// everything a MIR launch takes, as plain bytes between the units (the same struct in each: same headers, same flags)
struct MirLaunch {
    Slots s; Snapshot sn; Cuts cu; MirJob mj;
    int check_cycles, iters_cap, cap_rows;
    double* rhs; int32_t* rows; DevState* states; int out_stride;
    int first;                                                              // k_node_lds_mir: first node of the launch = index of its outcome
    unsigned* done_flag; unsigned done_seq; int* done_count;
    int n_nodes; const int32_t* order; int* queue;                          // k_node_queue_mir
    double* volume_out;                                                     // k_fractional_volume
};
enum { MIR_K_NODE_LDS_1024 = 0, MIR_K_NODE_LDS_512 = 1, MIR_K_NODE_QUEUE_512 = 2, MIR_K_VOLUME = 3 };
