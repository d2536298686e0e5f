// jslp_packed.hip.h -- the pack of small LPs (include/jslpp_packed.h): one workgroup per LP, the WHOLE tableau and its index maps in LDS.
//
// Two parts, each included once per unit (no #pragma once on purpose):
//   * the layout (always): where the pieces of one LP lie in the arena image and in LDS, the per-LP descriptor and the launch arguments --
//     host and device read the same functions, jslpp_lds_bytes is pk_lds_bytes;
//   * the kernels and their launch function (-DJSLP_PACKED_KERNELS; needs jslp_kernels.hip.h in front: Cand / the orders / wave_reduce /
//     block_reduce / eliminate / nonzero16 / suffix_is_square / begin_simplex / many_global).  The product compiles them in a unit of
//     their own (jslp_tu_packed.hip); a single-unit build includes them at the end of jslp_hip.hip.
//
// Why a kernel of its own: k_simplex_lds_many keeps the selection state in LDS and the tableau in global memory, so every pivot of a
// 3 x 3 LP pays a strided column gather, a row read and the gated rows' round trips through L2.  A tableau of a few thousand cells fits
// in LDS whole: here a pivot touches global memory twice, with stores nobody waits for (the history pair and the trace pair).
#ifndef JSLP_PACKED_LAYOUT
#define JSLP_PACKED_LAYOUT

// ---- layout ---------------------------------------------------------------------------------------------------------------------------
// Arena image of one LP (what the ONE H2D copy brings, 16-byte aligned, a multiple of 16 bytes):
//   [DevState | matrix H x W doubles, reference layout (stride W), padded to an even count | integer block]
// Integer block, the same in the image and in LDS, every piece padded to 16 bytes so that the block moves as a run of 16-byte words:
//   [varIndexByRow H | varIndexByCol W | rowByVarIndex n_idx | colByVarIndex n_idx | unrestricted flags, n_idx bytes]
// with n_idx = W + 2 H + 2, as jslp_engine_create(height, width, row_capacity = height) sizes the maps.  In a pack with cut rows
// (include/jslpt_tree.h) every H of this layout is the LP's row capacity RC, of which the first `height` rows hold the tableau.
// LDS image: [tableau H x S doubles | pivot column H doubles | (pad to 16 bytes) | integer block], S = the row stride padded to an ODD
// number of doubles: the pivot-column gather has lane r reading A[r][c], and with an odd stride 32 consecutive rows fall into 32
// distinct pairs of the 64 four-byte banks -- conflict-free for ds_read_b64 (an even stride of 2^k doubles would be 2^k-way).
struct PackInts { int32_t vibr, vibc, rbv, cbv, unr, total; };  // offsets / size in 4-byte words
__host__ __device__ __forceinline__ int32_t pk_pad4(int32_t n) { return (n + 3) & ~3; }
__host__ __device__ __forceinline__ int32_t pk_n_idx(int32_t H, int32_t W) { return W + 2 * H + 2; }
__host__ __device__ __forceinline__ int32_t pk_stride(int32_t W) { return W | 1; }
__host__ __device__ __forceinline__ PackInts pk_ints(int32_t H, int32_t W) {
    const int32_t n = pk_n_idx(H, W);
    PackInts o;
    o.vibr = 0;
    o.vibc = pk_pad4(H);
    o.rbv = o.vibc + pk_pad4(W);
    o.cbv = o.rbv + pk_pad4(n);
    o.unr = o.cbv + pk_pad4(n);
    o.total = o.unr + pk_pad4((n + 3) / 4);
    return o;
}
// An LP with n_opt >= 1 optional objectives (include/jslps_soft.h) carries their rows in both places: in the image n_opt x W doubles
// (stride W) directly behind the matrix, at pk_opt_image_off; in LDS n_opt x S doubles directly behind the pivot column, with the same odd
// stride S.  With n_opt == 0 every offset and byte count below is what it was before there were such rows.
__host__ __device__ __forceinline__ long long pk_opt_image_off(int32_t H, int32_t W) { return ((long long)H * W + 1) & ~1LL; }  // in doubles, behind the matrix
__host__ __device__ __forceinline__ long long pk_image_doubles(int32_t H, int32_t W, int32_t n_opt = 0) {  // the matrix (and the optional rows) in the image
    return (pk_opt_image_off(H, W) + (long long)n_opt * W + 1) & ~1LL;
}
__host__ __device__ __forceinline__ long long pk_lds_doubles(int32_t H, int32_t W, int32_t n_opt = 0) {
    return ((long long)H * pk_stride(W) + H + (long long)n_opt * pk_stride(W) + 1) & ~1LL;
}
__host__ __device__ __forceinline__ long long pk_lds_bytes(int32_t H, int32_t W, int32_t n_opt = 0) {
    return 8 * pk_lds_doubles(H, W, n_opt) + 4LL * pk_ints(H, W).total;
}

// One LP of a pack: built on the host ONCE, at create; one entry per workgroup.
struct PackLp {
    char* image;        // this LP's arena image (see above)
    int2* hist;         // cycle-check history of the current phase, hist_cap pairs
    int2* trace;        // pivot trace since the upload, trace_cap pairs
    double precision;
    long long out_off;  // first entry of this LP's RHS column / row map in the result block
    int32_t H, W;
    int32_t hist_cap, trace_cap;
    int32_t iters_cap;
    int32_t batch, use_partial;  // partial-pricing parameters (simplex.ts:118-127)
    int32_t RC;         // rows the image and the LDS layout are sized for: H, or H + cut rows in a pack made by jslpt_pack_create
    int32_t n_opt;      // optional objectives (0: the LP runs in an OPT = false build)
    double* opt_out;    // this LP's n_opt x W optional rows in the result block
};
// The kind of an LP of a pack, which is also the build of the kernel its tree runs in: the default service (PACK_PLAIN), the same with
// optional objectives (PACK_OPT, include/jslps_soft.h), a MIR LP (include/jslpc_tree_mir.h), an enhanced LP (include/jslpe_tree_enhanced.h),
// an incremental LP (include/jslpi_tree_incremental.h).  k_simplex_packed has the first two builds only.
enum PackKind : int32_t { PACK_PLAIN = 0, PACK_OPT = 1, PACK_MIR = 2, PACK_ENH = 3, PACK_INC = 4 };
// arguments of one launch, travelling as bytes between the units (the same struct in every unit)
struct PackLaunch {
    const PackLp* lps;
    const int32_t* order;  // blockIdx.x -> LP index (the LPs of this build)
    const int32_t* cc;     // per-LP checkForCycles, or nullptr: cc_all for every LP
    int32_t cc_all, tree;  // tree 0: k_simplex_packed, 1: k_tree_packed (jslp_tree.hip.h)
    int32_t tol;           // k_tree_packed: 1: the TOL build of that kind (include/jslpg_tree_tolerance.h; every LP of `order` has a tolerance), 0: the other
    int32_t build;         // the PackKind whose build of that kernel runs: every LP of `order` is of this kind (k_simplex_packed: PACK_OPT, or
                           // PACK_PLAIN for every other kind)
    void* states;          // result block: DevState per LP (LP order) ...
    double* rhs;           // ... the RHS columns one after the other ...
    int32_t* rows;         // ... and the row maps
    const void* trees;     // tree 1: the TreeLp table ...
    void* tree_out;        // ... and the TreeRec per LP
};
// The large class (include/jslpb_big_lds.h): an LP whose LDS image exceeds PACK_SMALL_LDS runs in the large build of its kind, a workgroup of
// PACK_BIG_THREADS threads with a compute unit to itself (jslp_tu_packed_big.hip).  ONE thread count ships (profiles/packed_big_times.md has
// the candidates' table); -DJSLP_PACK_BIG_THREADS on every unit builds a development library at another.
#ifndef JSLP_PACK_BIG_THREADS
#define JSLP_PACK_BIG_THREADS 1024
#endif
static_assert(JSLP_PACK_BIG_THREADS == 256 || JSLP_PACK_BIG_THREADS == 512 || JSLP_PACK_BIG_THREADS == 1024, "the large builds' thread count");
#define PACK_SMALL_LDS 65536       // JSLPP_LDS_LIMIT: the dynamic LDS of the 64- and 256-thread builds at most
#define PACK_BIG_LDS (156 * 1024)  // JSLPB_LDS_LIMIT: of the large builds
#define PACK_CU_LDS (160 * 1024)   // static plus dynamic LDS of one workgroup at most
#endif  // JSLP_PACKED_LAYOUT

#if defined(JSLP_PACKED_KERNELS) && !defined(JSLP_PACKED_KERNELS_DONE)
#define JSLP_PACKED_KERNELS_DONE

#define PK_HIST 128  // first pairs of the cycle-check history kept in LDS: while the history fits, the suffix test runs on them
struct PackSmem {
    Smem g;              // cross-wave stage of block_reduce
    int2 hist[PK_HIST];
};

// the winner of a selection in every thread: one wave reduces with shuffles alone, four waves meet in LDS (block_reduce)
template <int THREADS, class Better>
__device__ __forceinline__ Cand pk_reduce(Cand x, Better better, Smem& sm) {
    if constexpr (THREADS == 64) {
        x = wave_reduce(x, better);
        Cand r;
        r.v = __shfl(x.v, 0, 64);
        r.i = __shfl(x.i, 0, 64);
        r.b = __shfl(x.b, 0, 64);
        return r;
    } else {
        return block_reduce(x, better, sm);
    }
}

// what one simplex() leaves in registers.  outcome: 0 running, 1 optimal, 2 unbounded, 3 cycle, 4 infeasible, 5 iteration cap, 6 history full
struct PkRun { int phase, it1, it2, hist_n, entered2, outcome, unbounded_col; };

// simplex() of the H x W tableau that LDS holds (row stride S, its maps and flags next to it), for k_tree_packed (jslp_tree.hip.h), which
// runs it once per node: phase 1 / phase 2 / pivot / checkForCycles.  The loop restates select_step / prepare_pivot / update_rows_wg
// (jslp_core.inc.h) over LDS with its scalars in registers, as simplex_wg_lds does over global memory; arithmetic, orders and tie-breaks
// are the core's own functions.  Bounded by iters_left.  The caller puts a barrier in front (LDS complete) and one behind.
// A SECOND COPY of k_simplex_packed's loop below, line for line, on purpose: with the kernel calling this function its 256-thread build
// took 59 VGPRs instead of 57 (profiles/packed_tree_kernel_resources.md), so the kernel keeps its own text.  Change both together:
// tests/test_pack_edges_gpu.py holds each copy to the oracle at the edges of these loops (the kernel's through the LP packs, this one as tree roots).
// OPT: the LP has n_opt >= 1 optional objectives, their rows at oo (stride S); every line of theirs sits under `if constexpr (OPT)`.
template <int THREADS, bool OPT>
__device__ __forceinline__ PkRun pk_simplex(double* A, double* pcol, const int H, const int W, const int S, int32_t* vibr, int32_t* vibc, int32_t* rbv,
                                            int32_t* cbv, const uint8_t* unr, const double precision, const int check_cycles, const PackLp& m, int2* ghist,
                                            int2* gtrace, PackSmem& sm, int& iters_left, long long& trace_n, double* oo, const int n_opt) {
    const int tid = threadIdx.x;
    // the row update's thread grid: CW columns (a power of two covering the width, at most the workgroup) x RP rows at a time
    int cshift = 0;
    while ((1 << cshift) < W && (1 << cshift) < THREADS) cshift++;
    const int CW = 1 << cshift, RP = THREADS >> cshift, col0 = tid & (CW - 1), rsub = tid >> cshift;

    int phase = 1, it1 = 0, it2 = 0, hist_n = 0, entered2 = 0;
    int outcome = 0, unbounded_col = 0;
    while (outcome == 0) {
        if (iters_left <= 0) { outcome = 5; break; }
        int pr = 0, pc = 0;
        if (phase == 1) {
            // leaving row: most negative RHS below -precision, first index on ties (simplex.ts:39-49)
            Cand best; best.v = -precision; best.i = 0; best.b = 0;
            for (int r = 1 + tid; r < H; r += THREADS) {
                const double v = A[r * S];
                if (v < best.v) { best.v = v; best.i = r; }
            }
            best = pk_reduce<THREADS>(best, MinFirst(), sm.g);
            if (best.i == 0) {  // :51-54 feasible: phase 2 starts in this same iteration with a fresh history (:102)
                phase = 2; entered2 = 1; hist_n = 0;
            } else {
                pr = best.i;
                // entering column: max -cost/coef over unrestricted or coef < -precision (simplex.ts:56-71)
                const double* row = A + pr * S;
                Cand q; q.v = -INFINITY; q.i = 0; q.b = 0;
                for (int col = 1 + tid; col < W; col += THREADS) {
                    const double coef = row[col];
                    const bool un = unr[vibc[col]] != 0;
                    if (un || coef < -precision) {
                        const double quo = -A[col] / coef;
                        if (q.v < quo) { q.v = quo; q.i = col; }
                    }
                }
                q = pk_reduce<THREADS>(q, MaxFirst(), sm.g);
                if (q.i == 0) { outcome = 4; break; }  // :73-76 infeasible
                pc = q.i;
            }
        }
        if (phase == 2) {
            // Dantzig pricing with the reference's batch rule (simplex.ts:118-219): the first batch holding a candidate
            // wins; inside it the largest value, first index on ties
            Cand e; e.v = precision; e.i = 0; e.b = 0;
            for (int col = 1 + tid; col < W; col += THREADS) {
                const double rc = A[col];
                const bool un = unr[vibc[col]] != 0;
                const int b = m.use_partial ? (col - 1) / m.batch : 0;
                const double val = (un && rc < 0) ? -rc : rc;
                if (val > precision) {
                    Cand cand; cand.v = val; cand.i = col; cand.b = b;
                    const bool take = PriceFirst()(cand, e);
                    e.v = take ? cand.v : e.v;
                    e.i = take ? cand.i : e.i;
                    e.b = take ? cand.b : e.b;
                }
            }
            e = pk_reduce<THREADS>(e, PriceFirst(), sm.g);
            int opt_row = -1;  // which optional objective named the entering column (-1: the cost row)
            if constexpr (OPT) {
                // simplex.ts:221-263 as select_step restates it: no column prices out on the cost row -> objective by objective in priority
                // order, among the columns within +-precision on the cost row and on every earlier objective (every batch was scanned
                // without a winner, so the deferred set spans all of them): the largest value above precision, first index on ties
                for (int o = 0; e.i == 0 && o < n_opt; o++) {
                    Cand x; x.v = precision; x.i = 0; x.b = 0;
                    for (int col = 1 + tid; col < W; col += THREADS) {
                        const double rc0 = A[col];
                        bool deferred = -precision < rc0 && rc0 < precision;
                        for (int q = 0; deferred && q < o; q++) {
                            const double rq = oo[q * S + col];
                            deferred = -precision < rq && rq < precision;
                        }
                        if (!deferred) continue;
                        const double rc = oo[o * S + col];
                        if (-precision < rc && rc < precision) continue;
                        const bool un = unr[vibc[col]] != 0;
                        const double val = (un && rc < 0) ? -rc : rc;
                        const bool take = val > x.v;  // strict: the first index wins ties inside a thread (my columns ascend)
                        x.v = take ? val : x.v;
                        x.i = take ? col : x.i;
                    }
                    e = pk_reduce<THREADS>(x, PriceFirst(), sm.g);
                    if (e.i != 0) opt_row = o;
                }
            }
            if (e.i == 0) { outcome = 1; break; }  // optimal (simplex.ts:265-269)
            pc = e.i;
            int neg_flag;
            {   // isReducedCostNegative of the winner, from the row that named it
                double rc = A[pc];
                if constexpr (OPT) { if (opt_row >= 0) rc = oo[opt_row * S + pc]; }
                neg_flag = (unr[vibc[pc]] != 0 && rc < 0) ? 1 : 0;
            }
            // ratio test (simplex.ts:271-296) in its order-free form: the first row passing the degenerate test wins
            // outright, otherwise the first-index argmin of the accepted quotients.  One reduction: an accepted quotient is above
            // precision > 0, so a degenerate row enters as -Infinity and MinFirst breaks the ties among them by the first index.
            Cand mq; mq.v = INFINITY; mq.i = 0; mq.b = 0;
            int rdeg = 0;
            for (int r = 1 + tid; r < H; r += THREADS) {
                const double colv = A[r * S + pc];
                const double rhs = A[r * S];
                if (-precision < colv && colv < precision) continue;
                if (colv > 0 && precision > rhs && rhs > -precision) {
                    if (rdeg == 0) rdeg = r;  // (my rows ascend)
                    continue;
                }
                const double quo = neg_flag ? -rhs / colv : rhs / colv;
                if (quo > precision && mq.v > quo) { mq.v = quo; mq.i = r; }
            }
            if (rdeg != 0) { mq.v = -INFINITY; mq.i = rdeg; }
            mq = pk_reduce<THREADS>(mq, MinFirst(), sm.g);
            if (mq.i == 0) { outcome = 2; unbounded_col = pc; break; }  // unbounded (simplex.ts:298-303)
            pr = mq.i;
        }
        const int leaving = vibr[pr], entering = vibc[pc];
        // cycle check (simplex.ts:78-93 / 305-320): append first, test, stop WITHOUT pivoting on a hit.  The host rebuilds the
        // reference's [start, length] message from the global copy.
        if (check_cycles) {
            if (hist_n >= m.hist_cap) { outcome = 6; break; }
            if (tid == 0) {
                const int2 pair = make_int2(leaving, entering);
                ghist[hist_n] = pair;
                if (hist_n < PK_HIST) sm.hist[hist_n] = pair;
            }
            __syncthreads();
            hist_n += 1;
            const bool cycle = hist_n <= PK_HIST ? suffix_is_square(sm.hist, hist_n, sm.g) : suffix_is_square(ghist, hist_n, sm.g);
            if (cycle) { outcome = 3; break; }
        }
        // ---- pivot(pr, pc) (simplex.ts:330-391) ------------------------------------------------------------------------------------
        const double quot = A[pr * S + pc];  // :335
        int any = 0;
        for (int r = tid; r < H; r += THREADS) {  // the pivot column: lane r reads A[r][pc], conflict-free with the odd stride
            const double k = A[r * S + pc];
            pcol[r] = k;
            any |= (r != pr && nonzero16(k)) ? 1 : 0;
        }
        // any row that will execute the inner loop of :367-391 lazily zeroes the tiny pivot-row entries
        const int anyrow = __syncthreads_or(any);  // (also orders the quot read above against the row write below)
        double* prow = A + pr * S;
        for (int col = tid; col < W; col += THREADS) {
            const double val = prow[col];
            const bool innz = nonzero16(val);                          // :356
            double v = innz ? val / quot : 0.0;                        // :357 / :361  (IEEE division)
            if (col == pc) v = 1.0 / quot;                             // :364
            if (innz && anyrow && !nonzero16(v) && v != 0.0) v = 0.0;  // :381-383
            prow[col] = v;
        }
        if (tid == 0) {  // :339-349
            vibr[pr] = entering;
            vibc[pc] = leaving;
            rbv[entering] = pr;
            rbv[leaving] = -1;
            cbv[entering] = -1;
            cbv[leaving] = pc;
            if (trace_n < m.trace_cap) gtrace[trace_n] = make_int2(pr, pc);
        }
        trace_n += 1;
        if (phase == 1) it1 += 1; else it2 += 1;
        iters_left -= 1;
        __syncthreads();  // the normalised pivot row and the pivot column are complete
        for (int r = rsub; r < H; r += RP) {
            const double k = pcol[r];
            if (r == pr || !nonzero16(k)) continue;  // the row gate, :370-375
            double* row = A + r * S;
            for (int col = col0; col < W; col += CW) {
                if (col == pc) { row[col] = -k / quot; continue; }  // :387 overwrites whatever the loop did to column pc
                const double p = prow[col];
                if (nonzero16(p)) row[col] = eliminate(row[col], k, p);  // :376-386, both roundings
            }
        }
        if constexpr (OPT) {
            // the optional objectives (simplex.ts:394-412) as prepare_pivot restates them: the same elimination with EXACT `!= 0` tests, on the
            // final pivot row (lazy zeroing included), one (objective, column) cell per thread and step.  Column pc waits for the barrier:
            // every thread has read an objective's coefficient before its owner overwrites it
            for (int q = tid; q < n_opt * W; q += THREADS) {
                const int o = q / W, col = q - o * W;
                if (col == pc) continue;
                double* rc = oo + o * S;
                const double coefficient = rc[pc];
                if (coefficient != 0.0) {
                    const double v0 = prow[col];
                    if (v0 != 0.0) rc[col] = eliminate(rc[col], coefficient, v0);
                }
            }
            __syncthreads();
            for (int o = tid; o < n_opt; o += THREADS) {
                const double coefficient = oo[o * S + pc];
                if (coefficient != 0.0) oo[o * S + pc] = -coefficient / quot;  // :410
            }
        }
        __syncthreads();
    }
    PkRun o;
    o.phase = phase; o.it1 = it1; o.it2 = it2; o.hist_n = hist_n; o.entered2 = entered2; o.outcome = outcome; o.unbounded_col = unbounded_col;
    return o;
}

// simplex() of LP order[blockIdx.x] of a pack: load the LP into LDS, run phase 1 / phase 2 / pivot / checkForCycles there (the loop of
// pk_simplex above, in a copy of the kernel's own), write the tableau, the maps, the state, the RHS column and the row map back once.  THREADS = 64: one wave -- the block barriers degenerate (the compiler drops s_barrier for a
// one-wave workgroup) and every reduction is wave_reduce alone; THREADS = 256: four waves.  Every loop is bounded by the pivot cap; the
// kernel waits on nothing outside its workgroup.  The image and the LDS layout are those of RC rows (RC = H but in a pack with cut rows,
// include/jslpt_tree.h), of which H hold the tableau.
// OPT = true: the LPs with optional objectives (include/jslps_soft.h): their rows come with the image, live in LDS behind the pivot column,
// and go back into the image and into the result block with everything else.
template <int THREADS, bool OPT>
__global__ void __launch_bounds__(THREADS) k_simplex_packed(const PackLp* __restrict__ lps, const int32_t* __restrict__ order, const int32_t* __restrict__ cc,
                                                            int cc_all, DevState* __restrict__ out_states, double* __restrict__ out_rhs,
                                                            int32_t* __restrict__ out_rows) {
    extern __shared__ __attribute__((aligned(16))) double pk_lds[];
    __shared__ PackSmem sm;
    const int idx = order[blockIdx.x];
    const PackLp m = lps[idx];  // one uniform copy at entry
    const int tid = threadIdx.x;
    const int H = m.H, W = m.W, RC = m.RC, S = pk_stride(W);
    const PackInts io = pk_ints(RC, W);
    const double precision = m.precision;
    const int check_cycles = cc ? cc[idx] : cc_all;
    int n_opt = 0;
    if constexpr (OPT) n_opt = m.n_opt;
    // LDS, indexed from the extern base: ds_read / ds_write, never flat
    double* A = pk_lds;
    double* pcol = pk_lds + RC * S;
    double* oo = pcol + RC;  // (OPT) the optional rows, stride S
    int32_t* ints = reinterpret_cast<int32_t*>(pk_lds + pk_lds_doubles(RC, W, n_opt));
    int32_t* vibr = ints + io.vibr;
    int32_t* vibc = ints + io.vibc;
    int32_t* rbv = ints + io.rbv;
    int32_t* cbv = ints + io.cbv;
    const uint8_t* unr = reinterpret_cast<const uint8_t*>(ints + io.unr);
    // global memory (the descriptor's pointers were loaded from memory: say where they point, see many_global)
    char* image = many_global(m.image);
    DevState* st = reinterpret_cast<DevState*>(image);
    double2* gA = reinterpret_cast<double2*>(image + sizeof(DevState));
    int4* gI = reinterpret_cast<int4*>(image + sizeof(DevState) + 8 * pk_image_doubles(RC, W, n_opt));
    double* gO = reinterpret_cast<double*>(image + sizeof(DevState)) + pk_opt_image_off(RC, W);  // (OPT) the optional rows, stride W
    int2* ghist = many_global(m.hist);
    int2* gtrace = many_global(m.trace);

    // ---- load: the matrix as 16-byte words (stride W -> stride S), the integer block verbatim --------------------------------------
    const int cells = H * W, pairs = (cells + 1) >> 1, words = io.total >> 2;
    for (int q = tid; q < pairs; q += THREADS) {
        const double2 v = gA[q];
        const int e = 2 * q, r = e / W, c = e - r * W;
        A[r * S + c] = v.x;
        if (e + 1 < cells) {
            const bool wrap = c + 1 == W;
            A[(wrap ? r + 1 : r) * S + (wrap ? 0 : c + 1)] = v.y;
        }
    }
    for (int q = tid; q < words; q += THREADS) reinterpret_cast<int4*>(ints)[q] = gI[q];
    if constexpr (OPT)
        for (int q = tid; q < n_opt * W; q += THREADS) {
            const int o = q / W;
            oo[o * S + (q - o * W)] = gO[q];
        }
    if (tid == 0) begin_simplex(st, m.iters_cap);  // simplex.ts:14-23
    long long trace_n = st->trace_n;
    __syncthreads();

    // the row update's thread grid: CW columns (a power of two covering the width, at most the workgroup) x RP rows at a time
    int cshift = 0;
    while ((1 << cshift) < W && (1 << cshift) < THREADS) cshift++;
    const int CW = 1 << cshift, RP = THREADS >> cshift, col0 = tid & (CW - 1), rsub = tid >> cshift;

    int phase = 1, it1 = 0, it2 = 0, hist_n = 0, iters_left = m.iters_cap, entered2 = 0;
    // outcome: 0 running, 1 optimal, 2 unbounded, 3 cycle, 4 infeasible, 5 iteration cap, 6 history full
    int outcome = 0, unbounded_col = 0;
    while (outcome == 0) {
        if (iters_left <= 0) { outcome = 5; break; }
        int pr = 0, pc = 0;
        if (phase == 1) {
            // leaving row: most negative RHS below -precision, first index on ties (simplex.ts:39-49)
            Cand best; best.v = -precision; best.i = 0; best.b = 0;
            for (int r = 1 + tid; r < H; r += THREADS) {
                const double v = A[r * S];
                if (v < best.v) { best.v = v; best.i = r; }
            }
            best = pk_reduce<THREADS>(best, MinFirst(), sm.g);
            if (best.i == 0) {  // :51-54 feasible: phase 2 starts in this same iteration with a fresh history (:102)
                phase = 2; entered2 = 1; hist_n = 0;
            } else {
                pr = best.i;
                // entering column: max -cost/coef over unrestricted or coef < -precision (simplex.ts:56-71)
                const double* row = A + pr * S;
                Cand q; q.v = -INFINITY; q.i = 0; q.b = 0;
                for (int col = 1 + tid; col < W; col += THREADS) {
                    const double coef = row[col];
                    const bool un = unr[vibc[col]] != 0;
                    if (un || coef < -precision) {
                        const double quo = -A[col] / coef;
                        if (q.v < quo) { q.v = quo; q.i = col; }
                    }
                }
                q = pk_reduce<THREADS>(q, MaxFirst(), sm.g);
                if (q.i == 0) { outcome = 4; break; }  // :73-76 infeasible
                pc = q.i;
            }
        }
        if (phase == 2) {
            // Dantzig pricing with the reference's batch rule (simplex.ts:118-219): the first batch holding a candidate
            // wins; inside it the largest value, first index on ties
            Cand e; e.v = precision; e.i = 0; e.b = 0;
            for (int col = 1 + tid; col < W; col += THREADS) {
                const double rc = A[col];
                const bool un = unr[vibc[col]] != 0;
                const int b = m.use_partial ? (col - 1) / m.batch : 0;
                const double val = (un && rc < 0) ? -rc : rc;
                if (val > precision) {
                    Cand cand; cand.v = val; cand.i = col; cand.b = b;
                    const bool take = PriceFirst()(cand, e);
                    e.v = take ? cand.v : e.v;
                    e.i = take ? cand.i : e.i;
                    e.b = take ? cand.b : e.b;
                }
            }
            e = pk_reduce<THREADS>(e, PriceFirst(), sm.g);
            int opt_row = -1;  // which optional objective named the entering column (-1: the cost row)
            if constexpr (OPT) {
                // simplex.ts:221-263 as select_step restates it: no column prices out on the cost row -> objective by objective in priority
                // order, among the columns within +-precision on the cost row and on every earlier objective (every batch was scanned
                // without a winner, so the deferred set spans all of them): the largest value above precision, first index on ties
                for (int o = 0; e.i == 0 && o < n_opt; o++) {
                    Cand x; x.v = precision; x.i = 0; x.b = 0;
                    for (int col = 1 + tid; col < W; col += THREADS) {
                        const double rc0 = A[col];
                        bool deferred = -precision < rc0 && rc0 < precision;
                        for (int q = 0; deferred && q < o; q++) {
                            const double rq = oo[q * S + col];
                            deferred = -precision < rq && rq < precision;
                        }
                        if (!deferred) continue;
                        const double rc = oo[o * S + col];
                        if (-precision < rc && rc < precision) continue;
                        const bool un = unr[vibc[col]] != 0;
                        const double val = (un && rc < 0) ? -rc : rc;
                        const bool take = val > x.v;  // strict: the first index wins ties inside a thread (my columns ascend)
                        x.v = take ? val : x.v;
                        x.i = take ? col : x.i;
                    }
                    e = pk_reduce<THREADS>(x, PriceFirst(), sm.g);
                    if (e.i != 0) opt_row = o;
                }
            }
            if (e.i == 0) { outcome = 1; break; }  // optimal (simplex.ts:265-269)
            pc = e.i;
            int neg_flag;
            {   // isReducedCostNegative of the winner, from the row that named it
                double rc = A[pc];
                if constexpr (OPT) { if (opt_row >= 0) rc = oo[opt_row * S + pc]; }
                neg_flag = (unr[vibc[pc]] != 0 && rc < 0) ? 1 : 0;
            }
            // ratio test (simplex.ts:271-296) in its order-free form: the first row passing the degenerate test wins
            // outright, otherwise the first-index argmin of the accepted quotients.  One reduction: an accepted quotient is above
            // precision > 0, so a degenerate row enters as -Infinity and MinFirst breaks the ties among them by the first index.
            Cand mq; mq.v = INFINITY; mq.i = 0; mq.b = 0;
            int rdeg = 0;
            for (int r = 1 + tid; r < H; r += THREADS) {
                const double colv = A[r * S + pc];
                const double rhs = A[r * S];
                if (-precision < colv && colv < precision) continue;
                if (colv > 0 && precision > rhs && rhs > -precision) {
                    if (rdeg == 0) rdeg = r;  // (my rows ascend)
                    continue;
                }
                const double quo = neg_flag ? -rhs / colv : rhs / colv;
                if (quo > precision && mq.v > quo) { mq.v = quo; mq.i = r; }
            }
            if (rdeg != 0) { mq.v = -INFINITY; mq.i = rdeg; }
            mq = pk_reduce<THREADS>(mq, MinFirst(), sm.g);
            if (mq.i == 0) { outcome = 2; unbounded_col = pc; break; }  // unbounded (simplex.ts:298-303)
            pr = mq.i;
        }
        const int leaving = vibr[pr], entering = vibc[pc];
        // cycle check (simplex.ts:78-93 / 305-320): append first, test, stop WITHOUT pivoting on a hit.  The host rebuilds the
        // reference's [start, length] message from the global copy.
        if (check_cycles) {
            if (hist_n >= m.hist_cap) { outcome = 6; break; }
            if (tid == 0) {
                const int2 pair = make_int2(leaving, entering);
                ghist[hist_n] = pair;
                if (hist_n < PK_HIST) sm.hist[hist_n] = pair;
            }
            __syncthreads();
            hist_n += 1;
            const bool cycle = hist_n <= PK_HIST ? suffix_is_square(sm.hist, hist_n, sm.g) : suffix_is_square(ghist, hist_n, sm.g);
            if (cycle) { outcome = 3; break; }
        }
        // ---- pivot(pr, pc) (simplex.ts:330-391) ------------------------------------------------------------------------------------
        const double quot = A[pr * S + pc];  // :335
        int any = 0;
        for (int r = tid; r < H; r += THREADS) {  // the pivot column: lane r reads A[r][pc], conflict-free with the odd stride
            const double k = A[r * S + pc];
            pcol[r] = k;
            any |= (r != pr && nonzero16(k)) ? 1 : 0;
        }
        // any row that will execute the inner loop of :367-391 lazily zeroes the tiny pivot-row entries
        const int anyrow = __syncthreads_or(any);  // (also orders the quot read above against the row write below)
        double* prow = A + pr * S;
        for (int col = tid; col < W; col += THREADS) {
            const double val = prow[col];
            const bool innz = nonzero16(val);                          // :356
            double v = innz ? val / quot : 0.0;                        // :357 / :361  (IEEE division)
            if (col == pc) v = 1.0 / quot;                             // :364
            if (innz && anyrow && !nonzero16(v) && v != 0.0) v = 0.0;  // :381-383
            prow[col] = v;
        }
        if (tid == 0) {  // :339-349
            vibr[pr] = entering;
            vibc[pc] = leaving;
            rbv[entering] = pr;
            rbv[leaving] = -1;
            cbv[entering] = -1;
            cbv[leaving] = pc;
            if (trace_n < m.trace_cap) gtrace[trace_n] = make_int2(pr, pc);
        }
        trace_n += 1;
        if (phase == 1) it1 += 1; else it2 += 1;
        iters_left -= 1;
        __syncthreads();  // the normalised pivot row and the pivot column are complete
        for (int r = rsub; r < H; r += RP) {
            const double k = pcol[r];
            if (r == pr || !nonzero16(k)) continue;  // the row gate, :370-375
            double* row = A + r * S;
            for (int col = col0; col < W; col += CW) {
                if (col == pc) { row[col] = -k / quot; continue; }  // :387 overwrites whatever the loop did to column pc
                const double p = prow[col];
                if (nonzero16(p)) row[col] = eliminate(row[col], k, p);  // :376-386, both roundings
            }
        }
        if constexpr (OPT) {
            // the optional objectives (simplex.ts:394-412) as prepare_pivot restates them: the same elimination with EXACT `!= 0` tests, on the
            // final pivot row (lazy zeroing included), one (objective, column) cell per thread and step.  Column pc waits for the barrier:
            // every thread has read an objective's coefficient before its owner overwrites it
            for (int q = tid; q < n_opt * W; q += THREADS) {
                const int o = q / W, col = q - o * W;
                if (col == pc) continue;
                double* rc = oo + o * S;
                const double coefficient = rc[pc];
                if (coefficient != 0.0) {
                    const double v0 = prow[col];
                    if (v0 != 0.0) rc[col] = eliminate(rc[col], coefficient, v0);
                }
            }
            __syncthreads();
            for (int o = tid; o < n_opt; o += THREADS) {
                const double coefficient = oo[o * S + pc];
                if (coefficient != 0.0) oo[o * S + pc] = -coefficient / quot;  // :410
            }
        }
        __syncthreads();
    }
    // ---- epilogue: everything back once -------------------------------------------------------------------------------------------
    __syncthreads();
    for (int q = tid; q < pairs; q += THREADS) {
        const int e = 2 * q, r = e / W, c = e - r * W;
        const bool wrap = c + 1 == W;
        double2 v;
        v.x = A[r * S + c];
        v.y = e + 1 < cells ? A[(wrap ? r + 1 : r) * S + (wrap ? 0 : c + 1)] : 0.0;
        gA[q] = v;
    }
    for (int q = tid; q < words; q += THREADS) gI[q] = reinterpret_cast<const int4*>(ints)[q];
    for (int r = tid; r < H; r += THREADS) {
        out_rhs[m.out_off + r] = A[r * S];
        out_rows[m.out_off + r] = vibr[r];
    }
    if constexpr (OPT) {  // the final rows: into the image (a second call continues from them) and home with the result block
        double* out_opt = many_global(m.opt_out);
        for (int q = tid; q < n_opt * W; q += THREADS) {
            const int o = q / W;
            const double v = oo[o * S + (q - o * W)];
            gO[q] = v;
            out_opt[q] = v;
        }
    }
    if (tid == 0) {
        st->phase = phase;
        st->it1 = it1;
        st->it2 = it2;
        st->hist_n = hist_n;
        st->iters_left = iters_left;
        st->trace_n = trace_n;
        st->entered_phase2 = entered2;
        if (entered2) st->feasible = 1;
        if (outcome == 1) st->optimal = 1;
        if (outcome == 2) { st->bounded = 0; st->unbounded_var = vibc[unbounded_col]; }
        if (outcome == 3) { st->cycle_phase = phase; st->feasible = 0; }
        if (outcome == 4) st->feasible = 0;
        if (outcome == 5) st->err = ERR_ITER_LIMIT;
        if (outcome == 6) st->err = ERR_HIST_FULL;
        st->status = ST_DONE;
        st->do_pivot = 0;
        st->obj_cell = A[0];
    }
    __syncthreads();
    static_assert(sizeof(DevState) % 8 == 0 && sizeof(DevState) / 8 <= 64, "DevState is copied by one wave, a word per lane");
    if (tid < (int)(sizeof(DevState) / 8))
        reinterpret_cast<long long*>(out_states + idx)[tid] = reinterpret_cast<const long long*>(st)[tid];
}

// ---- which builds of the pack kernels this unit holds ------------------------------------------------------------------------------------
// JSLP_PACK_BUILDS: a mask with bit (1 << PackKind) set for every build the unit instantiates, in plain numbers so that it also works in an #if.
// Not given: every build (0x1f, the single-unit build).  0x03: k_simplex_packed and the plain and OPT builds of k_tree_packed
// (jslp_tu_packed.hip); 0x04, 0x08, 0x10: the MIR, ENH, INC builds of k_tree_packed (jslp_tu_tree_mir.hip, _enh, _inc).  A launch of a build
// that is not the unit's own instantiates nothing (pack_dispatch, jslp_tree.hip.h, then answers -1), as res_row_built does for the
// register-resident kernel.
#ifndef JSLP_PACK_BUILDS
#define JSLP_PACK_BUILDS 0x1f
#endif
static_assert((1 << PACK_PLAIN | 1 << PACK_OPT) == 0x03 && 1 << PACK_MIR == 0x04 && 1 << PACK_ENH == 0x08 && 1 << PACK_INC == 0x10, "the units' masks name these builds");
constexpr bool pack_build_here(int build) { return ((JSLP_PACK_BUILDS) >> build & 1) != 0; }
// JSLP_PACK_TOL: which side of k_tree_packed's TOL flag (include/jslpg_tree_tolerance.h) the unit instantiates -- 0 (not given in a unit
// that names its builds): the builds without it, and k_simplex_packed, as before there was such a flag; 1: the TOL twins of the unit's
// builds alone (jslp_tu_tree_tol.hip: a unit of their own, so that the other units compile what they compiled); 2: both (the single-unit build).
#ifndef JSLP_PACK_TOL
#define JSLP_PACK_TOL 2
#endif
constexpr bool pack_tol_here(bool tol) { return (JSLP_PACK_TOL) == 2 || ((JSLP_PACK_TOL) == 1) == tol; }
// JSLP_PACK_BIG: which side of the large class (include/jslpb_big_lds.h) the unit instantiates -- 0 (every unit that names its builds): the
// 64- and 256-thread builds, as before there was such a class; 1: the large builds of the unit's kinds alone (jslp_tu_packed_big.hip: a unit
// of their own, so that the other units compile what they compiled); 2 (not given): both (the single-unit build).
#ifndef JSLP_PACK_BIG
#define JSLP_PACK_BIG 2
#endif
constexpr bool pack_big_here(bool big) { return (JSLP_PACK_BIG) == 2 || ((JSLP_PACK_BIG) == 1) == big; }
// A large build's launch: the first one on a device raises the kernel's dynamic-LDS ceiling to PACK_BIG_LDS (the runtime refuses more than
// 64 KiB without it) and holds static plus dynamic LDS to the compute unit's 160 KiB.  Returns hipSuccess, or the error that forbids the launch.
template <class Kernel>
static hipError_t pack_big_prepare(Kernel kernel, size_t lds, unsigned long long* ready) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(__atomic_load_n(ready, __ATOMIC_ACQUIRE) & bit)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, PACK_BIG_LDS);
        if (e != hipSuccess) return e;
        hipFuncAttributes fa;
        e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel));
        if (e != hipSuccess) return e;
        // sharedSizeBytes + lds <= 160 KiB for every lds a launch may come with (the unit's static_assert holds the structs to the reserve)
        if (fa.sharedSizeBytes + (size_t)PACK_BIG_LDS > (size_t)PACK_CU_LDS) return hipErrorLaunchOutOfResources;
        __atomic_fetch_or(ready, bit, __ATOMIC_RELEASE);
    }
    return lds <= (size_t)PACK_BIG_LDS ? hipSuccess : hipErrorLaunchOutOfResources;
}

// one build of k_simplex_packed: launches when (threads, a.build) and the class of `lds` are its own.  BIG: a large build -- *err is what
// forbade its launch, if anything did
template <int T, int BUILD, bool BIG = false>
static bool pk_launch(int threads, unsigned grid, size_t lds, const PackLaunch& a, hipStream_t s, hipError_t* err) {
    if constexpr (!pack_build_here(BUILD) || !pack_tol_here(false) || !pack_big_here(BIG)) {
        return false;
    } else {
        if (threads != T || a.build != BUILD || (lds > PACK_SMALL_LDS) != BIG) return false;
        if constexpr (BIG) {
            static unsigned long long ready = 0;
            *err = pack_big_prepare(k_simplex_packed<T, BUILD == PACK_OPT>, lds, &ready);
            if (*err != hipSuccess) return true;
        }
        hipLaunchKernelGGL((k_simplex_packed<T, BUILD == PACK_OPT>), dim3(grid), dim3(T), lds, s, a.lps, a.order, a.cc, a.cc_all, static_cast<DevState*>(a.states), a.rhs,
                           a.rows);
        return true;
    }
}
#endif  // JSLP_PACKED_KERNELS
