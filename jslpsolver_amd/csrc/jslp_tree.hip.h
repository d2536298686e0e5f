// jslp_tree.hip.h -- the branch-and-bound tree of every LP of a pack, walked inside ONE launch (include/jslpt_tree.h): one workgroup per
// LP holds the tableau at its ROW CAPACITY in LDS (jslp_packed.hip.h's layout with RC rows) and runs the default service's loop
// (branch-and-cut.ts:54-199) itself: pop, prune, restore + addCutConstraints + simplex, isIntegral / getMostFractionalVar, the two pushes.
//
// Two parts like jslp_packed.hip.h (included behind it, once per unit): the layout (always) and the kernels (-DJSLP_PACKED_KERNELS).
//
// Memory of one LP:
//   LDS     the tableau RC x S doubles, the pivot column, (the optional rows, n_opt x S,) the integer block sized for RC rows --
//           jslpt_lds_bytes / jslps_tree_lds_bytes; (a MIR LP, include/jslpc_tree_mir.h: one isInteger byte per variable index behind it --
//           jslpc_tree_lds_bytes;)
//   image   [DevState | matrix | integer block | n_int, the integer variables' indexes]: the upload, and from iteration 1 on the SAVED
//           ROOT (written once, read by every later node: an L2-resident restore; the tableau is never written back);
//   heap    heap_cap entries of 16 bytes {relaxedEvaluation, seq, slot} -- min-heap.ts as it is, executed by thread 0;
//   pool    heap_cap + 3 cut lists of cut_rows cuts (16 bytes each) behind a 16-byte header: one per heap entry, the node under
//           evaluation, the incumbent, and the list being built; a free stack hands the slots out.
// Every scalar of the tree (the incumbent's evaluation, the counters, the heap size) is computed by every thread alike and lives in
// registers; thread 0 alone touches the heap and the pool and publishes what the others need through LDS.
#ifndef JSLP_TREE_LAYOUT
#define JSLP_TREE_LAYOUT

struct TreeCut { double value; int32_t var; int32_t type; };    // type 0 = "min" (x >= value), 1 = "max" (x <= value), as Cuts::type
struct TreeEntry { double key; int32_t seq; int32_t slot; };    // slot -1: the empty cut list of the root
struct TreeMirRec { int32_t rounds, rows_added, simplexes, root_rows, rows_high_water, pad[3]; };  // what a MIR build reports per LP: jslpc_mir_result field for field
// An enhanced LP (include/jslpe_tree_enhanced.h) runs in the ENH build of the kernel.  Its LDS image is a tree LP's; what the enhanced service
// adds lives in global memory and is thread 0's alone, like the heap: the depth-first stack grows DOWN from the top of the heap array (stack
// and heap share its heap_cap entries), and behind the array lies the pseudocost table, one TreePseudo per integer variable in model order.
// A cut of such an LP carries that position in its type: type = (position << 1) | ("max" ? 1 : 0).
struct TreePseudo { double up_sum, down_sum; int32_t up_count, down_count, pad[2]; };
struct TreeEnhRec { int32_t solutions_found, stack_high_water, moved_to_heap, pseudo_updates, scored_by_pseudocost, dropped_nodes, pad[2]; };  // jslpe_tree_result
// An incremental LP (include/jslpi_tree_incremental.h) runs in the INC build of the kernel: an enhanced LP's memory, with the checkpoint arena
// behind the pseudocost table -- max_checkpoints slots of tree_ckpt_bytes each: a TreeCkptHead, the rows of the row capacity at stride W in
// 16-byte words (the saved root's layout), the whole integer block.  Its policy carries max_checkpoints above the two rules (<< 8).  The
// checkpoint an entry starts from rides in its cut list's header, behind the length: TREE_CK_NO_CUT (a best-first child: no new cut, no
// checkpoint), TREE_CK_NONE (a new cut -- the list's last -- but no checkpoint: the budget was spent), or the checkpoint's number.
// The LP's TreeIncRec follows its TreeEnhRec in the result block.
struct TreeCkptHead { int32_t height, feasible; double evaluation; };
struct TreeIncRec { int32_t checkpoints_used, incremental_nodes, rows_high_water, checkpoint_rows_high_water, pad[4]; };  // jslpi_tree_result
// An LP with options.tolerance (include/jslpg_tree_tolerance.h) runs in the TOL build of its kind.  TreeLp and the kernel's arguments are what
// they were: what such an LP adds rides in the three spare words of its image's integer-variable header (behind n_int) -- word 1 the distance,
// in units of 256 bytes, from the pack's TreeRec array to its TreeTolRec array in the result block, words 2 and 3 the factor, the host's
// 1 + tolerance (a minimisation) or 1 - tolerance (a maximisation), any double.
struct TreeTolRec { double best_possible, threshold; int32_t stopped, left, pad[2]; };  // jslpg_tolerance_result
enum { TREE_CK_NO_CUT = -2, TREE_CK_NONE = -1, TREE_MAX_CHECKPOINTS = 64 };
enum { ENH_BEST_FIRST = 1, ENH_DEPTH_FIRST = 2, ENH_HYBRID = 3, ENH_MOST_FRACTIONAL = 1, ENH_PSEUDOCOST = 2, ENH_STRONG = 3, ENH_STRONG_CANDIDATES = 5 };
struct TreeLp {
    TreeEntry* heap;
    char* pool;
    int32_t* free_list;
    double rcoef;  // Math.round(1 / precision), computed on the host like decode_state's
    int32_t cut_rows, heap_cap, max_nodes;
    int32_t policy;  // 0: the default service; an enhanced LP: node selection | branching << 4 (ENH_*); an incremental LP: the same | max_checkpoints << 8
    union {
        double* best_opt;     // n_opt doubles next to the heap: column 0 of the incumbent's optional rows (thread 0 alone reads and writes them)
        TreeMirRec* mir_out;  // a MIR LP (include/jslpc_tree_mir.h; never one with optional objectives): its record in the result block
        TreeEnhRec* enh_out;  // an enhanced LP (never one with optional objectives or MIR): its record in the result block (an incremental LP: its TreeIncRec behind it)
    };
};
enum { TREE_OK = 0, TREE_ERR_NODES = 1, TREE_ERR_HEAP = 2, TREE_ERR_CUTS = 3, TREE_ERR_BRANCH = 4, TREE_ERR_MIR_ROWS = 5, TREE_ERR_MIR_ROUNDS = 6, TREE_ERR_INC_ROWS = 7 };
struct TreeRec {  // what the kernel reports per LP next to its DevState
    double evaluation;
    int32_t iterations, is_integral, final_height, nodes_pushed, heap_high_water, cuts_high_water, err, pad;
};
__host__ __device__ __forceinline__ long long tree_slot_bytes(int32_t cut_rows) { return 16LL * (1 + cut_rows); }
__host__ __device__ __forceinline__ long long tree_pseudo_bytes(int32_t RC, int32_t W) { return (long long)sizeof(TreePseudo) * pk_n_idx(RC, W); }  // (an LP has at most n_idx integer variables)
__host__ __device__ __forceinline__ long long tree_ckpt_bytes(int32_t RC, int32_t W) {  // one checkpoint slot of an incremental LP
    return (long long)sizeof(TreeCkptHead) + 16 * (((long long)RC * W + 1) >> 1) + 4LL * pk_ints(RC, W).total;
}
__host__ __device__ __forceinline__ long long tree_ivars_bytes(int32_t RC, int32_t W) { return 16 + 4LL * pk_pad4(pk_n_idx(RC, W)); }
// A MIR LP (include/jslpc_tree_mir.h) runs in a MIR build of the kernel.  Its LDS image is the tree LP's at its row capacity with
// variable.isInteger per variable index behind the integer block: n_idx bytes padded to 16, built by the kernel from the image's list of
// integer variables (the image itself is a tree LP's).  jslpc_tree_lds_bytes is tree_mir_lds_bytes.
#define TMIR_MAX_ROUNDS 64  // rounds of ONE node: JSLPR_MAX_ROUNDS of include/jslpr_mir.h (static_assert in jslp_hip.hip)
__host__ __device__ __forceinline__ int32_t tree_mir_flag_words(int32_t RC, int32_t W) { return pk_pad4((pk_n_idx(RC, W) + 3) / 4); }
__host__ __device__ __forceinline__ long long tree_mir_lds_bytes(int32_t RC, int32_t W) { return pk_lds_bytes(RC, W) + 4LL * tree_mir_flag_words(RC, W); }
#endif  // JSLP_TREE_LAYOUT

#if defined(JSLP_PACKED_KERNELS) && !defined(JSLP_TREE_KERNELS_DONE)
#define JSLP_TREE_KERNELS_DONE
#include "jslp_tree_mir.hip.h"  // the device functions of the MIR builds

struct TreeSmem {
    PackSmem ps;
    double key;                // the popped entry's relaxedEvaluation
    int32_t slot, code, n_high, n_low;
};

// min-heap.ts:43-49
__device__ __forceinline__ bool tree_before(const TreeEntry& a, const TreeEntry& b) {
    if (a.key != b.key) return a.key < b.key;
    return a.seq > b.seq;
}
// min-heap.ts push (thread 0): the bubble-up loop with a hole
__device__ __forceinline__ void tree_push(TreeEntry* h, int n, TreeEntry e) {
    int i = n;
    while (i > 0) {
        const int p = (i - 1) >> 1;
        const TreeEntry pe = h[p];
        if (!tree_before(e, pe)) break;
        h[i] = pe;
        i = p;
    }
    h[i] = e;
}
// min-heap.ts pop (thread 0): n = entries before the pop
__device__ __forceinline__ TreeEntry tree_pop(TreeEntry* h, int n) {
    const TreeEntry top = h[0];
    const TreeEntry last = h[n - 1];
    n -= 1;
    if (n == 0) return top;
    int i = 0;
    const int half = n >> 1;
    while (i < half) {
        int c = 2 * i + 1;
        TreeEntry ce = h[c];
        if (c + 1 < n) {
            const TreeEntry re = h[c + 1];
            if (tree_before(re, ce)) { c += 1; ce = re; }
        }
        if (!tree_before(ce, last)) break;
        h[i] = ce;
        i = c;
    }
    h[i] = last;
    return top;
}
// Math.round (ties toward +Infinity; the subtraction is exact), as branch_acc_add's
__device__ __forceinline__ double tree_round(double x) {
    if (!(fabs(x) < INFINITY)) return x;
    const double f = floor(x);
    return (x - f >= 0.5) ? f + 1.0 : f;
}

// Tableau.solve() of LP order[blockIdx.x] under the default branch-and-cut service.  THREADS as k_simplex_packed.  Bounded: every
// simplex by the pivot cap, the node loop by max_nodes evaluations and by the heap (each iteration pops one entry; pushes are
// bounded by heap_cap); the kernel waits on nothing outside its workgroup.
// OPT = true: the LPs with optional objectives (include/jslps_soft.h).  Their rows are saved with the root and come back with every restore
// (backup.ts:35-43, 94-104), addCutConstraints leaves them alone, and a node whose evaluation EQUALS the incumbent's is compared with it
// objective by objective on column 0 of the rows (branch-and-cut.ts:107-127).
// MIR = true: the LPs of a model with options.useMIRCuts (include/jslpc_tree_mir.h; never with OPT).  Every node's simplex -- the root's, a
// later node's, the final re-evaluation's -- is followed by the loop of branch-and-cut.ts:38-52: computeFractionalVolume(true), applyMIRCuts,
// simplex again, the volume again, until it shrinks by less than 10 % (jslp_tree_mir.hip.h).  The root's MIR rows are appended before
// save(): the saved root is Hs >= H0 rows tall and every later node starts from it.  Each simplex of the loop has the pivot cap and the
// cycle-check history of a call of its own, and folds feasible / bounded / evaluation as a node's does.  Bounded like everything else: a
// round whose rows exceed the row capacity, and TMIR_MAX_ROUNDS rounds of one node without a stop, end the LP with an error of its own.
// MIR = false instantiates the kernel as it was before there was such a build.
// ENH = true: the LPs of a model with options.nodeSelection / options.branching (include/jslpe_tree_enhanced.h; never with OPT or MIR), under the
// enhanced service (enhanced-branch-and-cut.ts:223-434).  The tableau, the saved root, the cut rows and the simplex are the default
// service's; the tree policy differs: a depth-first stack beside the heap and the hybrid switch at the first incumbent, the pseudocost
// table with its order-dependent update, and selectBranchingVariable (:112-196) scanned across the lanes.  Node selection and branching
// rule are the LP's own (TreeLp::policy), uniform across its workgroup.  ENH = false instantiates the kernel, instruction for instruction,
// as it was before there was such a build.
// INC = true (with ENH, whose machinery it is built on): the LPs of a model with options.useIncremental (include/jslpi_tree_incremental.h), under
// the incremental service (incremental-branch-and-cut.ts:280-496).  The enhanced walk, with parent checkpoints: a node that branches
// while the walk is depth-first copies its solved tableau into the LP's arena (checkpoint_save, the whole workgroup), and a child that
// carries one starts from it with ONE new cut row (checkpoint_restore + add_cuts_at) instead of the root and its whole list.  Pseudocosts
// are updated from a node's new cut only, `strong` means pseudocost, and a checkpoint brings its evaluation with it.  INC = false
// instantiates the kernel as it was before there was such a build.
// TOL = true (with any of the above): the LPs of a model with options.tolerance (include/jslpg_tree_tolerance.h).  bestPossibleEval is the
// evaluation of the LP's first simplex that ends optimal (tableau.ts:420-430, `simplexIters === 0`); the threshold is looked at at the top of
// every turn behind the emptiness test and BEFORE the pop, and a turn that finds the incumbent below it lowers toleranceFlag and still runs:
// the loop ends at the next turn's condition (branch-and-cut.ts:73-87).  Every line of it is under `if constexpr (TOL)`: TOL = false
// instantiates the kernel, instruction for instruction, as it was before there was such a build.
template <int THREADS, bool OPT, bool MIR = false, bool ENH = false, bool INC = false, bool TOL = false>
__global__ void __launch_bounds__(THREADS) k_tree_packed(const PackLp* __restrict__ lps, const TreeLp* __restrict__ trees, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ cc, int cc_all, DevState* __restrict__ out_states,
                                                         double* __restrict__ out_rhs, int32_t* __restrict__ out_rows, TreeRec* __restrict__ out_tree) {
    extern __shared__ __attribute__((aligned(16))) double pk_lds[];
    __shared__ TreeSmem sm;
    __shared__ TreeMirSm ms;  // (MIR; no other build refers to it)
    static_assert(!(MIR && OPT), "a MIR LP has no optional objectives (include/jslpc_tree_mir.h)");
    static_assert(!(ENH && (OPT || MIR)), "an enhanced LP has neither optional objectives nor MIR cuts (include/jslpe_tree_enhanced.h)");
    static_assert(!(INC && (OPT || MIR)), "an incremental LP has neither optional objectives nor MIR cuts (include/jslpi_tree_incremental.h)");
    static_assert(!INC || ENH, "the INC build is the ENH build with checkpoints");
    const int idx = order[blockIdx.x];
    const PackLp m = lps[idx];
    const TreeLp t = trees[idx];
    const int tid = threadIdx.x;
    const int H0 = m.H, W = m.W, RC = m.RC, S = pk_stride(W);
    const PackInts io = pk_ints(RC, W);
    const double precision = m.precision;
    const int check_cycles = cc ? cc[idx] : cc_all;
    int n_opt = 0;
    if constexpr (OPT) n_opt = m.n_opt;
    double* A = pk_lds;
    double* pcol = pk_lds + RC * S;
    double* oo = pcol + RC;  // (OPT) the optional rows, stride S
    int32_t* ints = reinterpret_cast<int32_t*>(pk_lds + pk_lds_doubles(RC, W, n_opt));
    int32_t* vibr = ints + io.vibr;
    int32_t* vibc = ints + io.vibc;
    int32_t* rbv = ints + io.rbv;
    int32_t* cbv = ints + io.cbv;
    const uint8_t* unr = reinterpret_cast<const uint8_t*>(ints + io.unr);
    uint8_t* is_int = reinterpret_cast<uint8_t*>(ints + io.total);  // (MIR) variable.isInteger per variable index, behind the integer block
    char* image = many_global(m.image);
    DevState* st = reinterpret_cast<DevState*>(image);
    double2* gA = reinterpret_cast<double2*>(image + sizeof(DevState));
    int4* gI = reinterpret_cast<int4*>(image + sizeof(DevState) + 8 * pk_image_doubles(RC, W, n_opt));
    const int32_t* gV = reinterpret_cast<const int32_t*>(image + sizeof(DevState) + 8 * pk_image_doubles(RC, W, n_opt) + 4LL * io.total);
    double* gO = reinterpret_cast<double*>(image + sizeof(DevState)) + pk_opt_image_off(RC, W);  // (OPT) the optional rows, stride W
    double* best_opt = many_global(t.best_opt);
    const int n_int = gV[0];
    const int32_t* ivars = gV + 4;
    int2* ghist = many_global(m.hist);
    int2* gtrace = many_global(m.trace);
    TreeEntry* heap = many_global(t.heap);
    char* pool = many_global(t.pool);
    int32_t* free_list = many_global(t.free_list);
    const long long slot_bytes = tree_slot_bytes(t.cut_rows);

    // `rows` rows and the whole integer block, global <-> LDS in 16-byte words (stride W <-> stride S; a word may hold the last cell of one row
    // and the first of the next, and the last word half a pair when rows * W is odd): the saved root's, and (INC) a checkpoint's
    int Hs = H0;  // rows of the saved root: the LP's own, (MIR) with the root's MIR rows from save() on
    const int words = io.total >> 2;
    auto rows_in = [&](const double2* srcA, const int4* srcI, int rows) {
        const int cells = rows * W, pairs = (cells + 1) >> 1;
        for (int q = tid; q < pairs; q += THREADS) {
            const double2 v = srcA[q];
            const int e = 2 * q, r = e / W, c = e - r * W;
            A[r * S + c] = v.x;
            if (e + 1 < cells) {
                const bool wrap = c + 1 == W;
                A[(wrap ? r + 1 : r) * S + (wrap ? 0 : c + 1)] = v.y;
            }
        }
        for (int q = tid; q < words; q += THREADS) reinterpret_cast<int4*>(ints)[q] = srcI[q];
    };
    auto rows_out = [&](double2* dstA, int4* dstI, int rows) {
        const int cells = rows * W, pairs = (cells + 1) >> 1;
        for (int q = tid; q < pairs; q += THREADS) {
            const int e = 2 * q, r = e / W, c = e - r * W;
            const bool wrap = c + 1 == W;
            double2 v;
            v.x = A[r * S + c];
            v.y = e + 1 < cells ? A[(wrap ? r + 1 : r) * S + (wrap ? 0 : c + 1)] : 0.0;
            dstA[q] = v;
        }
        for (int q = tid; q < words; q += THREADS) dstI[q] = reinterpret_cast<const int4*>(ints)[q];
    };
    // the saved root: image <-> LDS
    auto restore = [&]() {
        rows_in(gA, gI, Hs);
        if constexpr (OPT)
            for (int q = tid; q < n_opt * W; q += THREADS) {
                const int o = q / W;
                oo[o * S + (q - o * W)] = gO[q];
            }
    };
    auto save = [&]() {
        rows_out(gA, gI, Hs);
        if constexpr (OPT)
            for (int q = tid; q < n_opt * W; q += THREADS) {
                const int o = q / W;
                gO[q] = oo[o * S + (q - o * W)];
            }
    };
    // addCutConstraints (cutting-strategies.ts:16-72) of the list in `slot` on the restored root: every cut row reads rows below Hs
    // and the restored maps only, so the rows are built side by side, one (cut, column) cell per thread and step; returns the height
    // ((MIR) or -1 with nothing written: the root's MIR rows have left the list no room below the row capacity).  In general the list's cuts
    // from `first` on, on a tableau `base` rows tall: the restored root and 0, or (INC) a restored checkpoint and the list's last cut
    auto add_cuts_at = [&](int slot, int base, int first) -> int {
        if (slot < 0) return base;
        const char* sp = pool + slot * slot_bytes;
        const int n = *reinterpret_cast<const int32_t*>(sp) - first;
        if constexpr (MIR)
            if (base + n > RC) return -1;
        const TreeCut* cuts = reinterpret_cast<const TreeCut*>(sp + 16) + first;
        for (int q = tid; q < n * W; q += THREADS) {
            const int h = q / W, col = q - h * W;
            TreeCut c = cuts[h];
            if constexpr (ENH) c.type &= 1;  // (the integer variable's position rides above bit 0)
            const double sign = c.type == 0 ? -1.0 : 1.0;  // "min" -> -1 (:41)
            const int var_row = rbv[c.var], var_col = cbv[c.var];
            double v = 0.0;
            if (var_row == -1) {  // non-basic variable: unit row (:46-53)
                if (col == 0) v = sign * c.value;
                else if (col == var_col) v = sign;
            } else {              // basic variable: negated copy of its row (:54-62)
                const double s = A[var_row * S + col];
                v = col == 0 ? sign * (c.value - s) : -sign * s;
            }
            A[(base + h) * S + col] = v;
        }
        __syncthreads();  // (the maps read above are written below)
        for (int h = tid; h < n; h += THREADS) {  // getNewElementIndex + map updates (:64-69)
            const int slack = W + base - 2 + h;
            vibr[base + h] = slack;
            rbv[slack] = base + h;
            cbv[slack] = -1;
        }
        return base + n;
    };
    auto add_cuts = [&](int slot) -> int { return add_cuts_at(slot, Hs, 0); };

    if constexpr (MIR) {  // variable.isInteger, from the image's list (restore() below moves the integer block in front of it only)
        for (int q = tid; q < tree_mir_flag_words(RC, W); q += THREADS) reinterpret_cast<int32_t*>(is_int)[q] = 0;
        __syncthreads();
        for (int k = tid; k < n_int; k += THREADS) is_int[ivars[k]] = 1;
    }
    // (ENH) the pseudocost table behind the heap array: every call starts with none (pseudoCosts = new Map(), :69)
    TreePseudo* pseudo = reinterpret_cast<TreePseudo*>(heap + t.heap_cap);
    if constexpr (ENH)
        for (int k = tid; k < n_int; k += THREADS) {
            TreePseudo z; z.up_sum = 0.0; z.down_sum = 0.0; z.up_count = 0; z.down_count = 0; z.pad[0] = z.pad[1] = 0;
            pseudo[k] = z;
        }
    // (INC) the checkpoint arena behind the pseudocost table.  checkpoint_save: what LDS holds now -- the node's solved tableau, H rows, and
    // the whole integer block -- into slot k, with tableau.evaluation and tableau.feasible (createCheckpoint, :55-70); checkpoint_restore:
    // slot k back (restoreCheckpoint, :72-107), returns its head.  The copies are the whole workgroup's, like save() / restore(); thread 0
    // writes the head; the caller places the barriers.  A slot is written once per call (the counter only goes up) and read after a barrier.
    char* ck_arena = reinterpret_cast<char*>(pseudo) + tree_pseudo_bytes(RC, W);
    const long long ck_bytes = tree_ckpt_bytes(RC, W), ck_ints_off = ck_bytes - 4LL * io.total;
    auto checkpoint_save = [&](int k, int rows, double eval, int feas) {
        char* cp = ck_arena + k * ck_bytes;
        if (tid == 0) {
            TreeCkptHead h; h.height = rows; h.feasible = feas; h.evaluation = eval;
            *reinterpret_cast<TreeCkptHead*>(cp) = h;
        }
        rows_out(reinterpret_cast<double2*>(cp + sizeof(TreeCkptHead)), reinterpret_cast<int4*>(cp + ck_ints_off), rows);
    };
    auto checkpoint_restore = [&](int k) -> TreeCkptHead {
        const char* cp = ck_arena + k * ck_bytes;
        const TreeCkptHead h = *reinterpret_cast<const TreeCkptHead*>(cp);
        rows_in(reinterpret_cast<const double2*>(cp + sizeof(TreeCkptHead)), reinterpret_cast<const int4*>(cp + ck_ints_off), h.height);
        return h;
    };
    restore();
    long long trace_n = st->trace_n;
    if constexpr (OPT)  // bestOptionalObjectivesEvaluations (:66-69)
        if (tid == 0)
            for (int o = 0; o < n_opt; o++) best_opt[o] = INFINITY;
    __syncthreads();

    int H = H0, feasible = 1, unb_var = -1, iters_left = m.iters_cap;
    PkRun o;
    double evaluation = 0.0, best_eval = INFINITY;
    int iterations = 0, found = 0, best_slot = -1, have_best = 0, cur_slot = -1;
    int heap_n = 0, seq = 1, free_n = 0, fresh_n = 0, pushes = 1, heap_hw = 1, cuts_hw = 0;  // (the root's push and pop are not executed)
    int terr = (n_int > 0 && t.heap_cap < 1) ? (int)TREE_ERR_HEAP : (int)TREE_OK, serr = ERR_NONE;
    bool root = true, done = false;
    // (ENH) the enhanced service's registers, uniform like the others: which container the next node comes from, the stack's size, and
    // what the LP's TreeEnhRec reports.  The root starts on the stack unless the selection is best-first (:246-255); the heap's sequence
    // numbers count its own pushes only.
    // (INC) `strong` does not exist in the incremental service and means pseudocost (:202-219); max_checkpoints rides above the two rules
    const int node_sel = t.policy & 15;
    const int branching = INC ? (((t.policy >> 4) & 15) == ENH_STRONG ? (int)ENH_PSEUDOCOST : (t.policy >> 4) & 15) : t.policy >> 4;
    const int max_ck = INC ? min(t.policy >> 8, (int)TREE_MAX_CHECKPOINTS) : 0;
    // (INC) checkpoints taken (the next free slot), nodes that started from one, the tallest tableau and the tallest checkpoint; what the
    // node under evaluation starts from and what its children will (TREE_CK_*, or a checkpoint's number)
    int ck_count = 0, inc_nodes = 0, rows_hw = H0, ck_rows_hw = H0, cur_ck = TREE_CK_NO_CUT, child_ck = TREE_CK_NO_CUT;
    bool use_df = ENH && node_sel != ENH_BEST_FIRST;
    int stack_n = 0, stack_hw = use_df ? 1 : 0, solutions = 0, moved = 0, pseudo_updates = 0, scored = 0, dropped = 0;
    if constexpr (ENH)
        if (use_df) seq = 0;
    double parent_eval = 0.0;  // (declared out here: a declaration inside the node loop changes the code of the other builds)
    auto release = [&](int slot) {  // a cut list nobody refers to any more goes back on the free stack
        if (slot < 0) return;
        if (tid == 0) free_list[free_n] = slot;
        free_n += 1;
    };
    // (TOL) bestPossibleEval * factor as of now (0 * factor until the first optimum), whether bestPossibleEval is still open, !toleranceFlag,
    // whether the loop ended on it, and the LP's record: best_possible and the last threshold go there as they arise (thread 0)
    double tol_threshold = 0.0, tol_factor = 0.0;
    bool bp_open = true, tol_stop = false, tol_broke = false;
    TreeTolRec* tol_rec = nullptr;
    if constexpr (TOL) {
        tol_factor = __hiloint2double(gV[3], gV[2]);
        tol_rec = reinterpret_cast<TreeTolRec*>(reinterpret_cast<char*>(out_tree) + 256LL * gV[1]) + idx;
        tol_threshold = __dmul_rn(0.0, tol_factor);  // (the root's turn: its threshold is the record's first, and an incumbent of +Infinity lowers no flag)
        if (tid == 0) {
            TreeTolRec z; z.best_possible = 0.0; z.threshold = tol_threshold; z.stopped = 0; z.left = 0; z.pad[0] = z.pad[1] = 0;
            *tol_rec = z;
        }
    }
    // (MIR) the loop behind a node's simplex (branch-and-cut.ts:38-52); false: the LP has ended with terr or serr set
    int mir_rounds = 0, mir_rows = 0, mir_simplexes = 0, mir_tallest = H0;
    auto mir_loop = [&]() -> bool {
        if constexpr (MIR) {
            double before = tmir_volume<THREADS>(A, S, vibr, H, is_int, precision, pcol, ms);
            for (int round = 0;; round++) {
                if (round >= TMIR_MAX_ROUNDS) { terr = TREE_ERR_MIR_ROUNDS; return false; }
                const int n = tmir_append<THREADS>(A, S, W, H, RC, vibr, vibc, rbv, cbv, is_int, precision, ms);
                if (n < 0) { terr = TREE_ERR_MIR_ROWS; return false; }
                H += n;
                mir_rounds += 1;
                mir_rows += n;
                mir_simplexes += 1;
                mir_tallest = max(mir_tallest, H);
                iters_left = m.iters_cap;
                o = pk_simplex<THREADS, OPT>(A, pcol, H, W, S, vibr, vibc, rbv, cbv, unr, precision, check_cycles, m, ghist, gtrace, sm.ps, iters_left, trace_n, oo, n_opt);
                __syncthreads();
                if (o.outcome >= 5) { serr = o.outcome == 5 ? (int)ERR_ITER_LIMIT : (int)ERR_HIST_FULL; return false; }
                feasible = (o.outcome == 3 || o.outcome == 4) ? 0 : 1;
                unb_var = o.outcome == 2 ? vibc[o.unbounded_col] : -1;
                if (o.outcome == 1)
                    evaluation = __ddiv_rn(tree_round(__dmul_rn(__dadd_rn(2.220446049250313e-16, A[0]), t.rcoef)), t.rcoef);
                else if (o.outcome == 2)
                    evaluation = -INFINITY;
                if constexpr (TOL)  // setEvaluation while simplexIters === 0 (tableau.ts:420-430): the LP's first optimum is bestPossibleEval
                    if (o.outcome == 1 && bp_open) {
                        if (tid == 0) tol_rec->best_possible = evaluation;
                        tol_threshold = __dmul_rn(evaluation, tol_factor);
                        bp_open = false;
                    }
                const double after = tmir_volume<THREADS>(A, S, vibr, H, is_int, precision, pcol, ms);
                if (after >= 0.9 * before) return true;  // (false for NaN: the loop goes on, as the reference's does)
                before = after;
            }
        }
        return true;
    };

    while (terr == TREE_OK && !done) {
        if (!root) {
            if constexpr (ENH) {  // :257-280: the stack's top while the walk is depth-first, the heap's best after
                if ((use_df ? stack_n : heap_n) == 0) break;
                if constexpr (TOL) {  // the loop condition's toleranceFlag, then :73-87 -- before the pop; strict, false for NaN
                    if (tol_stop) { tol_broke = true; break; }
                    if (tid == 0) tol_rec->threshold = tol_threshold;  // (the last one a turn computed)
                    tol_stop = best_eval < tol_threshold;
                }
                if (tid == 0) {
                    const TreeEntry e = use_df ? heap[t.heap_cap - stack_n] : tree_pop(heap, heap_n);
                    sm.key = e.key;
                    sm.slot = e.slot;
                }
            } else {
                if (heap_n == 0) break;
                if constexpr (TOL) {  // the loop condition's toleranceFlag, then :73-87 -- before the pop; strict, false for NaN
                    if (tol_stop) { tol_broke = true; break; }
                    if (tid == 0) tol_rec->threshold = tol_threshold;  // (the last one a turn computed)
                    tol_stop = best_eval < tol_threshold;
                }
                if (tid == 0) {
                    const TreeEntry e = tree_pop(heap, heap_n);
                    sm.key = e.key;
                    sm.slot = e.slot;
                }
            }
            __syncthreads();
            const double key = sm.key;
            cur_slot = sm.slot;
            if constexpr (ENH) {
                if (use_df) stack_n -= 1; else heap_n -= 1;
            } else {
                heap_n -= 1;
            }
            __syncthreads();  // (sm.key / sm.slot may be written again)
            if (key > best_eval) { release(cur_slot); continue; }  // :89-92
        }
        if (iterations >= t.max_nodes) { terr = TREE_ERR_NODES; break; }
        if constexpr (INC) {  // :342: parentEval before applyIncrementalCuts, which may bring a checkpoint's evaluation
            parent_eval = evaluation;
            cur_ck = (!root && cur_slot >= 0) ? reinterpret_cast<const int32_t*>(pool + cur_slot * slot_bytes)[1] : (int)TREE_CK_NO_CUT;
        }
        if (INC && cur_ck >= 0) {  // :249-253: the parent's checkpoint and the ONE new cut, the list's last
            const TreeCkptHead ch = checkpoint_restore(cur_ck);
            __syncthreads();
            evaluation = ch.evaluation;
            feasible = ch.feasible;
            H = ch.height;
            if (H + 1 > RC) { terr = TREE_ERR_INC_ROWS; break; }
            H = add_cuts_at(cur_slot, H, *reinterpret_cast<const int32_t*>(pool + cur_slot * slot_bytes) - 1);
            __syncthreads();
            inc_nodes += 1;
        } else if (!root) {  // applyCuts: restore + addCutConstraints (:33-37)
            restore();
            __syncthreads();
            H = add_cuts(cur_slot);
            __syncthreads();
            if constexpr (MIR)
                if (H < 0) { H = Hs; terr = TREE_ERR_MIR_ROWS; break; }
        }
        root = false;
        if constexpr (ENH && !INC) parent_eval = evaluation;  // tableau.evaluation as the PREVIOUS node left it (:287)
        iters_left = m.iters_cap;
        o = pk_simplex<THREADS, OPT>(A, pcol, H, W, S, vibr, vibc, rbv, cbv, unr, precision, check_cycles, m, ghist, gtrace, sm.ps, iters_left, trace_n, oo, n_opt);
        __syncthreads();
        if (o.outcome >= 5) { serr = o.outcome == 5 ? (int)ERR_ITER_LIMIT : (int)ERR_HIST_FULL; break; }
        iterations += 1;
        if constexpr (INC) rows_hw = max(rows_hw, H);
        feasible = (o.outcome == 3 || o.outcome == 4) ? 0 : 1;
        unb_var = o.outcome == 2 ? vibc[o.unbounded_col] : -1;
        if (o.outcome == 1)  // setEvaluation (tableau.ts:420-430); a node that reaches no optimum keeps the previous node's
            evaluation = __ddiv_rn(tree_round(__dmul_rn(__dadd_rn(2.220446049250313e-16, A[0]), t.rcoef)), t.rcoef);
        else if (o.outcome == 2)
            evaluation = -INFINITY;
        if constexpr (TOL)  // setEvaluation while simplexIters === 0 (tableau.ts:420-430): the LP's first optimum is bestPossibleEval
            if (o.outcome == 1 && bp_open) {
                if (tid == 0) tol_rec->best_possible = evaluation;
                tol_threshold = __dmul_rn(evaluation, tol_factor);
                bp_open = false;
            }
        if constexpr (MIR) {
            mir_simplexes += 1;
            mir_tallest = max(mir_tallest, H);
            if (n_int > 0 && !mir_loop()) break;
        }
        if (n_int == 0) break;  // no integer variables: a plain simplex() (tableau.ts:250-258)
        if constexpr (ENH) {  // enhanced-branch-and-cut.ts:292-427; every path ends this iteration
            if (!feasible || evaluation > best_eval) { release(cur_slot); continue; }  // :292-299
            // :301-314: the pseudocost of the node's LAST cut, from the evaluation the previous node left (a node off the stack or the heap
            // has at least one cut; NaN !== 0).  (INC) :358-367: of the node's NEW cut, which the children of a depth-first node have
            if ((INC ? cur_ck != TREE_CK_NO_CUT : cur_slot >= 0) && parent_eval != 0.0) {
                if (tid == 0) {
                    const char* sp = pool + cur_slot * slot_bytes;
                    const int n = *reinterpret_cast<const int32_t*>(sp);
                    const TreeCut c = reinterpret_cast<const TreeCut*>(sp + 16)[n - 1];
                    TreePseudo* d = pseudo + (c.type >> 1);
                    const double normalized = __ddiv_rn(fabs(__dsub_rn(evaluation, parent_eval)), 0.5);  // (fraction = 0.5 either way, :307)
                    if ((c.type & 1) == 0) { d->up_sum = __dadd_rn(d->up_sum, normalized); d->up_count += 1; }
                    else { d->down_sum = __dadd_rn(d->down_sum, normalized); d->down_count += 1; }
                }
                pseudo_updates += 1;
            }
            if (evaluation == best_eval) { release(cur_slot); continue; }  // :316-336 without optional objectives
            // isIntegral (mip-utils.ts:43-61), as the default build's scan decides it
            int nonint = 0;
            for (int k = tid; k < n_int; k += THREADS) {
                const int r = rbv[ivars[k]];
                if (r > 0) {
                    const double v = A[r * S];
                    nonint |= fabs(v - tree_round(v)) > precision ? 1 : 0;  // (NaN: false)
                }
            }
            nonint = __syncthreads_or(nonint);  // (thread 0's pseudocost update is behind this barrier for every lane)
            if (!nonint) {  // :338-376
                found = 1;
                solutions += 1;
                if (iterations == 1) { done = true; break; }
                release(best_slot);
                best_slot = cur_slot;
                have_best = 1;
                best_eval = evaluation;
                if (node_sel == ENH_HYBRID && use_df) {  // :366-376: the stack's entries, from the top, into the heap, each with a fresh seq
                    if (tid == 0) {
                        int hn = heap_n, sq = seq;
                        for (int j = stack_n; j > 0; j--) {  // (heap[hn] is at or below the entry just read: stack and heap fit heap_cap together)
                            TreeEntry e = heap[t.heap_cap - j];
                            e.seq = sq++;
                            tree_push(heap, hn, e);
                            hn += 1;
                        }
                    }
                    heap_n += stack_n;
                    seq += stack_n;
                    moved += stack_n;
                    stack_n = 0;
                    use_df = false;
                }
                continue;
            }
            if (iterations == 1) {  // :378-380, before the selection
                save();
                __syncthreads();
            }
            // selectBranchingVariable (:112-196).  A candidate is an integer variable, in model order, with a row and a fraction above
            // precision (so a finite one); every rule is a first-wins maximum over the candidates, reduced across the lanes.
            auto fraction_of = [&](int k) -> double {  // -1: no candidate
                const int r = rbv[ivars[k]];
                if (r == -1) return -1.0;
                const double v = A[r * S];
                const double f = fabs(v - tree_round(v));
                return f > precision ? f : -1.0;
            };
            auto js_max = [](double x, double y) -> double { return x != x ? x : (x > y ? x : y); };  // Math.max(x, y) for a number y: NaN stays NaN
            auto score_of = [&](int k, double f) -> double {  // getScore (:98-110)
                const TreePseudo d = pseudo[k];
                const double up = d.up_count > 0 ? __ddiv_rn(d.up_sum, (double)d.up_count) : 1.0;
                const double down = d.down_count > 0 ? __ddiv_rn(d.down_sum, (double)d.down_count) : 1.0;
                return __dmul_rn(js_max(__dmul_rn(up, __dsub_rn(1.0, f)), 1e-6), js_max(__dmul_rn(down, f), 1e-6));
            };
            Cand b; b.v = -2.0; b.i = 0; b.b = 0;
            if (!INC && branching == ENH_STRONG) {
                // :161-193: the five most fractional -- a stable descending sort keeps model order among equals, so five first-wins maxima,
                // each over what the earlier ones left -- then the first strictly greatest score among them, from -Infinity on
                int top[ENH_STRONG_CANDIDATES];
#pragma unroll
                for (int j = 0; j < ENH_STRONG_CANDIDATES; j++) top[j] = -1;
#pragma unroll
                for (int j = 0; j < ENH_STRONG_CANDIDATES; j++) {
                    Cand x; x.v = -2.0; x.i = 0; x.b = 0;
                    for (int k = tid; k < n_int; k += THREADS) {
                        bool taken = false;
#pragma unroll
                        for (int q = 0; q < ENH_STRONG_CANDIDATES; q++) taken |= top[q] == k;
                        const double f = taken ? -1.0 : fraction_of(k);
                        if (f >= 0.0 && f > x.v) { x.v = f; x.i = k + 1; }
                    }
                    x = pk_reduce<THREADS>(x, MaxFirst(), sm.ps.g);
                    top[j] = x.i - 1;  // (-1: the candidates have run out)
                }
                double best_score = -INFINITY;
                b.i = top[0] + 1;
#pragma unroll
                for (int j = 0; j < ENH_STRONG_CANDIDATES; j++) {
                    if (top[j] < 0) continue;
                    const double f = fraction_of(top[j]);
                    const TreePseudo d = pseudo[top[j]];
                    const bool by_pseudo = d.up_count >= 2 && d.down_count >= 2;
                    scored += by_pseudo ? 1 : 0;
                    const double score = by_pseudo ? score_of(top[j], f) : __dmul_rn(f, __dsub_rn(1.0, f));
                    if (score > best_score) { best_score = score; b.i = top[j] + 1; }
                }
            } else {
                // most-fractional (:139-143): the first strictly largest fraction.  pseudocost (:145-159): the first strictly largest
                // score from -Infinity on, candidate 0 when none compares greater -- a score is positive or NaN, and NaN ranks as -1
                for (int k = tid; k < n_int; k += THREADS) {
                    const double f = fraction_of(k);
                    if (f < 0.0) continue;
                    double key = f;
                    if (branching == ENH_PSEUDOCOST) {
                        const double score = score_of(k, f);
                        key = score == score ? score : -1.0;
                    }
                    if (key > b.v) { b.v = key; b.i = k + 1; }
                }
                b = pk_reduce<THREADS>(b, MaxFirst(), sm.ps.g);
            }
            if (b.i == 0) { dropped += 1; release(cur_slot); continue; }  // :384: no candidate -- the node is dropped
            if constexpr (INC) {  // :440-445, :476-488: a checkpoint for both children while the walk is depth-first and the budget lasts
                child_ck = use_df ? TREE_CK_NONE : TREE_CK_NO_CUT;
                if (use_df && ck_count < max_ck) {
                    checkpoint_save(ck_count, H, evaluation, feasible);  // (read again behind the barriers below and the next pop's)
                    child_ck = ck_count;
                    ck_count += 1;
                    ck_rows_hw = max(ck_rows_hw, H);
                }
            }
            if (tid == 0) {  // :386-426: the two children's cut lists, then the stack (low first, so that high is popped first) or the heap (high first)
                const int pos = b.i - 1, var = ivars[pos];
                const double value = A[rbv[var] * S];
                const int src_n = cur_slot < 0 ? 0 : *reinterpret_cast<const int32_t*>(pool + cur_slot * slot_bytes);
                const TreeCut* src = reinterpret_cast<const TreeCut*>(pool + (cur_slot < 0 ? 0 : cur_slot) * slot_bytes + 16);
                int code = TREE_OK, fn = free_n, fr = fresh_n, hn = heap_n, sn = stack_n, sq = seq, len[2] = {0, 0};
                for (int ord = 0; ord < 2 && code == TREE_OK; ord++) {
                    const int child = use_df ? 1 - ord : ord;  // 0: high ("min" cut, ceil), 1: low ("max" cut, floor)
                    const int slot = fn > 0 ? free_list[--fn] : fr++;
                    char* dp = pool + slot * slot_bytes;
                    TreeCut* dst = reinterpret_cast<TreeCut*>(dp + 16);
                    int n = 0;
                    for (int k = 0; k <= src_n && code == TREE_OK; k++) {
                        TreeCut c;
                        if (k < src_n) {
                            c = src[k];
                            if (c.var == var && ((c.type & 1) == 0) != (child == 1)) continue;  // :393-405
                        } else {
                            c.value = child == 0 ? ceil(value) : floor(value);
                            c.var = var;
                            c.type = (pos << 1) | child;
                        }
                        if (n >= t.cut_rows) { code = TREE_ERR_CUTS; break; }
                        dst[n++] = c;
                    }
                    if (code != TREE_OK) break;
                    *reinterpret_cast<int32_t*>(dp) = n;
                    if constexpr (INC) reinterpret_cast<int32_t*>(dp)[1] = child_ck;
                    len[child] = n;
                    if (sn + hn >= t.heap_cap) { code = TREE_ERR_HEAP; break; }  // (stack and heap share the array)
                    TreeEntry e; e.key = evaluation; e.slot = slot;
                    if (use_df) { e.seq = 0; heap[t.heap_cap - 1 - sn] = e; sn += 1; }
                    else { e.seq = sq++; tree_push(heap, hn, e); hn += 1; }
                }
                sm.code = code;
                sm.n_high = len[0];
                sm.n_low = len[1];
            }
            __syncthreads();
            terr = sm.code;
            cuts_hw = max(cuts_hw, max(sm.n_high, sm.n_low));
            __syncthreads();
            if (terr != TREE_OK) break;
            for (int child = 0; child < 2; child++) {
                if (free_n > 0) free_n -= 1; else fresh_n += 1;
            }
            if (use_df) { stack_n += 2; stack_hw = max(stack_hw, stack_n); }
            else { heap_n += 2; seq += 2; }
            pushes += 2;
            heap_hw = max(heap_hw, stack_n + heap_n);
            release(cur_slot);
            continue;
        }
        if constexpr (OPT) {
            if (!feasible || evaluation > best_eval) { release(cur_slot); continue; }  // :99-105
            if (evaluation == best_eval) {  // :107-127: the tie is broken on the optional objectives, in priority order (NaN decides nothing)
                if (tid == 0) {
                    int worse = 1;
                    for (int k = 0; k < n_opt; k++) {
                        const double mine = oo[k * S], best = best_opt[k];
                        if (mine > best) break;
                        if (mine < best) { worse = 0; break; }
                    }
                    sm.code = worse;
                }
                __syncthreads();
                const int worse = sm.code;
                __syncthreads();  // (sm.code may be written again)
                if (worse) { release(cur_slot); continue; }
            }
        } else {
            if (!feasible || evaluation > best_eval || evaluation == best_eval) { release(cur_slot); continue; }  // :99-127
        }
        // isIntegral + getMostFractionalVar (mip-utils.ts:43-61, 100-126) over the integer variables in model order
        Cand b; b.v = -1.0; b.i = 0; b.b = 0;
        int nonint = 0;
        for (int k = tid; k < n_int; k += THREADS) {
            const int r = rbv[ivars[k]];
            if (r > 0) {
                const double v = A[r * S];
                const double frac = fabs(v - tree_round(v));
                nonint |= frac > precision ? 1 : 0;           // (NaN: false)
                const double fkey = frac == frac ? frac : -1.0;  // `fraction > biggest` is false for NaN
                if (fkey > b.v) { b.v = fkey; b.i = k + 1; }
            }
        }
        b = pk_reduce<THREADS>(b, MaxFirst(), sm.ps.g);
        nonint = __syncthreads_or(nonint);
        if (!nonint) {
            found = 1;
            if (iterations == 1) { done = true; break; }  // :132-135: no save, no final re-evaluation
            release(best_slot);
            best_slot = cur_slot;  // (the list changes owner: not released)
            have_best = 1;
            best_eval = evaluation;
            if constexpr (OPT)  // :138-141 (the next restore waits behind the barrier of the pop)
                if (tid == 0)
                    for (int k = 0; k < n_opt; k++) best_opt[k] = oo[k * S];
            continue;
        }
        if (!(b.v > 0.0)) { terr = TREE_ERR_BRANCH; break; }
        if (iterations == 1) {  // :155-157 ((MIR) with the root's MIR rows)
            if constexpr (MIR) Hs = H;
            save();
            __syncthreads();
        }
        if (tid == 0) {  // :160-191: the two children's cut lists and their pushes, the high child first
            const int var = ivars[b.i - 1];
            const double value = A[rbv[var] * S];
            const int src_n = cur_slot < 0 ? 0 : *reinterpret_cast<const int32_t*>(pool + cur_slot * slot_bytes);
            const TreeCut* src = reinterpret_cast<const TreeCut*>(pool + (cur_slot < 0 ? 0 : cur_slot) * slot_bytes + 16);
            int code = TREE_OK, fn = free_n, fr = fresh_n, hn = heap_n, sq = seq, len[2] = {0, 0};
            for (int child = 0; child < 2 && code == TREE_OK; child++) {  // 0: high ("min" cut, ceil), 1: low ("max" cut, floor)
                const int slot = fn > 0 ? free_list[--fn] : fr++;
                char* dp = pool + slot * slot_bytes;
                TreeCut* dst = reinterpret_cast<TreeCut*>(dp + 16);
                int n = 0;
                for (int k = 0; k <= src_n && code == TREE_OK; k++) {
                    TreeCut c;
                    if (k < src_n) {
                        c = src[k];
                        // a cut on the branching variable survives only in the child of its own type (:166-179)
                        if (c.var == var && (c.type == 0) != (child == 1)) continue;
                    } else {
                        c.value = child == 0 ? ceil(value) : floor(value);
                        c.var = var;
                        c.type = child;
                    }
                    if (n >= t.cut_rows) { code = TREE_ERR_CUTS; break; }
                    dst[n++] = c;
                }
                if (code != TREE_OK) break;
                *reinterpret_cast<int32_t*>(dp) = n;
                len[child] = n;
                if (hn >= t.heap_cap) { code = TREE_ERR_HEAP; break; }
                TreeEntry e; e.key = evaluation; e.seq = sq++; e.slot = slot;
                tree_push(heap, hn, e);
                hn += 1;
            }
            sm.code = code;
            sm.n_high = len[0];
            sm.n_low = len[1];
        }
        __syncthreads();
        terr = sm.code;
        cuts_hw = max(cuts_hw, max(sm.n_high, sm.n_low));
        __syncthreads();
        if (terr != TREE_OK) break;
        // what thread 0 did to the free stack, the heap and the counters, in every thread
        for (int child = 0; child < 2; child++) {
            if (free_n > 0) free_n -= 1; else fresh_n += 1;
        }
        heap_n += 2;
        seq += 2;
        pushes += 2;
        heap_hw = max(heap_hw, heap_n);
        release(cur_slot);
    }
    // :195-197: the incumbent's cut list is evaluated once more -- the final tableau, and its pivots join the trace
    if (terr == TREE_OK && serr == ERR_NONE && !done && have_best) {
        restore();
        __syncthreads();
        H = add_cuts(best_slot);
        __syncthreads();
        if constexpr (MIR)
            if (H < 0) { H = Hs; terr = TREE_ERR_MIR_ROWS; }
        if (!MIR || terr == TREE_OK) {
            iters_left = m.iters_cap;
            o = pk_simplex<THREADS, OPT>(A, pcol, H, W, S, vibr, vibc, rbv, cbv, unr, precision, check_cycles, m, ghist, gtrace, sm.ps, iters_left, trace_n, oo, n_opt);
            __syncthreads();
            if (o.outcome >= 5) serr = o.outcome == 5 ? (int)ERR_ITER_LIMIT : (int)ERR_HIST_FULL;
            if constexpr (INC) rows_hw = max(rows_hw, H);
            feasible = (o.outcome == 3 || o.outcome == 4) ? 0 : 1;
            unb_var = o.outcome == 2 ? vibc[o.unbounded_col] : -1;
            if (o.outcome == 1)
                evaluation = __ddiv_rn(tree_round(__dmul_rn(__dadd_rn(2.220446049250313e-16, A[0]), t.rcoef)), t.rcoef);
            else if (o.outcome == 2)
                evaluation = -INFINITY;
            if constexpr (TOL)  // setEvaluation while simplexIters === 0 (tableau.ts:420-430): the LP's first optimum is bestPossibleEval
                if (o.outcome == 1 && bp_open) {
                    if (tid == 0) tol_rec->best_possible = evaluation;
                    tol_threshold = __dmul_rn(evaluation, tol_factor);
                    bp_open = false;
                }
            if constexpr (MIR) {
                mir_simplexes += 1;
                mir_tallest = max(mir_tallest, H);
                if (serr == ERR_NONE) (void)mir_loop();
            }
        }
    }
    // ---- epilogue: the state, the RHS column and the row map of whatever LDS holds now ----------------------------------------------------
    __syncthreads();
    const bool ok = terr == TREE_OK && serr == ERR_NONE && iterations > 0;
    if (ok) {
        for (int r = tid; r < H; r += THREADS) {
            out_rhs[m.out_off + r] = A[r * S];
            out_rows[m.out_off + r] = vibr[r];
        }
        if constexpr (OPT) {  // the rows of whatever LDS holds: the incumbent's after the final re-evaluation
            double* out_opt = many_global(m.opt_out);
            for (int q = tid; q < n_opt * W; q += THREADS) {
                const int k = q / W;
                out_opt[q] = oo[k * S + (q - k * W)];
            }
        }
    }
    if (tid == 0) {
        st->H = H;
        st->last_element_index = W + H - 2;
        st->status = ST_DONE;
        st->do_pivot = 0;
        st->err = serr;
        st->trace_n = trace_n;
        st->iters_left = iters_left;
        if (ok) {
            st->phase = o.phase;
            st->it1 = o.it1;
            st->it2 = o.it2;
            st->hist_n = o.hist_n;
            st->entered_phase2 = o.entered2;
            st->feasible = feasible;
            st->bounded = o.outcome == 2 ? 0 : 1;
            st->optimal = o.outcome == 1 ? 1 : 0;
            st->unbounded_var = unb_var;
            st->cycle_phase = o.outcome == 3 ? o.phase : 0;
            st->obj_cell = A[0];
        }
        TreeRec rec;
        rec.evaluation = evaluation;
        rec.iterations = n_int > 0 ? iterations : 0;
        rec.is_integral = found;
        rec.final_height = H;
        rec.nodes_pushed = n_int > 0 ? pushes : 0;
        rec.heap_high_water = n_int > 0 ? heap_hw : 0;
        rec.cuts_high_water = cuts_hw;
        rec.err = terr;
        rec.pad = 0;
        out_tree[idx] = rec;
        if constexpr (MIR) {
            TreeMirRec mr;
            mr.rounds = mir_rounds; mr.rows_added = mir_rows; mr.simplexes = mir_simplexes;
            mr.root_rows = Hs - H0; mr.rows_high_water = mir_tallest - H0;
            mr.pad[0] = mr.pad[1] = mr.pad[2] = 0;
            *many_global(t.mir_out) = mr;
        }
        if constexpr (ENH) {
            TreeEnhRec er;
            er.solutions_found = solutions; er.stack_high_water = n_int > 0 ? stack_hw : 0; er.moved_to_heap = moved;
            er.pseudo_updates = pseudo_updates; er.scored_by_pseudocost = scored; er.dropped_nodes = dropped;
            er.pad[0] = er.pad[1] = 0;
            *many_global(t.enh_out) = er;
        }
        if constexpr (TOL)
            if (tol_broke) {  // (nothing has touched heap or stack since the loop ended)
                tol_rec->stopped = 1;
                tol_rec->left = heap_n + stack_n;
            }
        if constexpr (INC) {
            TreeIncRec ir;
            ir.checkpoints_used = ck_count; ir.incremental_nodes = inc_nodes; ir.rows_high_water = rows_hw - H0;
            ir.checkpoint_rows_high_water = ck_rows_hw - H0;
            ir.pad[0] = ir.pad[1] = ir.pad[2] = ir.pad[3] = 0;
            *reinterpret_cast<TreeIncRec*>(many_global(t.enh_out) + 1) = ir;
        }
    }
    __syncthreads();
    if (tid < (int)(sizeof(DevState) / 8))
        reinterpret_cast<long long*>(out_states + idx)[tid] = reinterpret_cast<const long long*>(st)[tid];
}

// one build of k_tree_packed, as pk_launch (MIR, ENH and INC come without OPT; an INC build is an ENH build)
template <int T, int BUILD, bool TOL = false, bool BIG = false>
static bool tree_launch(int threads, unsigned grid, size_t lds, const PackLaunch& a, hipStream_t s, hipError_t* err) {
    if constexpr (!pack_build_here(BUILD) || !pack_tol_here(TOL) || !pack_big_here(BIG)) {
        return false;
    } else {
        if (threads != T || a.build != BUILD || (a.tol != 0) != TOL || (lds > PACK_SMALL_LDS) != BIG) return false;
        if constexpr (BIG) {
            static unsigned long long ready = 0;
            *err = pack_big_prepare(k_tree_packed<T, BUILD == PACK_OPT, BUILD == PACK_MIR, BUILD == PACK_ENH || BUILD == PACK_INC, BUILD == PACK_INC, TOL>, lds, &ready);
            if (*err != hipSuccess) return true;
        }
        hipLaunchKernelGGL((k_tree_packed<T, BUILD == PACK_OPT, BUILD == PACK_MIR, BUILD == PACK_ENH || BUILD == PACK_INC, BUILD == PACK_INC, TOL>), dim3(grid), dim3(T), lds, s,
                           a.lps, static_cast<const TreeLp*>(a.trees), a.order, a.cc, a.cc_all, static_cast<DevState*>(a.states), a.rhs, a.rows,
                           static_cast<TreeRec*>(a.tree_out));
        return true;
    }
}
// THE table of the pack kernels' builds: launches the one (a.tree, threads, a.build) names; returns the hipError_t of the launch, or -1: no such
// build in this unit.  The error is PEEKED at, not taken: the caller's hipGetLastError still sees it and reports it.
// (the rows' order is the order the compiler instantiates the kernels in, and their code can depend on it: tools/asm_digest.py)
static int pack_dispatch(int threads, unsigned grid, size_t lds, const void* bytes, void* stream) {
    const PackLaunch& a = *static_cast<const PackLaunch*>(bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool hit;
    hipError_t err = hipSuccess;  // (a large build: what forbade its launch)
    constexpr int B = JSLP_PACK_BIG_THREADS;
    if (!a.tree)
        hit = pk_launch<64, PACK_PLAIN>(threads, grid, lds, a, s, &err) || pk_launch<256, PACK_PLAIN>(threads, grid, lds, a, s, &err) ||
              pk_launch<64, PACK_OPT>(threads, grid, lds, a, s, &err) || pk_launch<256, PACK_OPT>(threads, grid, lds, a, s, &err) ||
              // (the large builds behind every other, as the TOL builds below)
              pk_launch<B, PACK_PLAIN, true>(threads, grid, lds, a, s, &err) || pk_launch<B, PACK_OPT, true>(threads, grid, lds, a, s, &err);
    else
        hit = tree_launch<64, PACK_PLAIN>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_PLAIN>(threads, grid, lds, a, s, &err) ||
              tree_launch<64, PACK_OPT>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_OPT>(threads, grid, lds, a, s, &err) ||
              tree_launch<64, PACK_MIR>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_MIR>(threads, grid, lds, a, s, &err) ||
              tree_launch<64, PACK_ENH>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_ENH>(threads, grid, lds, a, s, &err) ||
              tree_launch<64, PACK_INC>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_INC>(threads, grid, lds, a, s, &err) ||
              // (the TOL builds behind every other, so that those are instantiated in the order they were)
              tree_launch<64, PACK_PLAIN, true>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_PLAIN, true>(threads, grid, lds, a, s, &err) ||
              tree_launch<64, PACK_OPT, true>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_OPT, true>(threads, grid, lds, a, s, &err) ||
              tree_launch<64, PACK_MIR, true>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_MIR, true>(threads, grid, lds, a, s, &err) ||
              tree_launch<64, PACK_ENH, true>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_ENH, true>(threads, grid, lds, a, s, &err) ||
              tree_launch<64, PACK_INC, true>(threads, grid, lds, a, s, &err) || tree_launch<256, PACK_INC, true>(threads, grid, lds, a, s, &err) ||
              // (the large builds, include/jslpb_big_lds.h: the default service, plain and OPT)
              tree_launch<B, PACK_PLAIN, false, true>(threads, grid, lds, a, s, &err) || tree_launch<B, PACK_OPT, false, true>(threads, grid, lds, a, s, &err);
    if (hit && err != hipSuccess) return (int)err;
    return hit ? (int)hipPeekAtLastError() : -1;
}
#endif  // JSLP_PACKED_KERNELS
