/*
 * jslpt_tree.h -- small MILPs in a pack: the branch-and-bound tree of every LP walked inside ONE launch.  An extension of
 * jslpp_packed.h, exported by the HIP library only.
 *
 * A pack made by jslpt_pack_create is a jslpp_pack whose LPs have a ROW CAPACITY (height + cut_rows) and a heap.  One workgroup per LP
 * holds the tableau at that capacity in LDS and runs Tableau.solve() of a model with integer variables under the DEFAULT service
 * (branch-and-cut.ts:54-199 with applyCuts = restore + addCutConstraints + simplex, :33-37): the root, the save, the heap of
 * min-heap.ts, isIntegral / getMostFractionalVar (mip-utils.ts), the two children per branch, the final re-evaluation of the
 * incumbent.  The kernel (k_tree_packed, jslpsolver_amd/csrc/jslp_tree.hip.h) returns when the tree is done; the host is not in the loop.
 *
 * Per LP the call leaves what the reference leaves, bit for bit: the result of the last relaxation evaluated (the incumbent's when
 * there is one, the last node's otherwise), the final RHS column and row map, the iteration count, and the pivot trace of EVERY node
 * in order, the final re-evaluation included.  A node that reaches no optimum keeps the evaluation of the node before it.
 *
 * Out of scope, by design (such models go through a jslp_engine): the incremental service, timeout, keep_solutions (options.tolerance
 * comes through jslpg_tree_tolerance.h), and
 * an LP whose LDS image at its row capacity exceeds JSLPP_LDS_LIMIT.  Optional objectives come through jslps_soft.h, and MIR cuts
 * (options.useMIRCuts: every node's MIR loop run in the kernel) through jslpc_tree_mir.h -- the two together stay out of scope.  The
 * enhanced service (options.nodeSelection / options.branching) comes through jslpe_tree_enhanced.h, without MIR cuts and without
 * optional objectives.
 *
 * jslpp_pack_set, jslpp_pack_host_matrix, jslpp_pack_upload, jslpp_pack_simplex, jslpp_pack_destroy, jslpp_pack_size and
 * jslpp_pack_pivot_trace work on such a pack as on any other.  The arena keeps the SAVED ROOT, not the final tableau: after
 * jslpt_pack_branch_and_cut, jslpp_pack_download, jslpp_pack_simplex and a second jslpt_pack_branch_and_cut need a new upload
 * (JSLP_ERR_STATE).
 *
 * Errors as jslpp_pack_simplex: argument and state errors before any work; per-LP failures in status[i] with out[i] and tree_out[i]
 * left as they were and every other LP solved; the call returns the first non-OK status and jslp_last_error() names the LP
 * ("LP <i>") and the capacity that was reached.
 */
#ifndef JSLPT_TREE_H
#define JSLPT_TREE_H

#include "jslpp_packed.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSLPT_MAX_NODES_DEFAULT 1000000 /* max_nodes = 0 */

typedef struct jslpt_tree_result {
    int32_t iterations;      /* nodes evaluated (branch-and-cut.ts `iterations`); 0 for an LP without integer variables      */
    int32_t is_integral;     /* an integral node was accepted (tableau.__isIntegral)                                          */
    int32_t final_height;    /* rows of the final tableau: height + the cuts of the node it holds                             */
    int32_t nodes_pushed;    /* heap pushes, the root's included                                                              */
    int32_t heap_high_water; /* most entries the heap held                                                                    */
    int32_t cuts_high_water; /* longest cut list pushed                                                                       */
} jslpt_tree_result;

/* jslpp_lds_bytes for an LP whose tableau and index maps are sized for row_capacity rows: equal to jslpp_lds_bytes(height, width)
 * at row_capacity == height, monotone in all three arguments, 0 when height < 2, width < 2 or row_capacity < height. */
int64_t jslpt_lds_bytes(int32_t height, int32_t width, int32_t row_capacity);

/*
 * jslpp_pack_create with, per LP, cut_rows[i] >= 0 further rows (row capacity height[i] + cut_rows[i]; the longest cut list a node
 * may carry) and a heap of heap_cap[i] >= 1 entries.  max_nodes > 0 caps the nodes evaluated per LP; 0 = JSLPT_MAX_NODES_DEFAULT.
 * max_pivots caps the pivots of ONE relaxation, as an engine's cap does.  An LP whose jslpt_lds_bytes exceeds JSLPP_LDS_LIMIT is
 * refused with JSLP_ERR_UNSUPPORTED naming the LP.
 */
int jslpt_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                      const int32_t* cut_rows, const int32_t* heap_cap, int32_t trace_cap, int32_t max_pivots, int32_t max_nodes);

/* LP i's integer variables: their indexes in model.integerVariables order (the order decides ties between equal fractions).
 * Before jslpp_pack_upload; n = 0 makes the LP a plain simplex().  An index outside the maps -> JSLP_ERR_ARG naming the LP. */
int jslpt_pack_set_integers(jslpp_pack* p, int32_t i, const int32_t* var_indexes, int32_t n);

/*
 * Tableau.solve() of every LP in at most one launch per kernel build, then one D2H copy.  check_cycles, status, device_ms as
 * jslpp_pack_simplex.  out[i]: the jslp_simplex_result of the last relaxation evaluated; tree_out[i] (may be NULL): the tree's
 * counters.  Per-LP JSLP_ERR_CAPACITY: the pivot cap or the history capacity of a relaxation, max_nodes, a full heap, a cut list
 * longer than cut_rows.  jslpp_pack_launches counts this call's launches.
 */
int jslpt_pack_branch_and_cut(jslpp_pack* p, const int32_t* check_cycles, jslp_simplex_result* out, jslpt_tree_result* tree_out,
                              int32_t* status, double* device_ms);

/* jslpp_pack_read_rhs after jslpt_pack_branch_and_cut: LP i's block [offsets[i], offsets[i + 1]) is sized by its row capacity;
 * the first final_height entries are valid. */
int jslpt_pack_read_rhs(jslpp_pack* p, const double** rhs, const int32_t** var_index_by_row, const int64_t** offsets);

#ifdef __cplusplus
}
#endif
#endif /* JSLPT_TREE_H */
