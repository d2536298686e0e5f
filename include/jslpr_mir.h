/* jslpr_mir.h -- a branch-and-bound node WITH its MIR-cut loop in one engine call.
 *
 * Extension of include/jslp_engine.h, exported by the HIP library only (like jslpx_branch.h / jslpm_many.h / jslpf_f32.h).
 *
 * With options.useMIRCuts the reference's LP relaxation of a node is restore + addCutConstraints + simplex followed by
 *     before = computeFractionalVolume(true); applyMIRCuts(); simplex(); after = computeFractionalVolume(true);
 * repeated until after >= 0.9 * before (branch-and-cut.ts:33-52; the incremental service: at most 3 rounds, feasible tableaus
 * only, incremental-branch-and-cut.ts:228-243).  jslpr_engine_relax_mir runs all of it per node inside the call -- where
 * jslp_engine_relax_batch evaluates a node in one launch of an LDS node kernel, in that one launch.
 */
#ifndef JSLPR_MIR_H
#define JSLPR_MIR_H

#include "jslp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSLPR_MAX_ROUNDS 64 /* rounds per node; max_rounds may not exceed it, and an unbounded loop that gets there fails */

typedef struct jslpr_mir_outcome { /* 32 bytes, one per node */
    int32_t rounds;        /* MIR rounds run (0: the loop did not start) */
    int32_t rows_added;    /* rows appended by all rounds */
    int32_t optimal_count; /* how many of the node's 1 + rounds simplex() calls ended optimal (host: simplexIters) */
    int32_t pivots;        /* pivots of all of them */
    double volume_before;  /* computeFractionalVolume(true) before / after the LAST round; 0 when rounds == 0 */
    double volume_after;
} jslpr_mir_outcome;

int32_t jslpr_mir_outcome_bytes(void);

/* Per node i: restore (checkpoint < 0: the saved root, or the live tableau when nothing was saved) or checkpoint_restore
 * (checkpoint >= 0; n_nodes must be 1), addCutConstraints of the cuts [cut_offsets[i], cut_offsets[i + 1]), simplex; then, unless
 * need_feasible is set and that simplex left feasible == 0, the MIR loop above for at most max_rounds rounds (max_rounds < 0: until
 * the volume rule stops it; JSLPR_MAX_ROUNDS rounds without a stop fail the call with JSLP_ERR_CAPACITY); then the read-back of
 * jslp_engine_relax_batch (rhs / var_index_by_row: out_stride >= row capacity entries per node, or NULL).
 *
 * out[i], rhs and var_index_by_row are what the LAST call of the sequence jslp_engine_relax(cuts_i), jslp_engine_mir_round, ...
 * returns on an engine holding the same root, with out[i].evaluation folded over the node's simplexes as the host folds
 * tableau.evaluation: an optimal one sets it, an unbounded one sets -Infinity, any other keeps the previous value -- which starts,
 * for every node, at the evaluation the call began with (the checkpoint's for checkpoint >= 0).  mir[i] says what the loop did.
 * The caveats of jslp_engine_relax_batch carry over: no [start, length] detail of a cycle when a batch runs in groups, the live
 * tableau unspecified after several nodes.  After a ONE-node call the live tableau holds that node with its MIR rows and the pivot
 * trace all its pivots.
 *
 * What differs from the sequence, and is not reported: (1) out[i].unbounded_var_index is the last simplex's; the variable of an EARLIER
 * unbounded simplex of the node (whose -Infinity the folded evaluation does carry) has no field in the 32-byte outcome.  (2) The host
 * half of jslp_work_counters (relaxations, simplex_calls, pivots, height_sum, cut_rows) advances as the sequence's does; restored_rows
 * does not: the sequence's jslp_engine_simplex leaves slot 0 out of sync with the saved root, so its next node restores every row,
 * while the one-launch shapes keep the slot in sync and restore the rows the node wrote.
 *
 * One launch or the sequence is decided for the WHOLE call: the MIR build of an LDS node kernel runs it when every group of the call
 * would be one launch of such a kernel (a saved root, the tableau's selection state fits LDS, no timing, the default JSLP_NODE_QUEUE /
 * JSLP_WG_BATCH_THREADS, no trailing group of one node); slots not yet in sync with the saved root are restored first.  Otherwise every
 * node of the call runs the engine's existing launches one after the other -- same results, several launches and a synchronisation
 * per round; JSLP_DEBUG_LAUNCH=1 shows which it was.
 *
 * JSLP_ERR_STATE before jslp_engine_set_integer_variables, JSLP_ERR_UNSUPPORTED with optional objectives, JSLP_ERR_ARG for
 * checkpoint >= 0 with n_nodes != 1 or max_rounds > JSLPR_MAX_ROUNDS, JSLP_ERR_CAPACITY when a node's rows exceed the row
 * capacity (the engine is usable again after jslp_engine_restore). */
int jslpr_engine_relax_mir(jslp_engine* e, int32_t checkpoint, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                           const int32_t* var_index, const double* value, int check_cycles, int32_t max_rounds,
                           int32_t need_feasible, jslp_simplex_result* out, jslpr_mir_outcome* mir, double* rhs,
                           int32_t* var_index_by_row, int32_t out_stride);

#ifdef __cplusplus
}
#endif
#endif
