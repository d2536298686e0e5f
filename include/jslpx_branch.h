/*
 * jslpx_branch.h -- branch records: an extension of the C ABI in jslp_engine.h, exported by the HIP library only.
 *
 * Between two relaxations the branch-and-bound tree reads, per node, the flags, the evaluation, isIntegral() and the
 * {index, value} getMostFractionalVar() returns (src/tableau/mip-utils.ts:43-61, 100-126; branch-and-cut.ts:90-199).
 * The branch record is exactly that, computed on the device from the node's final RHS column: 32 bytes per node
 * whatever the number of integer variables, instead of the compact read-back's 128 + 12 x n_watched.
 *
 * The record is computed over the WATCHED variables (jslp_engine_set_watched_variables) in registration order -- the
 * tree registers model.integerVariables -- with the engine's precision, bit for bit as the reference computes it:
 *   - a variable counts only when it is basic (row in (0, height)), as `row !== -1` in the reference;
 *   - round(v) is Math.round (ties toward +Infinity): f = floor(v); (v - f >= 0.5) ? f + 1 : f;
 *     fraction = |v - round(v)|;
 *   - is_integral unless some counted variable has fraction > precision (strictly; a NaN fraction does not count);
 *   - the branch variable is the FIRST counted variable with the strictly largest fraction, and only if that
 *     fraction is > 0 (NaN is never chosen); otherwise branch_var_index = -1 and branch_var_value = 0.0.
 * A record is written for every node, feasible or not.
 *
 * Every entry point requires jslp_engine_set_watched_variables first and fails with JSLP_ERR_ARG otherwise.
 */
#ifndef JSLPX_BRANCH_H
#define JSLPX_BRANCH_H

#include "jslp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSLPX_BRANCH_FEASIBLE 1    /* flags bit 0 */
#define JSLPX_BRANCH_BOUNDED 2     /* flags bit 1 */
#define JSLPX_BRANCH_OPTIMAL 4     /* flags bit 2 */
#define JSLPX_BRANCH_INTEGRAL 8    /* flags bit 3: isIntegral() */

typedef struct jslpx_branch_record { /* 32 bytes, one per node */
    int32_t flags;               /* JSLPX_BRANCH_*                                                          */
    int32_t unbounded_var_index; /* as jslp_simplex_result                                                  */
    int32_t branch_var_index;    /* getMostFractionalVar().index; -1 = null                                 */
    int32_t height;              /* rows after the node's cuts                                              */
    double obj_cell;             /* raw matrix[0]: the host derives `evaluation` from it exactly as the
                                    jslp_simplex_result of the same node does                              */
    double branch_var_value;     /* getMostFractionalVar().value; 0.0 when the index is -1                  */
} jslpx_branch_record;

/* sizeof(jslpx_branch_record): 32 */
int32_t jslpx_branch_record_bytes(void);

/* jslp_engine_relax_batch with the branch record as the read-back: out[i] is node i's record (host memory) */
int jslpx_engine_relax_batch_branch(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                    const int32_t* var_index, const double* value, int check_cycles,
                                    jslpx_branch_record* out);
/* the same without the copy: *out points into the engine's pinned read-back buffer (n_nodes records), valid until the next
 * call on this engine */
int jslpx_engine_relax_batch_branch_pinned(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                           const int32_t* var_index, const double* value, int check_cycles,
                                           const jslpx_branch_record** out);
/* the records left in DEVICE memory of the engine's device (n_nodes x 32 bytes, 16-byte aligned): the exchange payload of
 * the multi-process path.  Nothing is copied to the caller; the engine still checks every node for errors itself. */
int jslpx_engine_relax_batch_branch_device(jslp_engine* e, int32_t n_nodes, const int32_t* cut_offsets, const int8_t* type,
                                           const int32_t* var_index, const double* value, int check_cycles,
                                           void* d_records);
/* n records in HOST memory -> jslp_simplex_result: flags, unbounded index, height and obj_cell as recorded; evaluation as
 * every other entry point derives it (optimal: round((EPS + obj_cell) * rc) / rc; unbounded: -Infinity; otherwise the
 * evaluation the engine's last batch call started from).  Pivot counts and cycle details are not in the record: 0. */
int jslpx_engine_results_from_branch_records(jslp_engine* e, const void* records, int32_t n, jslp_simplex_result* out);

#ifdef __cplusplus
}
#endif
#endif /* JSLPX_BRANCH_H */
