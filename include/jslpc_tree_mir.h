/*
 * jslpc_tree_mir.h -- small MILPs with options.useMIRCuts in a pack: every node's MIR-cut loop run inside the tree kernel.  An extension
 * of jslpt_tree.h, exported by the HIP library only.
 *
 * A pack made by jslpc_tree_pack_create is a pack of jslpt_tree.h some of whose LPs are MIR LPs.  A MIR LP runs in a MIR build of
 * k_tree_packed (jslpsolver_amd/csrc/jslp_tree.hip.h, jslp_tree_mir.hip.h): behind the simplex of every node -- the root, every later
 * node, the final re-evaluation of the incumbent -- its workgroup runs applyCuts' loop of branch-and-cut.ts:38-52 in LDS:
 * computeFractionalVolume(true) (mip-utils.ts:67-92), applyMIRCuts (cutting-strategies.ts:74-212: up to 10 rows per round), simplex again,
 * the volume again, until it shrinks by less than 10 %.  The root's MIR rows are appended before save(), so they are part of every later
 * node.  Per LP the call leaves what the reference leaves, bit for bit, as jslpt_tree.h says; the pivots of every simplex join the trace.
 *
 * A MIR LP's rows come out of ONE row capacity, height + row_extra: the root's MIR rows, a node's cut list and the node's MIR rows.  Its
 * cut lists still hold at most cut_rows cuts.  The kernel ends whatever the data: a round or a cut list whose rows do not fit the row
 * capacity, and JSLPR_MAX_ROUNDS (include/jslpr_mir.h) rounds of one node without a stop, end that LP with JSLP_ERR_CAPACITY in status[i]
 * -- out[i], tree_out[i] and the LP's MIR record left as they were, every other LP solved -- and jslp_last_error() names the LP and
 * `row_extra` or `mir rounds`.
 *
 * jslpt_pack_set_integers (a MIR LP's integer variables are also its variable.isInteger), jslpp_pack_set / upload / destroy / size /
 * launches, jslpt_pack_branch_and_cut, jslpt_pack_read_rhs and jslpp_pack_pivot_trace work on such a pack as on any jslpt pack.  In
 * jslpt_tree_result final_height includes MIR rows; cuts_high_water stays the longest cut list.  A call is at most one launch per kernel
 * build that has LPs: (64 | 256 threads) x (plain, MIR) here, routed by the tableau cells at the row capacity as before.  With
 * JSLP_DEBUG_LAUNCH=1 a MIR build prints "[jslp] launch k_tree_packed<T,mir 1> n N lds B".
 *
 * Out of scope: a MIR LP with optional objectives (as jslpr_mir.h refuses the pair), and what jslpt_tree.h leaves out.
 */
#ifndef JSLPC_TREE_MIR_H
#define JSLPC_TREE_MIR_H

#include "jslpt_tree.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jslpc_mir_result {
    int32_t rounds;          /* MIR rounds of all nodes (applyMIRCuts + simplex each)                                          */
    int32_t rows_added;      /* rows those rounds appended: the reference's mirCuts                                            */
    int32_t simplexes;       /* simplex() runs of the tree: one per node, one per round, the final re-evaluation's             */
    int32_t root_rows;       /* rows of the saved root above the LP's height (0 when the root was never saved)                 */
    int32_t rows_high_water; /* rows of the tallest tableau above the LP's height: what row_extra has to hold                  */
} jslpc_mir_result;

/* jslpt_lds_bytes for a MIR LP: the tree LP's image at row_capacity rows and variable.isInteger per variable index behind it.  Monotone
 * in all three arguments, 0 when height < 2, width < 2 or row_capacity < height. */
int64_t jslpc_tree_lds_bytes(int32_t height, int32_t width, int32_t row_capacity);

/*
 * jslpt_pack_create with, per LP, row_extra[i]: negative -> a plain tree LP exactly as jslpt_pack_create makes it (row capacity
 * height[i] + cut_rows[i]); row_extra[i] >= cut_rows[i] -> a MIR LP with row capacity height[i] + row_extra[i].
 * 0 <= row_extra[i] < cut_rows[i] is JSLP_ERR_ARG; a MIR LP whose jslpc_tree_lds_bytes (a plain one whose jslpt_lds_bytes) exceeds
 * JSLPP_LDS_LIMIT is JSLP_ERR_UNSUPPORTED; both name the LP.
 */
int jslpc_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                           const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* row_extra, int32_t trace_cap, int32_t max_pivots,
                           int32_t max_nodes);

/* after jslpt_pack_branch_and_cut: out[i] for every LP of the pack whose status was JSLP_OK (all zero for a plain LP); the entry of an
 * LP that failed is left as it was.  JSLP_ERR_STATE before a tree call. */
int jslpc_pack_read_mir(jslpp_pack* p, jslpc_mir_result* out);

#ifdef __cplusplus
}
#endif
#endif /* JSLPC_TREE_MIR_H */
