/*
 * jslpi_tree_incremental.h -- small MILPs with options.useIncremental in a pack: the INCREMENTAL service's tree walked inside the tree
 * kernel, parent checkpoints on the device.  An extension of jslpe_tree_enhanced.h, exported by the HIP library only.
 *
 * A pack made by jslpi_tree_pack_create is a pack of jslpe_tree_enhanced.h some of whose LPs are INCREMENTAL LPs.  An incremental LP runs
 * in an INC build of k_tree_packed (jslpsolver_amd/csrc/jslp_tree.hip.h) under createIncrementalBranchAndCutService
 * (incremental-branch-and-cut.ts:130-499, the service main.ts:62-72 picks for such a model).  It is the enhanced service's walk -- the
 * depth-first stack beside the min-heap, the hybrid switch, the pseudocost table -- with these differences:
 *   - checkpoints: before a node branches, while the walk is depth-first and fewer than max_checkpoints were taken in this call, the
 *     node's whole solved tableau is copied into the LP's checkpoint arena (createCheckpoint, :55-70, :440-445).  The counter only counts
 *     up; no checkpoint is ever freed.  Both children get the checkpoint and their own new cut; best-first children get neither; entries
 *     the hybrid switch moves into the heap keep theirs;
 *   - a node with a checkpoint starts from it (restoreCheckpoint, :72-107: the matrix at the checkpoint's height, the four index maps,
 *     evaluation and feasible) with ONE new cut row on top (:249-253), its slack index width + height - 2.  Rows stack: every level of
 *     such a chain adds a row, even for a variable that has one.  Every other node restores the saved root and adds its whole cut list;
 *   - a node that starts from a checkpoint begins with the checkpoint's evaluation: when it reaches no optimum it leaves that one
 *     behind, and the NEXT node's parentEval reads it (:342);
 *   - pseudocosts are updated from a node's NEW cut only (:358-367): the children pushed while the walk was depth-first have one, with a
 *     checkpoint or without; the root and the best-first children have none;
 *   - branching "strong" does not exist in this service and means pseudocost (:202-219);
 *   - the final re-evaluation of the incumbent starts from the saved root with its whole cut list (:222-226, :492-494).
 * Per LP the call leaves what the reference leaves, bit for bit, as jslpt_tree.h says.
 *
 * An incremental LP has ONE row capacity, height + row_extra[i] (row_extra[i] >= cut_rows[i]), as a MIR LP has: its LDS image is
 * jslpi_tree_lds_bytes = jslpt_lds_bytes at that capacity.  A new cut row that does not fit is the per-LP JSLP_ERR_CAPACITY "row_extra
 * reached"; heap_cap, cut_rows and max_nodes are an enhanced LP's.  The checkpoint arena lies next to the LP's heap in global memory:
 * max_checkpoints[i] slots of jslpi_checkpoint_bytes each -- a 16-byte header {height, feasible, evaluation}, the rows of the row
 * capacity, the whole integer block -- handed out by a counter that starts at 0 with every call.
 *
 * jslpp_pack_set / upload / destroy / size / launches, jslpt_pack_set_integers, jslpt_pack_branch_and_cut, jslpt_pack_read_rhs and
 * jslpp_pack_pivot_trace work on such a pack as on any jslpt pack; jslpt_tree_result and jslpe_pack_read_enhanced report for an incremental
 * LP what they report for an enhanced one.  A call is at most one launch per kernel build that has LPs: (64 | 256 threads) x (plain, opt,
 * mir, enh, inc).  With JSLP_DEBUG_LAUNCH=1 an INC build prints "[jslp] launch k_tree_packed<T,inc 1> n N lds B".
 *
 * Out of scope: an incremental LP with MIR cuts (the service's MIR loop, :261-276: three rounds, feasible nodes only) or with optional
 * objectives (a checkpoint carries none, so the rows a node starts from would depend on the walk) -- JSLP_ERR_ARG naming the LP -- and
 * what jslpt_tree.h leaves out (timeout, keep_solutions; options.tolerance comes through jslpg_tree_tolerance.h).
 */
#ifndef JSLPI_TREE_INCREMENTAL_H
#define JSLPI_TREE_INCREMENTAL_H

#include "jslpe_tree_enhanced.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSLPI_MAX_CHECKPOINTS 64         /* the most max_checkpoints[i] may be                                      */
#define JSLPI_CHECKPOINTS_DEFAULT 50     /* maxCheckpoints of the reference (main.ts never passes another value)   */

typedef struct jslpi_tree_result {
    int32_t checkpoints_used;            /* checkpoints taken in this call                                          */
    int32_t incremental_nodes;           /* nodes that started from a checkpoint                                    */
    int32_t rows_high_water;             /* most rows beyond `height` a node's tableau had                          */
    int32_t checkpoint_rows_high_water;  /* most rows beyond `height` a checkpoint held                             */
    int32_t reserved[4];                 /* 0                                                                       */
} jslpi_tree_result;

/*
 * jslpe_tree_pack_create_mixed with, per LP, incremental[i] (0 / 1) and max_checkpoints[i] (0 .. JSLPI_MAX_CHECKPOINTS; read for an
 * incremental LP only).  An incremental LP's row_extra[i] >= cut_rows[i] is its row capacity and makes no MIR LP of it; its
 * node_selection[i] / branching[i] of 0 mean JSLPE_HYBRID / JSLPE_PSEUDOCOST.  JSLP_ERR_ARG naming the LP: incremental[i] outside 0 / 1,
 * max_checkpoints[i] out of range, no row_extra or one below cut_rows[i], optional objectives (n_optional[i] > 0).  JSLP_ERR_UNSUPPORTED
 * naming the LP: jslpi_tree_lds_bytes at its row capacity beyond 64 KiB.  n_optional may be NULL; row_extra may be NULL when no LP is
 * incremental.  Every argument is checked before the first device call.
 */
int jslpi_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                           const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, const int32_t* row_extra,
                           const int32_t* node_selection, const int32_t* branching, const int32_t* incremental,
                           const int32_t* max_checkpoints, int32_t trace_cap, int32_t max_pivots, int32_t max_nodes);

/* bytes of dynamic LDS an incremental LP needs at row_capacity = height + row_extra: jslpt_lds_bytes; 0 for a bad shape */
int64_t jslpi_tree_lds_bytes(int32_t height, int32_t width, int32_t row_capacity);

/* bytes of ONE checkpoint slot of such an LP (its arena holds max_checkpoints of them); 0 for a bad shape */
int64_t jslpi_checkpoint_bytes(int32_t height, int32_t width, int32_t row_capacity);

/* after jslpt_pack_branch_and_cut: out[i] for every LP of the pack whose status was JSLP_OK (all zero for an LP that is not incremental);
 * the entry of an LP that failed is left as it was.  JSLP_ERR_STATE before a tree call. */
int jslpi_pack_read_incremental(jslpp_pack* p, jslpi_tree_result* out);

#ifdef __cplusplus
}
#endif
#endif /* JSLPI_TREE_INCREMENTAL_H */
