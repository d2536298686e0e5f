/*
 * jslpe_tree_enhanced.h -- small MILPs with options.nodeSelection / options.branching in a pack: the ENHANCED service's tree walked inside
 * the tree kernel.  An extension of jslpt_tree.h, exported by the HIP library only.
 *
 * A pack made by jslpe_tree_pack_create is a pack of jslpt_tree.h some of whose LPs are ENHANCED LPs.  An enhanced LP runs in an ENH
 * build of k_tree_packed (jslpsolver_amd/csrc/jslp_tree.hip.h) under createEnhancedBranchAndCutService (enhanced-branch-and-cut.ts:58-437,
 * the service main.ts:74-80 picks for such a model).  The tableau, the saved root, the cut rows and the simplex are the default service's;
 * the tree policy differs:
 *   - node selection: a depth-first stack beside the min-heap.  depth-first and hybrid start on the stack, best-first on the heap; on the
 *     stack the LOW child is pushed first, so the high child is evaluated first; hybrid moves what the stack holds into the heap, from the
 *     top, at the first accepted integral node;
 *   - pseudocosts: one {upSum, upCount, downSum, downCount} per integer variable, updated from a node's LAST cut and the evaluation the
 *     PREVIOUS node left, before the tie check; every call starts with an empty table;
 *   - branching: most-fractional, pseudocost (getScore) or strong (the five most fractional, scored by getScore once both directions of a
 *     variable were seen twice, by fraction * (1 - fraction) until then); a node without a candidate is dropped.
 * Per LP the call leaves what the reference leaves, bit for bit, as jslpt_tree.h says.
 *
 * An enhanced LP's LDS image is exactly a tree LP's (jslpt_lds_bytes): it fits the pack when it would fit as a default one.  The stack
 * and the heap share the LP's heap_cap entries; the pseudocost table lies next to them in global memory.  Its integer variables
 * (jslpt_pack_set_integers) are distinct (JSLP_ERR_ARG otherwise).
 *
 * jslpp_pack_set / upload / destroy / size / launches, jslpt_pack_set_integers, jslpt_pack_branch_and_cut, jslpt_pack_read_rhs and
 * jslpp_pack_pivot_trace work on such a pack as on any jslpt pack.  In jslpt_tree_result of an enhanced LP heap_high_water is the most
 * entries stack and heap held TOGETHER -- what heap_cap has to hold -- and nodes_pushed counts new branches (the root's included), not the
 * entries the hybrid switch moves; the other fields are as before.  A full stack + heap is the per-LP JSLP_ERR_CAPACITY "heap_cap reached".
 * A call is at most one launch per kernel build that has LPs: (64 | 256 threads) x (plain, opt, mir, enh), routed by the tableau cells
 * at the row capacity as before.  With JSLP_DEBUG_LAUNCH=1 an ENH build prints "[jslp] launch k_tree_packed<T,enh 1> n N lds B".
 *
 * Out of scope: an enhanced LP with optional objectives or with MIR cuts (the enhanced service's MIR loop is another loop: three rounds,
 * feasible tableaus only) -- JSLP_ERR_ARG naming the LP -- and what jslpt_tree.h leaves out.
 */
#ifndef JSLPE_TREE_ENHANCED_H
#define JSLPE_TREE_ENHANCED_H

#include "jslpc_tree_mir.h"
#include "jslps_soft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* node_selection[i] */
#define JSLPE_BEST_FIRST 1
#define JSLPE_DEPTH_FIRST 2
#define JSLPE_HYBRID 3
/* branching[i] */
#define JSLPE_MOST_FRACTIONAL 1
#define JSLPE_PSEUDOCOST 2
#define JSLPE_STRONG 3

typedef struct jslpe_tree_result {
    int32_t solutions_found;      /* accepted integral nodes                                                          */
    int32_t stack_high_water;     /* most entries the depth-first stack held                                          */
    int32_t moved_to_heap;        /* entries the hybrid switch moved from the stack into the heap                     */
    int32_t pseudo_updates;       /* pseudocost updates                                                               */
    int32_t scored_by_pseudocost; /* `strong` candidates scored by getScore: both directions seen at least twice      */
    int32_t dropped_nodes;        /* nodes that were not integral and had no branching candidate                      */
    int32_t reserved[2];          /* 0                                                                                */
} jslpe_tree_result;

/*
 * jslpt_pack_create with, per LP, node_selection[i] and branching[i]: both 0 -> the LP runs under the default service exactly as
 * jslpt_pack_create makes it; otherwise an enhanced LP, and one of the two left 0 gets its default, JSLPE_HYBRID / JSLPE_PSEUDOCOST
 * (main.ts:76-77).  A value outside 0..3 is JSLP_ERR_ARG naming the LP; the LDS limit is jslpt_pack_create's.
 */
int jslpe_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                           const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* node_selection, const int32_t* branching,
                           int32_t trace_cap, int32_t max_pivots, int32_t max_nodes);

/*
 * The same for a pack that also holds LPs with optional objectives (n_optional, as jslps_tree_pack_create; may be NULL) or MIR LPs
 * (row_extra, as jslpc_tree_pack_create; may be NULL): every kind of tree LP in ONE pack.  An enhanced LP with n_optional[i] > 0 or
 * row_extra[i] >= 0, and a MIR LP with optional objectives, are JSLP_ERR_ARG naming the LP.
 */
int jslpe_tree_pack_create_mixed(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                                 const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, const int32_t* row_extra,
                                 const int32_t* node_selection, const int32_t* branching, int32_t trace_cap, int32_t max_pivots,
                                 int32_t max_nodes);

/* after jslpt_pack_branch_and_cut: out[i] for every LP of the pack whose status was JSLP_OK (all zero for an LP under the default
 * service); the entry of an LP that failed is left as it was.  JSLP_ERR_STATE before a tree call. */
int jslpe_pack_read_enhanced(jslpp_pack* p, jslpe_tree_result* out);

#ifdef __cplusplus
}
#endif
#endif /* JSLPE_TREE_ENHANCED_H */
