/*
 * jslpg_tree_tolerance.h -- options.tolerance honoured inside the tree kernel.  An extension of jslpi_tree_incremental.h, exported by the
 * HIP library only.
 *
 * A pack made by jslpg_tree_pack_create is a pack of jslpi_tree_incremental.h some of whose LPs carry the model's options.tolerance.  Such an
 * LP runs in the TOL build of its kind -- k_tree_packed (jslpsolver_amd/csrc/jslp_tree.hip.h) has a sixth template flag, and every one of the
 * ten builds (plain, OPT, MIR, ENH, INC at 64 or 256 threads) a TOL twin; the ten builds themselves compile to the instructions they had, so
 * an LP without tolerance pays nothing -- and its walk ends as the reference's three services end theirs
 * (branch-and-cut.ts:57-87, enhanced-branch-and-cut.ts:228-270, incremental-branch-and-cut.ts:297-324, the same text):
 *   - bestPossibleEval starts at 0 and is set ONCE, by the LP's first simplex that ends optimal (tableau.ts:420-430: setEvaluation while
 *     simplexIters === 0) -- as a rule the root's first, before its MIR rounds; a later node's when the root reaches no optimum; never by a
 *     restore of the saved root or of a checkpoint.  It is the rounded evaluation Math.round((EPSILON + A[0]) * rc) / rc;
 *   - at the top of every turn of the node loop, behind the emptiness test of the container in use and BEFORE the pop,
 *     acceptableThreshold = bestPossibleEval * factor with factor = 1 + tolerance for a minimisation and 1 - tolerance for a maximisation
 *     (computed on the host in double, as the JavaScript computes it), and a turn that finds bestEvaluation < acceptableThreshold (strict;
 *     false for NaN) lowers toleranceFlag;
 *   - that turn still runs: its node is popped, pruned or evaluated, may become the incumbent, may push children.  The loop ends at the NEXT
 *     turn's condition -- the stop is one node late -- and an empty container ends it first.  max_nodes and the other capacities keep their
 *     places: an LP that reaches max_nodes on the turn that lowered the flag reports the capacity;
 *   - the final re-evaluation of the incumbent runs as always.
 * Per LP the call leaves what the reference leaves, bit for bit, as jslpt_tree.h says.
 *
 * tolerance[i] <= 0 or NaN means none, as `tolerance > 0` decides in the reference; any other value is taken as it is, values >= 1 (a
 * maximisation's factor is then <= 0) and +Infinity included.  An LP without tolerance is walked, byte for byte, as the same LP of a pack made
 * by jslpi_tree_pack_create, in the same build, launched with the same line.  A call is at most one launch per kernel build that has LPs:
 * (64 | 256 threads) x (plain, opt, mir, enh, inc) x (without, with tolerance).  With JSLP_DEBUG_LAUNCH=1 a TOL build prints
 * "[jslp] launch k_tree_packed<T,tol 1> n N lds B", "<T,inc 1,tol 1>" and so on.  jslpp_pack_simplex knows no tolerance and launches as before.
 *
 * Out of scope: timeout (a clock cannot be pinned) and keep_solutions.
 */
#ifndef JSLPG_TREE_TOLERANCE_H
#define JSLPG_TREE_TOLERANCE_H

#include "jslpi_tree_incremental.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jslpg_tolerance_result {
    double best_possible;  /* bestPossibleEval when the walk ended: the LP's first optimal evaluation, 0 when there was none.  */
                           /* An INTEGRAL ROOT leaves its own evaluation here, as the reference's tableau does, not 0: of such */
                           /* an LP's record the three other fields are zero                                                   */
    double threshold;      /* the last acceptableThreshold computed; 0 * Infinity is reported as the quiet NaN 0x7ff8000000000000 */
    int32_t stopped;       /* 1: the loop ended on toleranceFlag with entries still waiting                                    */
    int32_t left;          /* the entries heap and stack held at that moment; 0 when stopped is 0                              */
    int32_t reserved[2];   /* 0                                                                                                */
} jslpg_tolerance_result;

/*
 * jslpi_tree_pack_create with, per LP, tolerance[i] and minimize[i] (1: the model minimises, 0: it maximises; read for every LP when the
 * array is given).  Both may be NULL, each on its own: no tolerance array makes the pack jslpi_tree_pack_create's; no minimize array means
 * every LP minimises.  JSLP_ERR_ARG naming the LP: minimize[i] outside 0 / 1, and what jslpi_tree_pack_create refuses.  Every argument is checked before the
 * first device call.
 */
int jslpg_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                           const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, const int32_t* row_extra,
                           const int32_t* node_selection, const int32_t* branching, const int32_t* incremental,
                           const int32_t* max_checkpoints, const double* tolerance, const int32_t* minimize, int32_t trace_cap,
                           int32_t max_pivots, int32_t max_nodes);

/* after jslpt_pack_branch_and_cut: out[i] for every LP of the pack whose status was JSLP_OK (all zero for an LP without tolerance); the
 * entry of an LP that failed is left as it was.  JSLP_ERR_STATE before a tree call. */
int jslpg_pack_read_tolerance(jslpp_pack* p, jslpg_tolerance_result* out);

#ifdef __cplusplus
}
#endif
#endif /* JSLPG_TREE_TOLERANCE_H */
