/*
 * jslps_soft.h -- optional objectives in a pack: small LPs and MILPs with soft constraints solved in LDS.  An extension of
 * jslpp_packed.h and jslpt_tree.h, exported by the HIP library only.
 *
 * Every soft constraint of a model (a constraint with `weight` or `priority`) becomes an optional objective: a further cost row that
 * decides the entering column whenever no column prices out on the main cost row (simplex.ts:221-263) and that every pivot updates
 * with exact `!== 0` tests (simplex.ts:394-412).  A jslp_engine takes them through jslp_engine_set_optional_objectives; a pack made by
 * one of the creates below takes them per LP and keeps them in LDS beside the tableau:
 *
 *   arena image of an LP   n_optional x width doubles (stride width) directly behind the matrix;
 *   LDS                    n_optional x S doubles directly behind the pivot column, S = the tableau's odd row stride.
 *
 * The LPs with optional objectives run in builds of their own of the two pack kernels (k_simplex_packed<.., OPT = true>,
 * k_tree_packed<.., OPT = true>), so a call is at most FOUR launches -- 64 or 256 threads, each with or without OPT --, and a pack
 * without optional objectives launches exactly what it launched before.  JSLP_DEBUG_LAUNCH prints an OPT launch as
 * `k_simplex_packed<64,opt 1> n N lds B`.  Which thread count an LP gets is decided by its tableau cells at the row capacity alone.
 *
 * Per LP the calls leave what an engine leaves after the same upload and jslp_engine_set_optional_objectives, bit for bit: the result,
 * the tableau or RHS column, the maps, the pivot trace and the optional rows.  In a pack with trees the rows are saved with the root
 * and come back with every restore (backup.ts:35-43, 94-104); a node whose evaluation equals the incumbent's is compared with it on
 * column 0 of the rows, in priority order (branch-and-cut.ts:107-127, 138-141); the rows left are those of the last relaxation
 * evaluated -- the incumbent's after the final re-evaluation.
 *
 * All functions with n_optional == NULL, or 0 for every LP, are the functions of jslpp_packed.h / jslpt_tree.h.
 */
#ifndef JSLPS_SOFT_H
#define JSLPS_SOFT_H

#include "jslpt_tree.h"

#ifdef __cplusplus
extern "C" {
#endif

/* jslpp_lds_bytes for an LP with n_optional optional objectives.  Pure; equal to jslpp_lds_bytes at n_optional == 0; monotone in
 * every argument; 0 when height < 2, width < 2 or n_optional < 0. */
int64_t jslps_lds_bytes(int32_t height, int32_t width, int32_t n_optional);
/* the same for jslpt_lds_bytes (also 0 when row_capacity < height) */
int64_t jslps_tree_lds_bytes(int32_t height, int32_t width, int32_t row_capacity, int32_t n_optional);

/*
 * jslpp_pack_create / jslpt_pack_create with n_optional[i] >= 0 optional objectives reserved for LP i (NULL: none for any LP).  A
 * negative count -> JSLP_ERR_ARG naming the LP; an LP whose jslps_lds_bytes / jslps_tree_lds_bytes exceeds JSLPP_LDS_LIMIT ->
 * JSLP_ERR_UNSUPPORTED naming the LP ("LP <i>").
 */
int jslps_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                      const int32_t* n_optional, int32_t trace_cap, int32_t max_pivots);
int jslps_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                           const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, int32_t trace_cap,
                           int32_t max_pivots, int32_t max_nodes);

/*
 * LP i's optional objectives: n_optional[i] x width doubles, row o = optionalObjectives[o].reducedCosts in priority order, laid
 * out as jslp_engine_set_optional_objectives takes them.  Before jslpp_pack_upload, which fails with JSLP_ERR_STATE naming the
 * first LP that has rows reserved and none set.  An LP created with n_optional[i] == 0 -> JSLP_ERR_ARG.
 */
int jslps_pack_set_optional_objectives(jslpp_pack* p, int32_t i, const double* rows);
/* LP i's rows after the last jslpp_pack_simplex / jslpt_pack_branch_and_cut, out of the pack's pinned result block (they travel home
 * in the call's one D2H copy).  *n_out (may be NULL) = n_optional[i].  JSLP_ERR_STATE before the first solve after an upload.
 * jslpp_pack_simplex also writes them into the arena image, so a second call without an upload continues from them. */
int jslps_pack_get_optional_objectives(jslpp_pack* p, int32_t i, double* rows, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* JSLPS_SOFT_H */
