/*
 * jslpp_packed.h -- a pack of small LPs solved in LDS, one launch per batch: an extension of the C ABI in jslp_engine.h, exported by
 * the HIP library only (like jslpm_many.h, jslpx_branch.h and jslpr_mir.h).
 *
 * A `jslpp_pack` owns n independent small tableaus in ONE device arena: one H2D copy uploads all of them, one launch (per kernel
 * build) solves each in a workgroup of its own with the WHOLE tableau and its index maps in LDS (k_simplex_packed,
 * jslpsolver_amd/csrc/jslp_packed.hip.h), and one D2H copy brings back every state, RHS column and row map.  No jslp_engine is
 * involved: a pack call costs the host a few hundred nanoseconds per LP, not an engine's stream, events and descriptor.
 *
 * Per LP, jslpp_pack_simplex leaves exactly what jslp_engine_simplex leaves on a fresh engine created with
 * jslp_engine_create(height, width, row_capacity = height, precision) after the same upload: the result struct (flags, pivot
 * counts, cycle phase / start / length, obj_cell, evaluation -- kept when the call reaches no optimum), the final tableau, the four
 * index maps and the pivot trace, bit for bit (simplex.ts phase 1, phase 2, pivot and checkForCycles).
 *
 * What differs from an engine, by design:
 *   - the cycle-check history of an LP holds JSLPP_HIST_CAP pairs per phase (an engine: 2^20).  A phase that appends more ends with
 *     JSLP_ERR_CAPACITY in that LP's status, as an engine's does at its own capacity;
 *   - the pivot trace holds trace_cap pairs per LP (0: pivots are counted, not recorded);
 *   - a pack has no cut rows, no save / restore / relax, no work counters: none of them has an entry point here (optional
 *     objectives come through jslps_soft.h, cut rows and trees through jslpt_tree.h).  The one refusal a caller meets is the LDS
 *     limit: an LP whose LDS image (jslpp_lds_bytes) exceeds 64 KiB is refused at create with JSLP_ERR_UNSUPPORTED.  Such models
 *     go through a jslp_engine -- or, up to 156 KiB, through a pack made with big_lds (jslpb_big_lds.h).
 *
 * Errors: argument and state errors are reported before any work, and then nothing is solved.  An LP that reaches its pivot cap or
 * its history capacity gets the engine's code (JSLP_ERR_CAPACITY) in status[i] and its out[i] is left as it was; every other LP is
 * still solved; the call returns the first non-OK status (lowest i) and jslp_last_error() names that LP ("LP <i>").
 *
 * Threading: a pack belongs to one host thread at a time; different packs may be driven from different threads.
 */
#ifndef JSLPP_PACKED_H
#define JSLPP_PACKED_H

#include "jslp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSLPP_LDS_LIMIT 65536 /* the dynamic LDS the pack kernels are launched with at most                    */
#define JSLPP_HIST_CAP 4096   /* pairs of one phase's cycle-check history, per LP                              */

typedef struct jslpp_pack jslpp_pack;

/* Dynamic LDS, in bytes, that an LP of this shape needs (the padded tableau, the pivot column, the four index maps and the
 * unrestricted flags).  A pure function: no device call.  0 when height < 2 or width < 2.  Monotone in both arguments. */
int64_t jslpp_lds_bytes(int32_t height, int32_t width);

/*
 * n LPs of height[i] x width[i] with tolerance precision[i] (tableau.ts:96).  trace_cap: pivot pairs recorded per LP (>= 0).
 * max_pivots > 0 caps phase-1 plus phase-2 pivots per LP and call; 0 = the engine's safety cap (2000000 + 200 x (height + width)).
 * Refused before anything is allocated: n < 0, null arrays with n > 0, a height or width below 2, a precision that is not a
 * number (JSLP_ERR_ARG); an LP whose jslpp_lds_bytes exceeds JSLPP_LDS_LIMIT (JSLP_ERR_UNSUPPORTED, "LP <i>").
 */
int jslpp_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                      int32_t trace_cap, int32_t max_pivots);
/* hands the stream and the events back to the library's resource pool (jslp_release_pooled_resources frees them) */
void jslpp_pack_destroy(jslpp_pack* p);
int32_t jslpp_pack_size(const jslpp_pack* p);

/*
 * Filling, as jslp_engine_host_matrix + jslp_engine_upload do for one engine.  host_matrix hands out LP i's zero-filled
 * height x width matrix inside the pack's pinned upload image (reference layout, stride = width); it stays valid until destroy.
 * set copies LP i's matrix (NULL: keep what the image holds, e.g. what was written through host_matrix), var_index_by_row
 * (height entries, [0] = -1), var_index_by_col (width entries, [0] = -1) and the unrestricted variable indexes.  An index outside
 * the maps (width + 2 x height + 2 entries, as jslp_engine_create sizes them) -> JSLP_ERR_ARG naming the LP.
 * upload is ONE H2D copy of the image; it resets every LP's state, evaluation, counters and trace like jslp_engine_upload.
 * Every LP must have been set since create (JSLP_ERR_STATE names the first that was not).
 */
int jslpp_pack_host_matrix(jslpp_pack* p, int32_t i, double** matrix, int64_t* n_doubles);
int jslpp_pack_set(jslpp_pack* p, int32_t i, const double* matrix, const int32_t* var_index_by_row, const int32_t* var_index_by_col,
                   const int32_t* unrestricted_var_indexes, int32_t n_unrestricted);
int jslpp_pack_upload(jslpp_pack* p);

/*
 * Tableau.simplex() of every LP: at most one launch per kernel build (one-wave workgroups for the tiny LPs, 256 threads for the
 * rest), then one D2H copy of [states | RHS columns | row maps].  check_cycles: n flags, or NULL = all 1.  out: n results.
 * status: n codes, or NULL.  *device_ms (may be NULL): the time between HIP events around the launches on the pack's stream.
 * A second call without an upload continues from the final tableaus.
 */
int jslpp_pack_simplex(jslpp_pack* p, const int32_t* check_cycles, jslp_simplex_result* out, int32_t* status, double* device_ms);
/* kernel launches of the last jslpp_pack_simplex: 0, 1 or 2 -- up to 4 in a pack with optional objectives (jslps_soft.h), up to 6 with
 * large LPs (jslpb_big_lds.h) */
int32_t jslpp_pack_launches(const jslpp_pack* p);

/*
 * The read-back of the last jslpp_pack_simplex, in the pack's pinned result block: the RHS columns and the row maps of all LPs
 * one after the other, LP i at [offsets[i], offsets[i + 1]) (n + 1 offsets).  Valid until the next call on the pack.
 */
int jslpp_pack_read_rhs(jslpp_pack* p, const double** rhs, const int32_t** var_index_by_row, const int64_t** offsets);
/* jslp_engine_download for LP i: matrix height x width (stride width); any pointer may be NULL */
int jslpp_pack_download(jslpp_pack* p, int32_t i, double* matrix, int32_t* var_index_by_row, int32_t* var_index_by_col,
                        int32_t* row_by_var_index, int32_t* col_by_var_index);
/* jslp_engine_pivot_trace for LP i: *n_pivots = pivots since the upload; asking for more pairs than trace_cap recorded fails
 * with JSLP_ERR_CAPACITY (the count is still returned) */
int jslpp_pack_pivot_trace(jslpp_pack* p, int32_t i, int32_t* row_col, int64_t max_pairs, int64_t* n_pivots);

#ifdef __cplusplus
}
#endif
#endif /* JSLPP_PACKED_H */
