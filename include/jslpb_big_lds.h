/*
 * jslpb_big_lds.h -- packs whose LPs may take the whole LDS of a compute unit.  An extension of jslpg_tree_tolerance.h (and so of
 * jslpp_packed.h, jslps_soft.h and jslpt_tree.h), exported by the HIP library only.
 *
 * A pack of jslpp_packed.h stops at a 64 KiB LDS image per LP (JSLPP_LDS_LIMIT), the limit of other chips.  A compute unit of the MI355X has
 * 160 KiB of LDS and one workgroup may have all of it.  A pack made by one of the two creates below with big_lds = 1 takes LPs up to
 * JSLPB_LDS_LIMIT bytes: 160 KiB minus a 4 KiB reserve for the kernels' own static LDS (the cross-wave stage of the reductions, the first pairs
 * of the cycle-check history, the tree's scalars).  A square LP then fits up to 138 x 138 instead of 87 x 87.
 *
 * In such a pack
 *   - an LP whose LDS image (jslpp_lds_bytes, jslps_lds_bytes, jslpt_lds_bytes or jslps_tree_lds_bytes, whichever applies) is at most
 *     JSLPP_LDS_LIMIT bytes is exactly the LP the older create makes: the same image, the same build (64 or 256 threads), the same
 *     JSLP_DEBUG_LAUNCH line;
 *   - an LP above JSLPP_LDS_LIMIT and at most JSLPB_LDS_LIMIT bytes is a LARGE LP.  It runs in the large build of its kind, a workgroup of
 *     jslpb_pack_big_threads() threads that has its compute unit to itself (jslpsolver_amd/csrc/jslp_tu_packed_big.hip: the same kernel
 *     templates at that thread count).  Large builds exist for k_simplex_packed, plain and with optional objectives, and for k_tree_packed
 *     under the default service, plain and with optional objectives.  Their launch lines keep their form:
 *     "[jslp] launch k_simplex_packed<T> n N lds B" with B > 65536, "<T,opt 1>", "k_tree_packed<T>" and so on;
 *   - a MIR, an enhanced or an incremental LP, and any LP with a tolerance, keeps the 64 KiB rule: one whose image exceeds JSLPP_LDS_LIMIT is
 *     refused with JSLP_ERR_UNSUPPORTED naming the LP and its kind;
 *   - an LP whose image exceeds JSLPB_LDS_LIMIT is refused with JSLP_ERR_UNSUPPORTED naming the LP.
 * Everything else works on such a pack unchanged: set, upload, simplex, branch_and_cut, every read-back, the optional-objective setters and
 * getters.  A large LP's heap, cut-list pool and share of the result block are sized as any LP's, from its cut rows and its row capacity.
 * jslpp_pack_launches counts up to 6 launches of a plain simplex on a pack with large LPs.
 *
 * Every argument is checked before the first device call.  After the argument checks a create with big_lds = 1 asks the device for
 * hipDeviceAttributeMaxSharedMemoryPerBlock and fails with JSLP_ERR_UNSUPPORTED naming the device when that is below 163840 bytes.
 *
 * Out of scope: large builds of the MIR, enhanced, incremental and tolerance kinds; two LPs per compute unit between 64 and 80 KiB as a tuning
 * target; one LP shared by several workgroups; timeout and keep_solutions.
 */
#ifndef JSLPB_BIG_LDS_H
#define JSLPB_BIG_LDS_H

#include "jslpg_tree_tolerance.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSLPB_LDS_LIMIT 159744 /* the dynamic LDS a large build is launched with at most: 160 KiB minus 4 KiB for the kernels' static LDS */

/*
 * jslps_pack_create (jslps_soft.h) with big_lds behind its arguments.  big_lds = 0: the call IS jslps_pack_create, byte for byte;
 * big_lds = 1: the pack's limit is JSLPB_LDS_LIMIT; any other value: JSLP_ERR_ARG.  n_optional may be NULL, as there.
 */
int jslpb_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                      const int32_t* n_optional, int32_t trace_cap, int32_t max_pivots, int32_t big_lds);

/*
 * jslpg_tree_pack_create (jslpg_tree_tolerance.h) with big_lds behind its arguments, as above.  Every table that may be NULL there may be
 * NULL here.
 */
int jslpb_tree_pack_create(jslpp_pack** out, int device, int32_t n, const int32_t* height, const int32_t* width, const double* precision,
                           const int32_t* cut_rows, const int32_t* heap_cap, const int32_t* n_optional, const int32_t* row_extra,
                           const int32_t* node_selection, const int32_t* branching, const int32_t* incremental,
                           const int32_t* max_checkpoints, const double* tolerance, const int32_t* minimize, int32_t trace_cap,
                           int32_t max_pivots, int32_t max_nodes, int32_t big_lds);

/* the thread count of the large builds (the T of their launch lines).  A pure function: no device call. */
int32_t jslpb_pack_big_threads(void);

#ifdef __cplusplus
}
#endif
#endif /* JSLPB_BIG_LDS_H */
