/*
 * jslpm_many.h -- many independent LPs in one call: an extension of the C ABI in jslp_engine.h, exported by the HIP library only.
 *
 * jslpm_simplex_many runs simplex() on n engines at once.  Every engine ends exactly as if
 * jslp_engine_simplex(engines[i], check_cycles[i], &out[i]) had been called on it alone: the same result (evaluation,
 * pivot counts, cycle phase / start / length), the same final tableau, index maps and pivot trace, the same work counters,
 * and later calls on the engine (save / restore / relax / download ...) behave the same.
 *
 * Routing, per engine and by the engine's own policy (JSLP_FORCE_PATH read at create still applies):
 *   - an engine whose simplex() runs in one workgroup with its selection state in LDS joins ONE launch of
 *     k_simplex_lds_many: one workgroup per LP (one launch per kernel build: plain, optional objectives).
 *     jslp_engine_last_path() then reads "workgroup-many".
 *   - every other engine (chip-wide tableaus, JSLP_NO_WGLDS=1, tableaus whose LDS state does not fit) is solved through
 *     its own path, one after another, AFTER the batch launch has completed: a cooperative chip-wide launch never
 *     overlaps the batch.
 * The launch waits for the work already enqueued on every member's stream, and every member's stream waits for the launch.
 *
 * Errors:
 *   - argument errors are reported before any work, and then nothing is solved: n < 0, a null `engines` or `out` with
 *     n > 0, an engine listed twice, engines on different devices -> JSLP_ERR_ARG; a null or not-uploaded engine ->
 *     JSLP_ERR_STATE.  n == 0 returns JSLP_OK.
 *   - an error of one LP's solve (iteration cap, history capacity ...) goes into status[i] (when `status` is not NULL);
 *     out[i] is then left as it was.  Every other LP is still solved.  The call returns the first non-OK status (lowest i)
 *     and jslp_last_error() names that LP's index.
 */
#ifndef JSLPM_MANY_H
#define JSLPM_MANY_H

#include "jslp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* check_cycles: n flags, or NULL = all 1.  out: n results.  status: n codes (JSLP_OK or the LP's error), or NULL. */
int jslpm_simplex_many(jslp_engine* const* engines, int32_t n, const int32_t* check_cycles, jslp_simplex_result* out,
                       int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* JSLPM_MANY_H */
