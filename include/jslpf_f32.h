/*
 * jslpf_f32.h -- the fp32 experiment as a sweep: an extension of the C ABI in jslp_engine.h, exported by the HIP library only.
 *
 * jslpf_simplex_f32_sweep runs simplex() on fp32 copies of the engine's LIVE tableau at n tolerances.  Run i returns exactly what
 * jslp_engine_simplex_f32(e, precisions[i], check_cycles, ...) returns, field by field and bit by bit (`evaluation` restated from
 * that run's obj_cell and precision).  The fp64 state is untouched, no pivot is traced and nothing is counted in jslp_work_counters.
 *
 * path:
 *   JSLPF_PATH_SELECT_UPDATE  the loop of jslp_engine_simplex_f32 (one select and one update launch per pivot), one run after the other
 *   JSLPF_PATH_ONE_LAUNCH     ONE launch of k32_simplex_lds for the whole call: one workgroup per run, each on its own fp32 copy, no
 *                             host round trip per pivot; JSLP_ERR_UNSUPPORTED when the tableau's fp32 LDS state does not fit
 *   JSLPF_PATH_AUTO           one launch when that state fits and the tableau is small, or mid-size and sparse (the bounds of the
 *                             engine's own one-workgroup policy); the select + update loop otherwise
 * *path_taken (when not NULL) receives JSLPF_PATH_SELECT_UPDATE or JSLPF_PATH_ONE_LAUNCH.
 *
 * out: n results.  rhs / var_index_by_row: n x stride arrays (run i's RHS column widened to double / row map at [i * stride ...]), or
 * NULL.  status: n codes, or NULL.  device_ms (when not NULL): one number for the call -- the launch, or the sum of the runs' loops.
 *
 * Errors:
 *   - reported before any device is touched, and then nothing runs: n < 0, n > JSLPF_MAX_RUNS, a null `precisions` or `out` with
 *     n > 0, an unknown `path`, a precision that is not > 0 -> JSLP_ERR_ARG; a null or not-uploaded engine -> JSLP_ERR_STATE.
 *     n == 0 returns JSLP_OK.
 *   - from the engine's state: `stride` below the live height with a non-NULL array -> JSLP_ERR_ARG; optional objectives ->
 *     JSLP_ERR_UNSUPPORTED; JSLPF_PATH_ONE_LAUNCH on a tableau whose LDS state does not fit -> JSLP_ERR_UNSUPPORTED.
 *   - an error of one run's solve (iteration cap, history capacity ...) goes into status[i]; out[i] is then left as it was and every
 *     other run still finishes.  The call returns the first non-OK status (lowest i) and jslp_last_error() names that run's index.
 */
#ifndef JSLPF_F32_H
#define JSLPF_F32_H

#include "jslp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JSLPF_MAX_RUNS 64

#define JSLPF_PATH_AUTO          0
#define JSLPF_PATH_SELECT_UPDATE 1   /* today's loop, one run after the other */
#define JSLPF_PATH_ONE_LAUNCH    2   /* k32_simplex_lds or JSLP_ERR_UNSUPPORTED */
int jslpf_simplex_f32_sweep(jslp_engine* e, const double* precisions, int32_t n, int check_cycles, int32_t path,
                            jslp_simplex_result* out, double* rhs, int32_t* var_index_by_row, int32_t stride,
                            int32_t* status, int32_t* path_taken, double* device_ms);

#ifdef __cplusplus
}
#endif
#endif /* JSLPF_F32_H */
