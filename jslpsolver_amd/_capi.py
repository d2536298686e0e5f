"""ctypes binding of the C ABI declared in include/jslp_engine.h (SYMBOLS) and of its HIP-only extensions include/jslpx_branch.h
(BRANCH_SYMBOLS), include/jslpm_many.h (MANY_SYMBOLS), include/jslpf_f32.h (F32_SYMBOLS), include/jslpr_mir.h (MIR_SYMBOLS) and
include/jslpp_packed.h (PACK_SYMBOLS) with include/jslpt_tree.h (TREE_SYMBOLS), include/jslps_soft.h (SOFT_SYMBOLS) and
include/jslpc_tree_mir.h (TREE_MIR_SYMBOLS), include/jslpe_tree_enhanced.h (TREE_ENH_SYMBOLS), include/jslpi_tree_incremental.h
(TREE_INC_SYMBOLS), include/jslpg_tree_tolerance.h (TREE_TOL_SYMBOLS) and include/jslpb_big_lds.h (BIG_SYMBOLS).

The same binding class serves two libraries that export identical symbols:
  * jslpsolver_amd/csrc/libjslp_hip.so -- the product (hand-written HIP kernels, gfx950)
  * oracle/libjslp_oracle.so           -- TEST ONLY, loaded explicitly by tests / smoke / cpu_baseline
`load_hip()` is the only loader the product uses and it raises when the HIP library is missing:
there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.environ.get("JSLP_HIP_LIBRARY") or os.path.join(_HERE, "csrc", "libjslp_hip.so")  # env: debug builds only

JSLP_OK = 0
JSLP_ERR_ARG, JSLP_ERR_DEVICE, JSLP_ERR_NOMEM, JSLP_ERR_STATE, JSLP_ERR_CAPACITY, JSLP_ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6
JSLP_CUT_MIN = 0
JSLP_CUT_MAX = 1


class SimplexResult(C.Structure):
    """struct jslp_simplex_result (include/jslp_engine.h)"""

    _fields_ = [
        ("feasible", C.c_int32),
        ("bounded", C.c_int32),
        ("optimal", C.c_int32),
        ("unbounded_var_index", C.c_int32),
        ("pivots_phase1", C.c_int32),
        ("pivots_phase2", C.c_int32),
        ("cycle_phase", C.c_int32),
        ("cycle_start", C.c_int32),
        ("cycle_length", C.c_int32),
        ("height", C.c_int32),
        ("obj_cell", C.c_double),
        ("evaluation", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class WorkCounters(C.Structure):
    """struct jslp_work_counters (include/jslp_engine.h)"""

    _fields_ = [(name, C.c_int64) for name in ("relaxations", "simplex_calls", "pivots", "gated_cells", "gated_rows",
                                              "restored_rows", "cut_rows", "height_sum", "resident_aborts", "resident_handovers",
                                              "resident_launches", "resident_refusals", "node_queue_launches", "resident_fetch_retries")]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


_P = C.POINTER
_i32p = _P(C.c_int32)
_f64p = _P(C.c_double)
_i8p = _P(C.c_int8)

# name -> (restype, argtypes); must list EVERY symbol include/jslp_engine.h declares
SYMBOLS = {
    "jslp_backend_name": (C.c_char_p, []),
    "jslp_last_error": (C.c_char_p, []),
    "jslp_device_count": (C.c_int, []),
    "jslp_release_pooled_resources": (None, []),
    "jslp_engine_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_double]),
    "jslp_engine_destroy": (None, [C.c_void_p]),
    "jslp_engine_upload": (C.c_int, [C.c_void_p, _f64p, _i32p, _i32p, _i32p, C.c_int32]),
    "jslp_engine_set_optional_objectives": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "jslp_engine_get_optional_objectives": (C.c_int, [C.c_void_p, _f64p, _i32p]),
    "jslp_engine_simplex": (C.c_int, [C.c_void_p, C.c_int, _P(SimplexResult)]),
    "jslp_engine_pivot": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "jslp_engine_save": (C.c_int, [C.c_void_p]),
    "jslp_engine_restore": (C.c_int, [C.c_void_p]),
    "jslp_engine_add_cuts": (C.c_int, [C.c_void_p, C.c_int32, _i8p, _i32p, _f64p]),
    "jslp_engine_relax": (C.c_int, [C.c_void_p, C.c_int32, _i8p, _i32p, _f64p, C.c_int, _P(SimplexResult), _f64p, _i32p]),
    "jslp_engine_relax_batch": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int,
                                          _P(SimplexResult), _f64p, _i32p, C.c_int32]),
    "jslp_engine_relax_batch_pinned": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int,
                                                 _P(SimplexResult), _P(_f64p), _P(_i32p), _i32p]),
    "jslp_engine_state_record_bytes": (C.c_int32, []),
    "jslp_engine_relax_batch_device": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int32]),
    "jslp_engine_results_from_states": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _P(SimplexResult)]),
    "jslp_engine_set_integer_variables": (C.c_int, [C.c_void_p, _i32p, C.c_int32]),
    "jslp_engine_apply_mir_cuts": (C.c_int, [C.c_void_p, _i32p]),
    "jslp_engine_mir_round": (C.c_int, [C.c_void_p, C.c_int, _i32p, _P(SimplexResult), _f64p, _i32p]),
    "jslp_engine_simplex_f32": (C.c_int, [C.c_void_p, C.c_double, C.c_int, _P(SimplexResult), _f64p, _i32p, _f64p]),
    "jslp_engine_checkpoint_create": (C.c_int, [C.c_void_p, _i32p]),
    "jslp_engine_checkpoint_restore": (C.c_int, [C.c_void_p, C.c_int32]),
    "jslp_engine_checkpoint_release": (C.c_int, [C.c_void_p, C.c_int32]),
    "jslp_engine_relax_from": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int,
                                         _P(SimplexResult), _f64p, _i32p, C.c_int32]),
    "jslp_engine_host_matrix": (C.c_int, [C.c_void_p, _P(_f64p), _P(C.c_int64)]),
    "jslp_engine_set_watched_variables": (C.c_int, [C.c_void_p, _i32p, C.c_int32]),
    "jslp_engine_relax_watched": (C.c_int, [C.c_void_p, C.c_int32, _i8p, _i32p, _f64p, C.c_int, _P(SimplexResult), _i32p, _f64p]),
    "jslp_engine_relax_batch_watched": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int, _P(SimplexResult), _i32p, _f64p]),
    "jslp_engine_relax_batch_watched_pinned": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int, _P(SimplexResult), _P(_i32p), _P(_f64p)]),
    "jslp_engine_relax_batch_watched_device": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jslp_engine_watched_count": (C.c_int32, [C.c_void_p]),
    "jslp_engine_set_counting": (C.c_int, [C.c_void_p, C.c_int]),
    "jslp_engine_get_counters": (C.c_int, [C.c_void_p, _P(WorkCounters)]),
    "jslp_pool_create": (C.c_int, [_P(C.c_void_p), C.c_void_p, _i32p, C.c_int32]),
    "jslp_pool_destroy": (None, [C.c_void_p]),
    "jslp_pool_size": (C.c_int, [C.c_void_p]),
    "jslp_pool_sync_root": (C.c_int, [C.c_void_p]),
    "jslp_pool_relax_batch": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int,
                                        _P(SimplexResult), _f64p, _i32p, C.c_int32]),
    "jslp_pool_relax_batch_pinned": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int,
                                               _P(SimplexResult), _P(_f64p), _P(_i32p), _i32p]),
    "jslp_pool_set_watched_variables": (C.c_int, [C.c_void_p, _i32p, C.c_int32]),
    "jslp_pool_relax_batch_watched": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int,
                                                _P(SimplexResult), _i32p, _f64p]),
    "jslp_pool_relax_batch_watched_pinned": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int,
                                                       _P(SimplexResult), _P(_i32p), _P(_f64p)]),
    "jslp_pool_watched_count": (C.c_int32, [C.c_void_p]),
    "jslp_pool_set_counting": (C.c_int, [C.c_void_p, C.c_int]),
    "jslp_pool_get_counters": (C.c_int, [C.c_void_p, _P(WorkCounters)]),
    "jslp_engine_dims": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p]),
    "jslp_engine_read_rhs": (C.c_int, [C.c_void_p, _f64p, _i32p]),
    "jslp_engine_download": (C.c_int, [C.c_void_p, _f64p, _i32p, _i32p, _i32p, _i32p]),
    "jslp_engine_pivot_trace": (C.c_int, [C.c_void_p, _i32p, C.c_int64, _P(C.c_int64)]),
    "jslp_engine_last_path": (C.c_char_p, [C.c_void_p]),
    "jslp_engine_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "jslp_engine_get_timing": (C.c_int, [C.c_void_p, _f64p, _P(C.c_int64), _f64p]),
}


class BranchRecord(C.Structure):
    """struct jslpx_branch_record (include/jslpx_branch.h): a node's outcome as the branch-and-bound tree reads it, 32 bytes"""

    _fields_ = [
        ("flags", C.c_int32),
        ("unbounded_var_index", C.c_int32),
        ("branch_var_index", C.c_int32),
        ("height", C.c_int32),
        ("obj_cell", C.c_double),
        ("branch_var_value", C.c_double),
    ]


BRANCH_FEASIBLE, BRANCH_BOUNDED, BRANCH_OPTIMAL, BRANCH_INTEGRAL = 1, 2, 4, 8
# numpy twin of BranchRecord (the records of a batch as one structured array)
BRANCH_RECORD_DTYPE = np.dtype([(name, np.int32 if ctype is C.c_int32 else np.float64) for name, ctype in BranchRecord._fields_])

# name -> (restype, argtypes); must list EVERY symbol include/jslpx_branch.h declares.  The extension is exported by the HIP library
# only: a Library resolves it when present (Library.has_branch) and the oracle goes without.
BRANCH_SYMBOLS = {
    "jslpx_branch_record_bytes": (C.c_int32, []),
    "jslpx_engine_relax_batch_branch": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int, C.c_void_p]),
    "jslpx_engine_relax_batch_branch_pinned": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int, _P(C.c_void_p)]),
    "jslpx_engine_relax_batch_branch_device": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int, C.c_void_p]),
    "jslpx_engine_results_from_branch_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _P(SimplexResult)]),
}


# name -> (restype, argtypes); must list EVERY symbol include/jslpm_many.h declares.  HIP library only, like BRANCH_SYMBOLS
# (Library.has_many).
MANY_SYMBOLS = {
    "jslpm_simplex_many": (C.c_int, [_P(C.c_void_p), C.c_int32, _i32p, _P(SimplexResult), _i32p]),
}

# name -> (restype, argtypes); must list EVERY symbol include/jslpf_f32.h declares.  HIP library only, like BRANCH_SYMBOLS
# (Library.has_f32).
F32_SYMBOLS = {
    "jslpf_simplex_f32_sweep": (C.c_int, [C.c_void_p, _f64p, C.c_int32, C.c_int, C.c_int32, _P(SimplexResult), _f64p, _i32p, C.c_int32,
                                          _i32p, _i32p, _f64p]),
}
JSLPF_PATH_AUTO, JSLPF_PATH_SELECT_UPDATE, JSLPF_PATH_ONE_LAUNCH = 0, 1, 2
JSLPF_MAX_RUNS = 64


class MirOutcome(C.Structure):
    """struct jslpr_mir_outcome (include/jslpr_mir.h): what the MIR loop of one node did, 32 bytes"""

    _fields_ = [
        ("rounds", C.c_int32),
        ("rows_added", C.c_int32),
        ("optimal_count", C.c_int32),
        ("pivots", C.c_int32),
        ("volume_before", C.c_double),
        ("volume_after", C.c_double),
    ]


MIR_OUTCOME_DTYPE = np.dtype([(name, np.int32 if ctype is C.c_int32 else np.float64) for name, ctype in MirOutcome._fields_])
JSLPR_MAX_ROUNDS = 64

# name -> (restype, argtypes); must list EVERY symbol include/jslpr_mir.h declares.  HIP library only, like BRANCH_SYMBOLS
# (Library.has_mir).
MIR_SYMBOLS = {
    "jslpr_mir_outcome_bytes": (C.c_int32, []),
    "jslpr_engine_relax_mir": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i32p, _i8p, _i32p, _f64p, C.c_int, C.c_int32, C.c_int32,
                                         _P(SimplexResult), C.c_void_p, _f64p, _i32p, C.c_int32]),
}


# numpy twin of SimplexResult: the results of a pack as one structured array (no per-LP ctypes struct)
RESULT_DTYPE = np.dtype([(name, np.int32 if ctype is C.c_int32 else np.float64) for name, ctype in SimplexResult._fields_])
assert RESULT_DTYPE.itemsize == C.sizeof(SimplexResult)

# name -> (restype, argtypes); must list EVERY symbol include/jslpp_packed.h declares.  HIP library only, like BRANCH_SYMBOLS
# (Library.has_pack).
PACK_SYMBOLS = {
    "jslpp_lds_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "jslpp_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, C.c_int32, C.c_int32]),
    "jslpp_pack_destroy": (None, [C.c_void_p]),
    "jslpp_pack_size": (C.c_int32, [C.c_void_p]),
    "jslpp_pack_host_matrix": (C.c_int, [C.c_void_p, C.c_int32, _P(_f64p), _P(C.c_int64)]),
    "jslpp_pack_set": (C.c_int, [C.c_void_p, C.c_int32, _f64p, _i32p, _i32p, _i32p, C.c_int32]),
    "jslpp_pack_upload": (C.c_int, [C.c_void_p]),
    "jslpp_pack_simplex": (C.c_int, [C.c_void_p, _i32p, C.c_void_p, _i32p, _f64p]),
    "jslpp_pack_launches": (C.c_int32, [C.c_void_p]),
    "jslpp_pack_read_rhs": (C.c_int, [C.c_void_p, _P(_f64p), _P(_i32p), _P(_P(C.c_int64))]),
    "jslpp_pack_download": (C.c_int, [C.c_void_p, C.c_int32, _f64p, _i32p, _i32p, _i32p, _i32p]),
    "jslpp_pack_pivot_trace": (C.c_int, [C.c_void_p, C.c_int32, _i32p, C.c_int64, _P(C.c_int64)]),
}
JSLPP_LDS_LIMIT = 65536

# name -> (restype, argtypes); must list EVERY symbol include/jslpt_tree.h declares.  HIP library only (Library.has_tree).
TREE_SYMBOLS = {
    "jslpt_lds_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "jslpt_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, C.c_int32, C.c_int32, C.c_int32]),
    "jslpt_pack_set_integers": (C.c_int, [C.c_void_p, C.c_int32, _i32p, C.c_int32]),
    "jslpt_pack_branch_and_cut": (C.c_int, [C.c_void_p, _i32p, C.c_void_p, C.c_void_p, _i32p, _f64p]),
    "jslpt_pack_read_rhs": (C.c_int, [C.c_void_p, _P(_f64p), _P(_i32p), _P(_P(C.c_int64))]),
}
# name -> (restype, argtypes); must list EVERY symbol include/jslps_soft.h declares.  HIP library only (Library.has_soft).
SOFT_SYMBOLS = {
    "jslps_lds_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "jslps_tree_lds_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "jslps_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, C.c_int32, C.c_int32]),
    "jslps_tree_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, C.c_int32, C.c_int32,
                                         C.c_int32]),
    "jslps_pack_set_optional_objectives": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "jslps_pack_get_optional_objectives": (C.c_int, [C.c_void_p, C.c_int32, _f64p, _i32p]),
}
# name -> (restype, argtypes); must list EVERY symbol include/jslpc_tree_mir.h declares.  HIP library only (Library.has_tree_mir).
TREE_MIR_SYMBOLS = {
    "jslpc_tree_lds_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "jslpc_tree_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, C.c_int32, C.c_int32,
                                         C.c_int32]),
    "jslpc_pack_read_mir": (C.c_int, [C.c_void_p, C.c_void_p]),
}
# name -> (restype, argtypes); must list EVERY symbol include/jslpe_tree_enhanced.h declares.  HIP library only (Library.has_tree_enh).
TREE_ENH_SYMBOLS = {
    "jslpe_tree_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _i32p, C.c_int32, C.c_int32,
                                         C.c_int32]),
    "jslpe_tree_pack_create_mixed": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p,
                                               C.c_int32, C.c_int32, C.c_int32]),
    "jslpe_pack_read_enhanced": (C.c_int, [C.c_void_p, C.c_void_p]),
}
# name -> (restype, argtypes); must list EVERY symbol include/jslpi_tree_incremental.h declares.  HIP library only (Library.has_tree_inc).
TREE_INC_SYMBOLS = {
    "jslpi_tree_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p,
                                         C.c_int32, C.c_int32, C.c_int32]),
    "jslpi_tree_lds_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "jslpi_checkpoint_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "jslpi_pack_read_incremental": (C.c_int, [C.c_void_p, C.c_void_p]),
}
# name -> (restype, argtypes); must list EVERY symbol include/jslpg_tree_tolerance.h declares.  HIP library only (Library.has_tree_tol).
TREE_TOL_SYMBOLS = {
    "jslpg_tree_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p,
                                         _f64p, _i32p, C.c_int32, C.c_int32, C.c_int32]),
    "jslpg_pack_read_tolerance": (C.c_int, [C.c_void_p, C.c_void_p]),
}
# name -> (restype, argtypes); must list EVERY symbol include/jslpb_big_lds.h declares.  HIP library only (Library.has_big_lds).
BIG_SYMBOLS = {
    "jslpb_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, C.c_int32, C.c_int32, C.c_int32]),
    "jslpb_tree_pack_create": (C.c_int, [_P(C.c_void_p), C.c_int, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p,
                                         _f64p, _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "jslpb_pack_big_threads": (C.c_int32, []),
}
JSLPB_LDS_LIMIT = 159744
# numpy twin of struct jslpg_tolerance_result
TOL_TREE_DTYPE = np.dtype([("best_possible", np.float64), ("threshold", np.float64), ("stopped", np.int32), ("left", np.int32),
                           ("reserved0", np.int32), ("reserved1", np.int32)])
# numpy twin of struct jslpi_tree_result
INC_TREE_DTYPE = np.dtype([(name, np.int32) for name in ("checkpoints_used", "incremental_nodes", "rows_high_water", "checkpoint_rows_high_water",
                                                         "reserved0", "reserved1", "reserved2", "reserved3")])
JSLPI_MAX_CHECKPOINTS = 64
JSLPI_CHECKPOINTS_DEFAULT = 50
# numpy twin of struct jslpe_tree_result
ENH_TREE_DTYPE = np.dtype([(name, np.int32) for name in ("solutions_found", "stack_high_water", "moved_to_heap", "pseudo_updates",
                                                         "scored_by_pseudocost", "dropped_nodes", "reserved0", "reserved1")])
# node_selection / branching of jslpe_tree_pack_create (0: the default service)
ENH_NODE_SELECTION = {"best-first": 1, "depth-first": 2, "hybrid": 3}
ENH_BRANCHING = {"most-fractional": 1, "pseudocost": 2, "strong": 3}
# numpy twin of struct jslpc_mir_result
MIR_TREE_DTYPE = np.dtype([(name, np.int32) for name in ("rounds", "rows_added", "simplexes", "root_rows", "rows_high_water")])
# numpy twin of struct jslpt_tree_result
TREE_DTYPE = np.dtype([(name, np.int32) for name in ("iterations", "is_integral", "final_height", "nodes_pushed", "heap_high_water",
                                                     "cuts_high_water")])
JSLPT_MAX_NODES_DEFAULT = 1000000


class EngineError(RuntimeError):
    pass


class Library:
    """A loaded engine library with typed entry points."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise EngineError("engine library not found: %s" % path)
        self.path = path
        self.dll = C.CDLL(path, mode=getattr(os, "RTLD_LOCAL", 0) | getattr(os, "RTLD_NOW", 2))
        for name, (restype, argtypes) in SYMBOLS.items():
            fn = getattr(self.dll, name)  # AttributeError => the library does not export the ABI
            fn.restype = restype
            fn.argtypes = argtypes
            setattr(self, name, fn)
        self.has_branch = self._bind_extension(BRANCH_SYMBOLS)
        self.has_many = self._bind_extension(MANY_SYMBOLS)
        self.has_f32 = self._bind_extension(F32_SYMBOLS)
        self.has_mir = self._bind_extension(MIR_SYMBOLS)
        self.has_pack = self._bind_extension(PACK_SYMBOLS)
        self.has_tree = self.has_pack and self._bind_extension(TREE_SYMBOLS)
        self.has_soft = self.has_tree and self._bind_extension(SOFT_SYMBOLS)
        self.has_tree_mir = self.has_tree and self._bind_extension(TREE_MIR_SYMBOLS)
        self.has_tree_enh = self.has_tree_mir and self.has_soft and self._bind_extension(TREE_ENH_SYMBOLS)
        self.has_tree_inc = self.has_tree_enh and self._bind_extension(TREE_INC_SYMBOLS)
        self.has_tree_tol = self.has_tree_inc and self._bind_extension(TREE_TOL_SYMBOLS)
        self.has_big_lds = self.has_tree_tol and self._bind_extension(BIG_SYMBOLS)

    def _bind_extension(self, symbols):
        """bind a HIP-only extension when the library exports all of it; False otherwise"""
        if not all(hasattr(self.dll, name) for name in symbols):
            return False
        for name, (restype, argtypes) in symbols.items():
            fn = getattr(self.dll, name)
            fn.restype = restype
            fn.argtypes = argtypes
            setattr(self, name, fn)
        return True

    @property
    def backend(self):
        return self.jslp_backend_name().decode()

    def check(self, rc, what):
        if rc != JSLP_OK:
            raise EngineError("%s failed (%d): %s" % (what, rc, self.jslp_last_error().decode()))


_hip = None


def load_hip():
    """The product's only loader.  Fails loudly: no HIP library, no engine."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise EngineError(
                "jslpsolver_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % HIP_LIB_PATH)
        _hip = Library(HIP_LIB_PATH)
    return _hip


def as_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def ptr_i32(a):
    return a.ctypes.data_as(_i32p) if a is not None else None


def ptr_f64(a):
    return a.ctypes.data_as(_f64p) if a is not None else None


def ptr_i8(a):
    return a.ctypes.data_as(_i8p) if a is not None else None
