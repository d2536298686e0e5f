"""Host-side mirror of the reference `Tableau` hot-path methods (src/tableau/tableau.ts:103-229) on top of
the C ABI.  Method names follow the reference: simplex / pivot / save / restore / addCutConstraints /
applyCuts, so parity tests read like the reference's own tests.
"""
import math

import numpy as np

from . import _capi
from ._capi import SimplexResult


class PackedCuts(tuple):
    """(n_nodes, cut_offsets, type, var_index, value) as Tableau.pack_cut_lists returns it -- a plain 5-tuple to every caller -- that also keeps the four
    ctypes pointers of its arrays: `a.ctypes.data_as(...)` costs ~2 us per array, four times per call, which is a fifth of a 40 us single-node batch."""

    def ptrs(self):
        p = self.__dict__.get("_ptrs")
        if p is None:
            _, offs, t, v, x = self
            p = self.__dict__["_ptrs"] = (_capi.ptr_i32(offs), _capi.ptr_i8(t), _capi.ptr_i32(v), _capi.ptr_f64(x))
        return p


def _cut_ptrs(packed):
    f = getattr(packed, "ptrs", None)
    if f is not None:
        return f()
    _, offs, t, v, x = packed
    return _capi.ptr_i32(offs), _capi.ptr_i8(t), _capi.ptr_i32(v), _capi.ptr_f64(x)


_VIEWS = {}


def _pinned_view(ptr, shape):
    """numpy view of an engine-owned pinned buffer (np.ctypeslib.as_array costs ~2 us a time): one view object per (address, shape, type) -- the
    engine hands out the same buffer call after call; a re-allocated buffer has another address and gets another view"""
    key = (_capi.C.cast(ptr, _capi.C.c_void_p).value, shape, ptr._type_)
    if key[0] is None:  # a call without nodes hands out no buffer
        return np.empty((0,) + tuple(shape[1:]), dtype=np.dtype(ptr._type_))
    v = _VIEWS.get(key)
    if v is None:
        if len(_VIEWS) > 256:
            _VIEWS.clear()
        v = _VIEWS[key] = np.ctypeslib.as_array(ptr, shape=shape)
    return v


class Tableau:
    """Device-resident dense simplex tableau (one `jslp_engine`).

    matrix is the reference layout (tableau.ts:49-54): row-major height x width float64, row 0 = reduced
    costs, column 0 = RHS.
    """

    def __init__(self, matrix, var_index_by_row, var_index_by_col, unrestricted=(), precision=1e-8,
                 row_capacity=None, device=0, lib=None, optional_objectives=None, integer_variables=None):
        self.lib = lib if lib is not None else _capi.load_hip()
        matrix = _capi.as_f64(matrix)
        if matrix.ndim != 2:
            raise ValueError("matrix must be height x width")
        self.height0, self.width = matrix.shape
        self.precision = float(precision)
        self.row_capacity = int(row_capacity if row_capacity is not None else self.height0)
        self._h = _capi.C.c_void_p()
        self.lib.check(self.lib.jslp_engine_create(_capi.C.byref(self._h), int(device), self.height0, self.width,
                                                   self.row_capacity, self.precision), "jslp_engine_create")
        vibr = _capi.as_i32(var_index_by_row)
        vibc = _capi.as_i32(var_index_by_col)
        unr = _capi.as_i32(list(unrestricted))
        if vibr.shape[0] != self.height0 or vibc.shape[0] != self.width:
            raise ValueError("index maps do not match the matrix shape")
        self.lib.check(self.lib.jslp_engine_upload(self._h, _capi.ptr_f64(matrix), _capi.ptr_i32(vibr),
                                                   _capi.ptr_i32(vibc), _capi.ptr_i32(unr), int(unr.shape[0])),
                       "jslp_engine_upload")
        self.n_optional = 0
        if optional_objectives is not None and len(optional_objectives) > 0:
            oo = _capi.as_f64(optional_objectives)
            if oo.ndim != 2 or oo.shape[1] != self.width:
                raise ValueError("optional objectives must be n x width")
            self.lib.check(self.lib.jslp_engine_set_optional_objectives(self._h, int(oo.shape[0]), _capi.ptr_f64(oo)),
                           "jslp_engine_set_optional_objectives")
            self.n_optional = int(oo.shape[0])
        self.integer_variables = frozenset(int(i) for i in integer_variables) if integer_variables is not None else frozenset()
        if integer_variables is not None and len(integer_variables) > 0:  # variable.isInteger for the MIR cuts
            iv = _capi.as_i32(list(integer_variables))
            self.lib.check(self.lib.jslp_engine_set_integer_variables(self._h, _capi.ptr_i32(iv), int(iv.shape[0])),
                           "jslp_engine_set_integer_variables")
        # tableau scalars the reference keeps on the Tableau object (tableau.ts:59-61,83-87)
        self.feasible = True
        self.bounded = True
        self.evaluation = 0.0
        self.simplexIters = 0
        self.bestPossibleEval = 0.0
        self.unboundedVarIndex = None
        self.last = None

    # ---- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.jslp_engine_destroy(self._h)
            self._h = _capi.C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference Tableau surface ------------------------------------------------------------
    @property
    def height(self):
        h = _capi.C.c_int32()
        self.lib.check(self.lib.jslp_engine_dims(self._h, _capi.C.byref(h), None, None), "jslp_engine_dims")
        return h.value

    def _absorb(self, res):
        """fold a jslp_simplex_result into the Tableau scalars exactly as simplex.ts/tableau.ts do"""
        self.last = res
        self.feasible = bool(res.feasible)
        self.bounded = bool(res.bounded)
        if res.optimal:  # setEvaluation + simplexIters += 1 (simplex.ts:265-269, tableau.ts:420-430)
            self.evaluation = res.evaluation
            if self.simplexIters == 0:
                self.bestPossibleEval = res.evaluation
            self.simplexIters += 1
        elif not res.bounded:  # simplex.ts:298-303
            self.evaluation = float("-inf")
            self.unboundedVarIndex = res.unbounded_var_index
        return res

    def simplex(self, check_cycles=True):
        res = SimplexResult()
        self.lib.check(self.lib.jslp_engine_simplex(self._h, int(bool(check_cycles)), _capi.C.byref(res)),
                       "jslp_engine_simplex")
        return self._absorb(res)

    def pivot(self, row, col):
        self.lib.check(self.lib.jslp_engine_pivot(self._h, int(row), int(col)), "jslp_engine_pivot")

    def save(self):
        self.lib.check(self.lib.jslp_engine_save(self._h), "jslp_engine_save")

    def restore(self):
        self.lib.check(self.lib.jslp_engine_restore(self._h), "jslp_engine_restore")

    @staticmethod
    def _pack_cuts(cuts):
        n = len(cuts)
        t = np.array([_capi.JSLP_CUT_MIN if c["type"] == "min" else _capi.JSLP_CUT_MAX for c in cuts], dtype=np.int8)
        v = np.array([c["varIndex"] for c in cuts], dtype=np.int32)
        x = np.array([c["value"] for c in cuts], dtype=np.float64)
        return n, t, v, x

    def addCutConstraints(self, cuts):
        n, t, v, x = self._pack_cuts(cuts)
        self.lib.check(self.lib.jslp_engine_add_cuts(self._h, n, _capi.ptr_i8(t), _capi.ptr_i32(v), _capi.ptr_f64(x)),
                       "jslp_engine_add_cuts")

    def applyCuts(self, cuts, check_cycles=True):
        """BranchAndCutService.applyCuts (branch-and-cut.ts:33-37) as ONE engine call; returns (result, rhs,
        varIndexByRow) -- the read-back isIntegral()/getMostFractionalVar() need."""
        n, t, v, x = self._pack_cuts(cuts)
        res = SimplexResult()
        rhs = np.empty(self.row_capacity, dtype=np.float64)
        vibr = np.empty(self.row_capacity, dtype=np.int32)
        self.lib.check(self.lib.jslp_engine_relax(self._h, n, _capi.ptr_i8(t), _capi.ptr_i32(v), _capi.ptr_f64(x),
                                                  int(bool(check_cycles)), _capi.C.byref(res), _capi.ptr_f64(rhs),
                                                  _capi.ptr_i32(vibr)), "jslp_engine_relax")
        self._absorb(res)
        return res, rhs[:res.height], vibr[:res.height]

    def pack_cut_lists(self, cut_lists):
        """cut lists -> the flat arrays jslp_engine_relax_batch takes (do this once when the same nodes are re-evaluated)"""
        n_nodes = len(cut_lists)
        offs = np.zeros(n_nodes + 1, dtype=np.int32)
        flat = []
        for i, cuts in enumerate(cut_lists):
            flat.extend(cuts)
            offs[i + 1] = len(flat)
        _, t, v, x = self._pack_cuts(flat)
        return PackedCuts((n_nodes, offs, t, v, x))

    def applyCutsBatch(self, cut_lists, check_cycles=True, packed=None, want_rows=True, copy=True):
        """Independent branch-and-bound nodes in one call.  copy=False returns views of the engine's pinned read-back
        buffer (jslp_engine_relax_batch_pinned): valid until the next call on this tableau."""
        pk = packed if packed is not None else self.pack_cut_lists(cut_lists)
        n_nodes, offs, t, v, x = pk
        out = (SimplexResult * max(n_nodes, 1))()
        stride = self.row_capacity
        if copy:
            rhs = np.empty((max(n_nodes, 1), stride), dtype=np.float64)
            vibr = np.empty((max(n_nodes, 1), stride), dtype=np.int32) if want_rows else None
            self.lib.check(self.lib.jslp_engine_relax_batch(self._h, n_nodes, _capi.ptr_i32(offs), _capi.ptr_i8(t),
                                                            _capi.ptr_i32(v), _capi.ptr_f64(x), int(bool(check_cycles)),
                                                            out, _capi.ptr_f64(rhs), _capi.ptr_i32(vibr), stride),
                           "jslp_engine_relax_batch")
            return [out[i] for i in range(n_nodes)], rhs, vibr
        p_rhs = _capi._f64p()
        p_rows = _capi._i32p()
        c_stride = _capi.C.c_int32()
        self.lib.check(self.lib.jslp_engine_relax_batch_pinned(
            self._h, n_nodes, *_cut_ptrs(pk),
            int(bool(check_cycles)), out, _capi.C.byref(p_rhs), _capi.C.byref(p_rows) if want_rows else None,
            _capi.C.byref(c_stride)), "jslp_engine_relax_batch_pinned")
        shape = (max(n_nodes, 1), c_stride.value)
        rhs = _pinned_view(p_rhs, shape)
        vibr = _pinned_view(p_rows, shape) if want_rows else None
        return out, rhs, vibr

    # ---- outcomes left in device memory (the one-process-per-GPU path: sharding.py) ----------------------------------
    def state_record_bytes(self):
        return int(self.lib.jslp_engine_state_record_bytes())

    def applyCutsBatchDevice(self, packed, check_cycles, states_ptr, rhs_ptr, rows_ptr, row_stride):
        """jslp_engine_relax_batch_device: raw addresses of memory on the engine's device (torch tensors' data_ptr(); plain host
        memory for the oracle library) receive the per-node state records, RHS columns and row maps; nothing is copied back"""
        n_nodes = packed[0]
        self.lib.check(self.lib.jslp_engine_relax_batch_device(
            self._h, n_nodes, *_cut_ptrs(packed), int(bool(check_cycles)),
            _capi.C.c_void_p(states_ptr), _capi.C.c_void_p(rhs_ptr), _capi.C.c_void_p(rows_ptr), int(row_stride)),
            "jslp_engine_relax_batch_device")

    def applyCutsBatchWatchedDevice(self, packed, check_cycles, states_ptr, rows_ptr, values_ptr):
        """jslp_engine_relax_batch_watched_device: the COMPACT outcome (state record + row / RHS cell of the watched variables per node)
        left in memory of the engine's device -- the exchange payload of the multi-process path (sharding.py)"""
        n_nodes = packed[0]
        self.lib.check(self.lib.jslp_engine_relax_batch_watched_device(
            self._h, n_nodes, *_cut_ptrs(packed), int(bool(check_cycles)),
            _capi.C.c_void_p(states_ptr), _capi.C.c_void_p(rows_ptr), _capi.C.c_void_p(values_ptr)),
            "jslp_engine_relax_batch_watched_device")

    def watched_count(self):
        """how many variables set_watched_variables registered on the engine (jslp_engine_watched_count)"""
        return int(self.lib.jslp_engine_watched_count(self._h))

    def results_from_states(self, states_u8, n_nodes):
        """raw state records (host bytes: this rank's or, after the exchange, another rank's) -> SimplexResult array"""
        out = (SimplexResult * max(n_nodes, 1))()
        buf = np.ascontiguousarray(states_u8, dtype=np.uint8)
        self.lib.check(self.lib.jslp_engine_results_from_states(self._h, _capi.C.c_void_p(buf.ctypes.data), int(n_nodes), out),
                       "jslp_engine_results_from_states")
        return out

    # ---- branch records (include/jslpx_branch.h): isIntegral() / getMostFractionalVar() of every node, 32 bytes per node ----------
    def _branch_native(self, what):
        """True: the library computes the records (HIP, jslpx_* exported); False: the oracle, whose records are restated here from its
        compact read-back (branch_record_from_watched).  A HIP library without the extension is an error, never a fallback."""
        if self.lib.has_branch:
            return True
        if self.lib.backend == "oracle-c":
            if self.watched_count() <= 0:
                raise _capi.EngineError("%s failed (%d): relax_batch_branch: after set_watched_variables" % (what, _capi.JSLP_ERR_ARG))
            return False
        raise _capi.EngineError("%s: %s does not export the branch-record extension (include/jslpx_branch.h)" % (what, self.lib.path))

    def _branch_restated(self, pk, check_cycles):
        """the oracle's records: its compact read-back of the same call, restated"""
        results, wrows, wvals = self.applyCutsBatchWatched(None, check_cycles=check_cycles, packed=pk)
        n = pk[0]
        res = [results[i] for i in range(n)]
        # the evaluation a node without an optimum keeps (fill_result): what the call started from
        self._branch_prev = next((r.evaluation for r in res if not r.optimal and r.bounded), self.evaluation)
        return branch_record_from_watched(res, wrows[:n], wvals[:n], self.watched, self.precision)

    def applyCutsBatchBranch(self, cut_lists, check_cycles=True, packed=None, copy=True):
        """Independent branch-and-bound nodes in one call whose read-back is the BRANCH RECORD of each node (flags, height, raw objective
        cell, isIntegral() and getMostFractionalVar() over the watched variables).  Returns (results, records): SimplexResult per node as
        results_from_branch_records derives it (no pivot counts) and the records as a numpy structured array (_capi.BRANCH_RECORD_DTYPE).
        copy=False: the records are a view of the engine's pinned buffer, valid until the next call on this tableau."""
        pk = packed if packed is not None else self.pack_cut_lists(cut_lists)
        n_nodes = pk[0]
        if not self._branch_native("applyCutsBatchBranch"):
            recs = self._branch_restated(pk, check_cycles)
            return self.results_from_branch_records(recs, n_nodes), recs
        if copy:
            recs = np.zeros(max(n_nodes, 1), dtype=_capi.BRANCH_RECORD_DTYPE)
            self.lib.check(self.lib.jslpx_engine_relax_batch_branch(self._h, n_nodes, *_cut_ptrs(pk), int(bool(check_cycles)),
                                                                     _capi.C.c_void_p(recs.ctypes.data)), "jslpx_engine_relax_batch_branch")
            recs = recs[:n_nodes]
        else:
            p = _capi.C.c_void_p()
            self.lib.check(self.lib.jslpx_engine_relax_batch_branch_pinned(self._h, n_nodes, *_cut_ptrs(pk), int(bool(check_cycles)),
                                                                            _capi.C.byref(p)), "jslpx_engine_relax_batch_branch_pinned")
            recs = np.zeros(0, dtype=_capi.BRANCH_RECORD_DTYPE)
            if n_nodes > 0:
                buf = (_capi.C.c_char * (n_nodes * _capi.BRANCH_RECORD_DTYPE.itemsize)).from_address(p.value)
                recs = np.frombuffer(buf, dtype=_capi.BRANCH_RECORD_DTYPE, count=n_nodes)
        return self.results_from_branch_records(recs, n_nodes), recs

    def applyCutsBatchBranchDevice(self, packed, check_cycles, records_ptr):
        """jslpx_engine_relax_batch_branch_device: the records (32 bytes per node) left at `records_ptr`, memory of the engine's device
        (a torch tensor's data_ptr(); host memory for the oracle, whose records are restated here); nothing else is copied back"""
        if not self._branch_native("applyCutsBatchBranchDevice"):
            recs = self._branch_restated(packed, check_cycles)
            _capi.C.memmove(int(records_ptr), recs.ctypes.data, recs.nbytes)
            return
        self.lib.check(self.lib.jslpx_engine_relax_batch_branch_device(self._h, packed[0], *_cut_ptrs(packed), int(bool(check_cycles)),
                                                                        _capi.C.c_void_p(records_ptr)), "jslpx_engine_relax_batch_branch_device")

    def results_from_branch_records(self, records, n_nodes):
        """branch records (host bytes or a structured array: this rank's or, after the exchange, another rank's) -> SimplexResult array,
        evaluation as every other entry point derives it; pivot counts 0"""
        out = (SimplexResult * max(n_nodes, 1))()
        buf = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
        if buf.size < n_nodes * _capi.BRANCH_RECORD_DTYPE.itemsize:
            raise ValueError("results_from_branch_records: %d bytes for %d records" % (buf.size, n_nodes))
        if self.lib.has_branch:
            self.lib.check(self.lib.jslpx_engine_results_from_branch_records(self._h, _capi.C.c_void_p(buf.ctypes.data), int(n_nodes), out),
                           "jslpx_engine_results_from_branch_records")
            return out
        self._branch_native("results_from_branch_records")
        recs = buf[:n_nodes * _capi.BRANCH_RECORD_DTYPE.itemsize].view(_capi.BRANCH_RECORD_DTYPE)
        rc = _js_round(1.0 / self.precision)
        prev = getattr(self, "_branch_prev", self.evaluation)
        for i in range(n_nodes):
            f = int(recs["flags"][i])
            r = out[i]
            r.feasible, r.bounded, r.optimal = int(bool(f & _capi.BRANCH_FEASIBLE)), int(bool(f & _capi.BRANCH_BOUNDED)), int(bool(f & _capi.BRANCH_OPTIMAL))
            r.unbounded_var_index = int(recs["unbounded_var_index"][i])
            r.height = int(recs["height"][i])
            r.obj_cell = float(recs["obj_cell"][i])
            r.evaluation = (_js_round((_EPSILON + r.obj_cell) * rc) / rc if r.optimal else (float("-inf") if not r.bounded else prev))
        return out

    # ---- compact read-back, work counters, pinned host build --------------------------------------------------
    def set_watched_variables(self, var_indexes):
        """the variable indexes the branch-and-bound tree reads between relaxations (the integer variables)"""
        w = _capi.as_i32(list(var_indexes))
        self.lib.check(self.lib.jslp_engine_set_watched_variables(self._h, _capi.ptr_i32(w), int(w.shape[0])),
                       "jslp_engine_set_watched_variables")
        self.n_watched = int(w.shape[0])
        self.watched = [int(i) for i in w]  # (what is registered: a caller that borrows the registration puts it back)

    def applyCutsWatched(self, cuts, check_cycles=True):
        """applyCuts whose read-back is only rowByVarIndex / the RHS cell of the watched variables"""
        n, t, v, x = self._pack_cuts(cuts)
        res = SimplexResult()
        rows = np.empty(self.n_watched, dtype=np.int32)
        vals = np.empty(self.n_watched, dtype=np.float64)
        self.lib.check(self.lib.jslp_engine_relax_watched(self._h, n, _capi.ptr_i8(t), _capi.ptr_i32(v), _capi.ptr_f64(x),
                                                          int(bool(check_cycles)), _capi.C.byref(res), _capi.ptr_i32(rows),
                                                          _capi.ptr_f64(vals)), "jslp_engine_relax_watched")
        self._absorb(res)
        return res, rows, vals

    def applyCutsBatchWatched(self, cut_lists, check_cycles=True, packed=None, copy=True):
        """applyCutsBatch whose read-back is, per node, rowByVarIndex / the RHS cell of the watched variables only: what a host
        that walks the tree itself reads per node, and ~10x fewer bytes over PCIe than the full RHS columns + row maps.
        copy=False returns views of the engine's pinned buffer (valid until the next call on this tableau)."""
        pk = packed if packed is not None else self.pack_cut_lists(cut_lists)
        n_nodes, offs, t, v, x = pk
        out = (SimplexResult * max(n_nodes, 1))()
        if not copy:
            p_rows = _capi._i32p()
            p_vals = _capi._f64p()
            self.lib.check(self.lib.jslp_engine_relax_batch_watched_pinned(
                self._h, n_nodes, *_cut_ptrs(pk), int(bool(check_cycles)), out,
                _capi.C.byref(p_rows), _capi.C.byref(p_vals)), "jslp_engine_relax_batch_watched_pinned")
            shape = (max(n_nodes, 1), self.n_watched)
            return out, _pinned_view(p_rows, shape), _pinned_view(p_vals, shape)
        rows = np.empty((max(n_nodes, 1), self.n_watched), dtype=np.int32)
        vals = np.empty((max(n_nodes, 1), self.n_watched), dtype=np.float64)
        self.lib.check(self.lib.jslp_engine_relax_batch_watched(self._h, n_nodes, _capi.ptr_i32(offs), _capi.ptr_i8(t), _capi.ptr_i32(v),
                                                                _capi.ptr_f64(x), int(bool(check_cycles)), out, _capi.ptr_i32(rows),
                                                                _capi.ptr_f64(vals)), "jslp_engine_relax_batch_watched")
        return out, rows, vals

    def set_counting(self, enabled):
        self.lib.check(self.lib.jslp_engine_set_counting(self._h, int(bool(enabled))), "jslp_engine_set_counting")

    def get_counters(self):
        c = _capi.WorkCounters()
        self.lib.check(self.lib.jslp_engine_get_counters(self._h, _capi.C.byref(c)), "jslp_engine_get_counters")
        return c.as_dict()

    def host_matrix(self):
        """height x width float64 view of the engine's pinned build buffer (zero-filled on every call); fill it and pass
        it to upload_host_matrix()"""
        p = _capi._f64p()
        n = _capi.C.c_int64()
        self.lib.check(self.lib.jslp_engine_host_matrix(self._h, _capi.C.byref(p), _capi.C.byref(n)), "jslp_engine_host_matrix")
        return np.ctypeslib.as_array(p, shape=(self.height0, self.width))

    def upload(self, matrix, var_index_by_row, var_index_by_col, unrestricted=()):
        """Tableau hand-over again (a new model of the same shape, or the buffer of host_matrix())"""
        vibr = _capi.as_i32(var_index_by_row)
        vibc = _capi.as_i32(var_index_by_col)
        unr = _capi.as_i32(list(unrestricted))
        m = np.ascontiguousarray(matrix, dtype=np.float64)
        self.lib.check(self.lib.jslp_engine_upload(self._h, _capi.ptr_f64(m), _capi.ptr_i32(vibr), _capi.ptr_i32(vibc),
                                                   _capi.ptr_i32(unr), int(unr.shape[0])), "jslp_engine_upload")

    # ---- fp32 experiment ------------------------------------------------------------------------------------
    def simplex_f32(self, precision, check_cycles=True):
        """simplex() on an fp32 copy of the live tableau with tolerance `precision` (SURVEY.md 8d, config 5's fp32-vs-fp64
        sweep).  The fp64 tableau and the Tableau scalars are left alone.  Returns (result, rhs, varIndexByRow, device ms)."""
        res = SimplexResult()
        rhs = np.empty(self.row_capacity, dtype=np.float64)
        vibr = np.empty(self.row_capacity, dtype=np.int32)
        ms = _capi.C.c_double(0.0)
        self.lib.check(self.lib.jslp_engine_simplex_f32(self._h, float(precision), int(bool(check_cycles)), _capi.C.byref(res),
                                                        _capi.ptr_f64(rhs), _capi.ptr_i32(vibr), _capi.C.byref(ms)),
                       "jslp_engine_simplex_f32")
        return res, rhs[:res.height], vibr[:res.height], ms.value

    F32_PATHS = {"auto": _capi.JSLPF_PATH_AUTO, "select_update": _capi.JSLPF_PATH_SELECT_UPDATE, "one_launch": _capi.JSLPF_PATH_ONE_LAUNCH}

    def simplex_f32_sweep(self, precisions, check_cycles=True, path="auto"):
        """simplex_f32 at every tolerance of `precisions` in one call (include/jslpf_f32.h): path "one_launch" solves them in ONE kernel
        launch, one workgroup per tolerance; "select_update" is the loop of simplex_f32, one run after the other; "auto" picks.
        Returns (runs, path_taken, device ms of the call) with runs[i] = (result, rhs, varIndexByRow) -- what simplex_f32(precisions[i])
        returns.  A run that ends on an error of its own (iteration cap ...) raises, naming the run."""
        if not self.lib.has_f32:
            raise _capi.EngineError("simplex_f32_sweep: %s does not export the fp32 sweep extension (include/jslpf_f32.h)" % self.lib.path)
        if path not in self.F32_PATHS:
            raise ValueError("simplex_f32_sweep: path must be one of %s" % ", ".join(sorted(self.F32_PATHS)))
        prec = _capi.as_f64(list(precisions))
        n = int(prec.shape[0])
        out = (SimplexResult * max(n, 1))()
        stride = self.row_capacity
        rhs = np.empty((max(n, 1), stride), dtype=np.float64)
        vibr = np.empty((max(n, 1), stride), dtype=np.int32)
        taken = _capi.C.c_int32(0)
        ms = _capi.C.c_double(0.0)
        self.lib.check(self.lib.jslpf_simplex_f32_sweep(self._h, _capi.ptr_f64(prec), n, int(bool(check_cycles)), self.F32_PATHS[path], out,
                                                        _capi.ptr_f64(rhs), _capi.ptr_i32(vibr), stride, None, _capi.C.byref(taken),
                                                        _capi.C.byref(ms)), "jslpf_simplex_f32_sweep")
        runs = []
        for i in range(n):
            res = SimplexResult.from_buffer_copy(out[i])
            runs.append((res, rhs[i, :res.height].copy(), vibr[i, :res.height].copy()))
        return runs, taken.value, ms.value

    # ---- MIR cuts (cutting-strategies.ts:74-212) --------------------------------------------------------
    def applyMIRCuts(self):
        """Tableau.applyMIRCuts (:199-212); returns the number of rows appended"""
        n = _capi.C.c_int32(0)
        self.lib.check(self.lib.jslp_engine_apply_mir_cuts(self._h, _capi.C.byref(n)), "jslp_engine_apply_mir_cuts")
        return n.value

    def mirRound(self, check_cycles=True):
        """one turn of the services' MIR loop (branch-and-cut.ts:41-43): applyMIRCuts + simplex + read-back.
        Returns (rows appended, result, rhs, varIndexByRow)."""
        n = _capi.C.c_int32(0)
        res = SimplexResult()
        rhs = np.empty(self.row_capacity, dtype=np.float64)
        vibr = np.empty(self.row_capacity, dtype=np.int32)
        self.lib.check(self.lib.jslp_engine_mir_round(self._h, int(bool(check_cycles)), _capi.C.byref(n), _capi.C.byref(res),
                                                      _capi.ptr_f64(rhs), _capi.ptr_i32(vibr)), "jslp_engine_mir_round")
        self._absorb(res)
        return n.value, res, rhs[:res.height], vibr[:res.height]

    # ---- a node with its MIR loop in ONE engine call (include/jslpr_mir.h) ------------------------------
    def _absorb_mir(self, res, outcome):
        """fold the outcome of a node evaluated WITH its MIR loop: `res` is the last simplex()'s result with the evaluation already folded
        over all of them (an optimal one sets it, an unbounded one sets -Infinity, any other keeps it), `outcome` says how many ended
        optimal.  A node none of whose simplexes set the evaluation leaves this object's as it is.  unboundedVarIndex follows the LAST simplex
        only: the 32-byte outcome record has no room for the variable of an earlier unbounded one (include/jslpr_mir.h)."""
        self.last = res
        self.feasible = bool(res.feasible)
        self.bounded = bool(res.bounded)
        n_opt = int(outcome["optimal_count"])
        if n_opt > 0 or res.evaluation == float("-inf"):
            self.evaluation = res.evaluation
        if n_opt > 0 and self.simplexIters == 0:
            self.bestPossibleEval = res.evaluation  # (the services evaluate the root round by round: they never get here)
        self.simplexIters += n_opt
        if not res.bounded:
            self.unboundedVarIndex = res.unbounded_var_index
        return res

    def _mir_native(self, what):
        """True: the library runs the loop (HIP, jslpr_* exported); False: the oracle, for which the call is restated below from
        applyCuts / applyCutsFrom + mirRound.  A HIP library without the extension is an error, never a fallback."""
        if self.lib.has_mir:
            return True
        if self.lib.backend == "oracle-c":
            return False
        raise _capi.EngineError("%s: %s does not export the MIR extension (include/jslpr_mir.h)" % (what, self.lib.path))

    @staticmethod
    def _mir_rounds_arg(max_rounds):
        if max_rounds is None or max_rounds < 0:
            return -1
        if max_rounds > _capi.JSLPR_MAX_ROUNDS:
            raise _capi.EngineError("relax_mir failed (%d): max_rounds > JSLPR_MAX_ROUNDS" % _capi.JSLP_ERR_ARG)
        return int(max_rounds)

    def _mir_restated(self, cuts, max_rounds, need_feasible, checkpoint, check_cycles):
        """the sequence the one-call form stands for, call by call: (result, outcome, rhs, varIndexByRow), this object's scalars folded"""
        if not self.integer_variables:
            raise _capi.EngineError("relax_mir failed (%d): after set_integer_variables" % _capi.JSLP_ERR_STATE)
        if self.n_optional > 0:
            raise _capi.EngineError("relax_mir failed (%d): optional objectives" % _capi.JSLP_ERR_UNSUPPORTED)
        if checkpoint is not None:
            (res, rhs, vibr), = self.applyCutsFrom(checkpoint, [cuts], check_cycles=check_cycles)
            self.absorb_from(checkpoint, res)
        else:
            res, rhs, vibr = self.applyCuts(cuts, check_cycles=check_cycles)
        oc = np.zeros((), dtype=_capi.MIR_OUTCOME_DTYPE)
        oc["optimal_count"] = int(bool(res.optimal))
        oc["pivots"] = res.pivots_phase1 + max(res.pivots_phase2, 0)
        if not (need_feasible and not self.feasible):
            limit = _capi.JSLPR_MAX_ROUNDS if max_rounds < 0 else max_rounds
            stopped = limit == 0
            while int(oc["rounds"]) < limit:
                before = fractional_volume_rows(self.integer_variables, rhs, vibr, self.precision)
                n, res, rhs, vibr = self.mirRound(check_cycles=check_cycles)
                after = fractional_volume_rows(self.integer_variables, rhs, vibr, self.precision)
                oc["rounds"] += 1
                oc["rows_added"] += n
                oc["optimal_count"] += int(bool(res.optimal))
                oc["pivots"] += res.pivots_phase1 + max(res.pivots_phase2, 0)
                oc["volume_before"], oc["volume_after"] = before, after
                if after >= 0.9 * before:
                    stopped = True
                    break
            if max_rounds < 0 and not stopped:
                raise _capi.EngineError("relax_mir failed (%d): the MIR loop reached JSLPR_MAX_ROUNDS" % _capi.JSLP_ERR_CAPACITY)
        out = SimplexResult.from_buffer_copy(res)
        out.evaluation = self.evaluation
        return out, oc, rhs, vibr

    def applyCutsMIR(self, cuts, max_rounds=None, need_feasible=False, checkpoint=None, check_cycles=True):
        """A node WITH its MIR loop as ONE engine call (jslpr_engine_relax_mir): restore (or restoreCheckpoint) + addCutConstraints +
        simplex, then -- unless need_feasible and the tableau is infeasible -- computeFractionalVolume / applyMIRCuts / simplex rounds until
        the volume stops shrinking by 10 % or max_rounds (None: the default service's unbounded loop) is reached.  Returns (result of the
        last simplex with the evaluation folded over all of them, outcome (_capi.MIR_OUTCOME_DTYPE), rhs, varIndexByRow); this object's
        scalars are folded as the call-by-call sequence folds them."""
        rounds = self._mir_rounds_arg(max_rounds)
        if not self._mir_native("applyCutsMIR"):
            return self._mir_restated(cuts, rounds, need_feasible, checkpoint, check_cycles)
        n, t, v, x = self._pack_cuts(cuts)
        offs = np.array([0, n], dtype=np.int32)
        res = SimplexResult()
        oc = np.zeros(1, dtype=_capi.MIR_OUTCOME_DTYPE)
        rhs = np.empty(self.row_capacity, dtype=np.float64)
        vibr = np.empty(self.row_capacity, dtype=np.int32)
        self.lib.check(self.lib.jslpr_engine_relax_mir(self._h, -1 if checkpoint is None else checkpoint["id"], 1, _capi.ptr_i32(offs), _capi.ptr_i8(t),
                                                       _capi.ptr_i32(v), _capi.ptr_f64(x), int(bool(check_cycles)), rounds, int(bool(need_feasible)),
                                                       _capi.C.byref(res), _capi.C.c_void_p(oc.ctypes.data), _capi.ptr_f64(rhs), _capi.ptr_i32(vibr),
                                                       self.row_capacity), "jslpr_engine_relax_mir")
        if checkpoint is not None:
            self.evaluation = checkpoint["evaluation"]
            self.feasible = checkpoint["feasible"]
        self._absorb_mir(res, oc[0])
        return res, oc[0], rhs[:res.height], vibr[:res.height]

    def applyCutsBatchMIR(self, cut_lists, max_rounds=None, need_feasible=False, check_cycles=True, packed=None):
        """Independent nodes of the saved root, each with its MIR loop, in one call.  Returns (results, outcomes, rhs, varIndexByRow) as
        applyCutsBatch lays them out (row stride = row_capacity).  Like applyCutsBatch it folds nothing into this object: the tree does,
        node by node, with _absorb_mir.  Every node's folded evaluation starts from the evaluation the call began with."""
        rounds = self._mir_rounds_arg(max_rounds)
        pk = packed if packed is not None else self.pack_cut_lists(cut_lists)
        n_nodes, offs, t, v, x = pk
        out = (SimplexResult * max(n_nodes, 1))()
        ocs = np.zeros(max(n_nodes, 1), dtype=_capi.MIR_OUTCOME_DTYPE)
        stride = self.row_capacity
        rhs = np.empty((max(n_nodes, 1), stride), dtype=np.float64)
        vibr = np.empty((max(n_nodes, 1), stride), dtype=np.int32)
        if self._mir_native("applyCutsBatchMIR"):
            self.lib.check(self.lib.jslpr_engine_relax_mir(self._h, -1, n_nodes, _capi.ptr_i32(offs), _capi.ptr_i8(t), _capi.ptr_i32(v), _capi.ptr_f64(x),
                                                           int(bool(check_cycles)), rounds, int(bool(need_feasible)), out,
                                                           _capi.C.c_void_p(ocs.ctypes.data), _capi.ptr_f64(rhs), _capi.ptr_i32(vibr), stride),
                           "jslpr_engine_relax_mir")
            return [out[i] for i in range(n_nodes)], ocs[:n_nodes], rhs, vibr
        scalars = ("last", "feasible", "bounded", "evaluation", "simplexIters", "bestPossibleEval", "unboundedVarIndex")
        kept = {k: getattr(self, k) for k in scalars}
        results = []
        try:
            for i in range(n_nodes):
                for k, val in kept.items():
                    setattr(self, k, val)
                cuts = [{"type": "min" if t[j] == _capi.JSLP_CUT_MIN else "max", "varIndex": int(v[j]), "value": float(x[j])}
                        for j in range(int(offs[i]), int(offs[i + 1]))]
                res, oc, r, w = self._mir_restated(cuts, rounds, need_feasible, None, check_cycles)
                results.append(res)
                ocs[i] = oc
                rhs[i, :res.height] = r
                vibr[i, :res.height] = w
        finally:
            for k, val in kept.items():
                setattr(self, k, val)
        return results, ocs[:n_nodes], rhs, vibr

    # ---- checkpoints (incremental-branch-and-cut.ts:31-107) -------------------------------------------
    def createCheckpoint(self):
        """createCheckpoint (:55-70): the matrix and the index maps stay in HBM; the host part of a StateCheckpoint
        (`evaluation`, `feasible`, :42-43) travels in the returned dict."""
        cid = _capi.C.c_int32(-1)
        self.lib.check(self.lib.jslp_engine_checkpoint_create(self._h, _capi.C.byref(cid)), "jslp_engine_checkpoint_create")
        return {"id": cid.value, "evaluation": self.evaluation, "feasible": self.feasible}

    def restoreCheckpoint(self, checkpoint):
        """restoreCheckpoint (:72-107)"""
        self.lib.check(self.lib.jslp_engine_checkpoint_restore(self._h, checkpoint["id"]), "jslp_engine_checkpoint_restore")
        self.evaluation = checkpoint["evaluation"]
        self.feasible = checkpoint["feasible"]

    def releaseCheckpoint(self, checkpoint):
        self.lib.check(self.lib.jslp_engine_checkpoint_release(self._h, checkpoint["id"]), "jslp_engine_checkpoint_release")

    def applyCutsFrom(self, checkpoint, cut_lists, check_cycles=True):
        """applyIncrementalCuts' fast path (:248-253) for one or more children of `checkpoint` in ONE engine call:
        restoreCheckpoint + addCutConstraints(cuts) + simplex + read-back per node.  Returns per node
        (result, rhs, varIndexByRow).  The engine's live tableau and its evaluation end as after the LAST node (the last of several
        children is evaluated on the live tableau itself); this object's `evaluation` / `feasible` are the caller's to fold, node by
        node, with absorb_from().  A checkpoint carries no optional objectives: on a model that has them send one child per call (the
        objective rows the other children would start from are whatever an earlier batch left in their slots)."""
        n_nodes, offs, t, v, x = self.pack_cut_lists(cut_lists)
        out = (SimplexResult * max(n_nodes, 1))()
        stride = self.row_capacity
        rhs = np.empty((max(n_nodes, 1), stride), dtype=np.float64)
        vibr = np.empty((max(n_nodes, 1), stride), dtype=np.int32)
        self.lib.check(self.lib.jslp_engine_relax_from(self._h, checkpoint["id"], n_nodes, _capi.ptr_i32(offs),
                                                       _capi.ptr_i8(t), _capi.ptr_i32(v), _capi.ptr_f64(x),
                                                       int(bool(check_cycles)), out, _capi.ptr_f64(rhs),
                                                       _capi.ptr_i32(vibr), stride), "jslp_engine_relax_from")
        return [(out[i], rhs[i, :out[i].height], vibr[i, :out[i].height]) for i in range(n_nodes)]

    def absorb_from(self, checkpoint, res):
        """the tableau scalars after restoreCheckpoint(checkpoint) + simplex() with outcome `res`"""
        self.evaluation = checkpoint["evaluation"]
        self.feasible = checkpoint["feasible"]
        return self._absorb(res)

    # ---- read-back --------------------------------------------------------------------------------
    def read_rhs(self):
        h = self.height
        rhs = np.empty(h, dtype=np.float64)
        vibr = np.empty(h, dtype=np.int32)
        self.lib.check(self.lib.jslp_engine_read_rhs(self._h, _capi.ptr_f64(rhs), _capi.ptr_i32(vibr)),
                       "jslp_engine_read_rhs")
        return rhs, vibr

    def download(self):
        h = _capi.C.c_int32()
        w = _capi.C.c_int32()
        n = _capi.C.c_int32()
        self.lib.check(self.lib.jslp_engine_dims(self._h, _capi.C.byref(h), _capi.C.byref(w), _capi.C.byref(n)),
                       "jslp_engine_dims")
        m = np.empty((h.value, w.value), dtype=np.float64)
        vibr = np.empty(h.value, dtype=np.int32)
        vibc = np.empty(w.value, dtype=np.int32)
        rbv = np.empty(n.value, dtype=np.int32)
        cbv = np.empty(n.value, dtype=np.int32)
        self.lib.check(self.lib.jslp_engine_download(self._h, _capi.ptr_f64(m), _capi.ptr_i32(vibr), _capi.ptr_i32(vibc),
                                                     _capi.ptr_i32(rbv), _capi.ptr_i32(cbv)), "jslp_engine_download")
        return m, vibr, vibc, rbv, cbv

    def optional_objectives(self):
        """current optionalObjectives[o].reducedCosts rows (n x width)"""
        rows = np.zeros((max(self.n_optional, 1), self.width), dtype=np.float64)
        n = _capi.C.c_int32()
        self.lib.check(self.lib.jslp_engine_get_optional_objectives(self._h, _capi.ptr_f64(rows), _capi.C.byref(n)),
                       "jslp_engine_get_optional_objectives")
        return rows[:n.value]

    def pivot_trace(self):
        n = _capi.C.c_int64()
        self.lib.check(self.lib.jslp_engine_pivot_trace(self._h, None, 0, _capi.C.byref(n)), "jslp_engine_pivot_trace")
        buf = np.empty(2 * max(n.value, 1), dtype=np.int32)
        self.lib.check(self.lib.jslp_engine_pivot_trace(self._h, _capi.ptr_i32(buf), n.value, _capi.C.byref(n)),
                       "jslp_engine_pivot_trace")
        return buf[:2 * n.value].reshape(-1, 2)

    def last_path(self):
        return self.lib.jslp_engine_last_path(self._h).decode()

    def set_timing(self, enabled):
        self.lib.check(self.lib.jslp_engine_set_timing(self._h, int(bool(enabled))), "jslp_engine_set_timing")

    def get_timing(self):
        ms = _capi.C.c_double()
        n = _capi.C.c_int64()
        tot = _capi.C.c_double()
        self.lib.check(self.lib.jslp_engine_get_timing(self._h, _capi.C.byref(ms), _capi.C.byref(n), _capi.C.byref(tot)),
                       "jslp_engine_get_timing")
        return ms.value, n.value, tot.value


class DevicePool:
    """jslp_pool: `tableau` (the primary) plus one engine per further device ordinal, each holding the primary's saved
    root; batches of independent nodes are split over the members.  devices[0] must be the primary's."""

    def __init__(self, tableau, devices):
        self.t = tableau
        self.lib = tableau.lib
        d = _capi.as_i32(list(devices))
        self._p = _capi.C.c_void_p()
        self.lib.check(self.lib.jslp_pool_create(_capi.C.byref(self._p), tableau._h, _capi.ptr_i32(d), int(d.shape[0])),
                       "jslp_pool_create")
        self.n_watched = 0  # (informational: the outputs are sized with jslp_pool_watched_count)

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self.lib.jslp_pool_destroy(self._p)
            self._p = _capi.C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return self.lib.jslp_pool_size(self._p)

    def sync_root(self):
        self.lib.check(self.lib.jslp_pool_sync_root(self._p), "jslp_pool_sync_root")

    def applyCutsBatch(self, cut_lists, check_cycles=True, packed=None, want_rows=True, copy=True):
        """Tableau.applyCutsBatch over every member of the pool"""
        t = self.t
        pk = packed if packed is not None else t.pack_cut_lists(cut_lists)
        n_nodes, offs, ty, v, x = pk
        out = (SimplexResult * max(n_nodes, 1))()
        stride = t.row_capacity
        if copy:
            rhs = np.empty((max(n_nodes, 1), stride), dtype=np.float64)
            vibr = np.empty((max(n_nodes, 1), stride), dtype=np.int32) if want_rows else None
            self.lib.check(self.lib.jslp_pool_relax_batch(self._p, n_nodes, _capi.ptr_i32(offs), _capi.ptr_i8(ty), _capi.ptr_i32(v),
                                                          _capi.ptr_f64(x), int(bool(check_cycles)), out, _capi.ptr_f64(rhs),
                                                          _capi.ptr_i32(vibr), stride), "jslp_pool_relax_batch")
            return [out[i] for i in range(n_nodes)], rhs, vibr
        p_rhs = _capi._f64p()
        p_rows = _capi._i32p()
        c_stride = _capi.C.c_int32()
        self.lib.check(self.lib.jslp_pool_relax_batch_pinned(
            self._p, n_nodes, *_cut_ptrs(pk), int(bool(check_cycles)),
            out, _capi.C.byref(p_rhs), _capi.C.byref(p_rows) if want_rows else None, _capi.C.byref(c_stride)),
            "jslp_pool_relax_batch_pinned")
        shape = (max(n_nodes, 1), c_stride.value)
        rhs = _pinned_view(p_rhs, shape)
        vibr = _pinned_view(p_rows, shape) if want_rows else None
        return out, rhs, vibr

    def set_watched_variables(self, var_indexes):
        """the variables whose row / RHS cell the compact read-back returns, on every member (jslp_pool_set_watched_variables)"""
        idx = _capi.as_i32(list(var_indexes))
        self.lib.check(self.lib.jslp_pool_set_watched_variables(self._p, _capi.ptr_i32(idx), int(idx.shape[0])),
                       "jslp_pool_set_watched_variables")
        self.n_watched = int(idx.shape[0])

    def applyCutsBatchWatched(self, cut_lists, check_cycles=True, packed=None, copy=True):
        """Tableau.applyCutsBatchWatched over every member of the pool: per node rowByVarIndex / the RHS cell of the watched
        variables (what mip-utils.ts:43-61, 100-126 read between relaxations); copy=False: views of the pool's pinned buffer"""
        t = self.t
        pk = packed if packed is not None else t.pack_cut_lists(cut_lists)
        n_nodes, offs, ty, v, x = pk
        out = (SimplexResult * max(n_nodes, 1))()
        # (the outputs are sized by what the LIBRARY will write -- jslp_pool_watched_count -- not by a Python-side shadow
        #  that a direct set_watched_variables on the primary engine would leave behind)
        n_watched = int(self.lib.jslp_pool_watched_count(self._p))
        if n_watched <= 0:
            raise _capi.EngineError("DevicePool.applyCutsBatchWatched: %s" % ("call set_watched_variables first" if n_watched == 0 else
                                    "the members' watched variables differ (set them through DevicePool.set_watched_variables)"))
        shape = (max(n_nodes, 1), n_watched)
        if not copy:
            p_rows = _capi._i32p()
            p_vals = _capi._f64p()
            self.lib.check(self.lib.jslp_pool_relax_batch_watched_pinned(
                self._p, n_nodes, *_cut_ptrs(pk), int(bool(check_cycles)), out,
                _capi.C.byref(p_rows), _capi.C.byref(p_vals)), "jslp_pool_relax_batch_watched_pinned")
            return out, _pinned_view(p_rows, shape), _pinned_view(p_vals, shape)
        rows = np.empty(shape, dtype=np.int32)
        vals = np.empty(shape, dtype=np.float64)
        self.lib.check(self.lib.jslp_pool_relax_batch_watched(self._p, n_nodes, _capi.ptr_i32(offs), _capi.ptr_i8(ty), _capi.ptr_i32(v),
                                                              _capi.ptr_f64(x), int(bool(check_cycles)), out, _capi.ptr_i32(rows),
                                                              _capi.ptr_f64(vals)), "jslp_pool_relax_batch_watched")
        return out, rows, vals

    def set_counting(self, enabled):
        self.lib.check(self.lib.jslp_pool_set_counting(self._p, int(bool(enabled))), "jslp_pool_set_counting")

    def get_counters(self):
        c = _capi.WorkCounters()
        self.lib.check(self.lib.jslp_pool_get_counters(self._p, _capi.C.byref(c)), "jslp_pool_get_counters")
        return c.as_dict()


_EPSILON = 2.220446049250313e-16


def simplex_many(tableaux, check_cycles=True):
    """simplex() of many independent tableaus in one engine call (include/jslpm_many.h): the results, in order, each folded into its
    Tableau exactly as Tableau.simplex() folds it.  `check_cycles` is one bool for all or one per tableau.

    Every tableau must use the same Library.  The HIP library solves the batch with jslpm_simplex_many; the CPU oracle (which does not
    export the extension) runs the same calls one by one; a HIP library without the extension is an error, never a fallback."""
    tableaux = list(tableaux)
    n = len(tableaux)
    if isinstance(check_cycles, (bool, int, np.bool_)):
        flags = [bool(check_cycles)] * n
    else:
        flags = [bool(c) for c in check_cycles]
        if len(flags) != n:
            raise ValueError("simplex_many: %d check_cycles flags for %d tableaus" % (len(flags), n))
    if n == 0:
        return []
    lib = tableaux[0].lib
    if any(t.lib is not lib for t in tableaux):
        raise ValueError("simplex_many: every tableau must use the same engine library")
    if not lib.has_many:
        if lib.backend == "oracle-c":
            return [t.simplex(check_cycles=c) for t, c in zip(tableaux, flags)]
        raise _capi.EngineError("simplex_many: %s does not export the batch extension (include/jslpm_many.h)" % lib.path)
    handles = (_capi.C.c_void_p * n)(*[t._h.value for t in tableaux])
    cc = _capi.as_i32([int(c) for c in flags])
    out = (SimplexResult * n)()
    status = np.zeros(n, dtype=np.int32)
    rc = lib.jslpm_simplex_many(handles, n, _capi.ptr_i32(cc), out, _capi.ptr_i32(status))
    if rc != _capi.JSLP_OK and not status.any():  # refused before any work
        lib.check(rc, "jslpm_simplex_many")
    for t, res, st in zip(tableaux, out, status):  # (an LP that failed leaves its tableau's scalars alone, as simplex() does)
        if st == _capi.JSLP_OK:
            t._absorb(res)
    lib.check(rc, "jslpm_simplex_many")
    return list(out)


def fractional_volume_rows(integer, rhs, vibr, precision):
    """computeFractionalVolume(ignoreIntegerValues = true) (mip-utils.ts:67-92): the product, in row order, of |value| over the basic
    variables of the set `integer` that are not at an integer value.  Math.min(NaN, x) is NaN and NaN < precision is false: a NaN
    row multiplies in."""
    volume = -1.0
    for r in range(1, len(vibr)):
        if int(vibr[r]) in integer:
            distance = abs(float(rhs[r]))
            a = distance - math.floor(distance) if math.isfinite(distance) else math.nan
            b = math.floor(distance + 1) if math.isfinite(distance) else distance
            nearest = math.nan if (a != a or b != b) else min(a, b)
            if nearest < precision:
                continue
            volume = distance if volume == -1.0 else volume * distance
    return 0.0 if volume == -1.0 else volume


def _js_round(x):
    """Math.round: nearest integer, ties toward +Infinity"""
    if x != x or x in (float("inf"), float("-inf")):
        return x
    f = float(np.floor(x))
    return f + 1.0 if x - f >= 0.5 else f


def branch_record_from_watched(results, wrows, wvals, watched, precision):
    """The branch record (include/jslpx_branch.h) restated from the compact read-back of the same nodes -- the oracle's records and the
    tests' yardstick.  results: SimplexResult per node (or one); wrows / wvals: [n, w] rows (-1 = not basic) and RHS cells of the watched
    variables `watched`, in registration order.  Returns a structured array (_capi.BRANCH_RECORD_DTYPE) of n records:
    isIntegral() (mip-utils.ts:43-61) and getMostFractionalVar() (:100-126) over the basic watched variables, Math.round ties toward
    +Infinity, fractions compared strictly (> precision, > the best so far: the first of equal fractions wins, NaN never does)."""
    if isinstance(results, SimplexResult):
        results = [results]
    n = len(results)
    rows = np.asarray(wrows, dtype=np.int64).reshape(n, -1)
    vals = np.asarray(wvals, dtype=np.float64).reshape(n, -1)
    watched = np.asarray(watched, dtype=np.int64)
    out = np.zeros(n, dtype=_capi.BRANCH_RECORD_DTYPE)
    with np.errstate(invalid="ignore"):
        for i, r in enumerate(results):
            basic = (rows[i] > 0) & (rows[i] < r.height)
            v = vals[i]
            f = np.floor(v)
            frac = np.abs(v - np.where(v - f >= 0.5, f + 1.0, f))
            integral = not bool(((frac > precision) & basic).any())
            key = np.where(basic & ~np.isnan(frac), frac, -1.0)
            k = int(np.argmax(key)) if key.size else 0  # first index of the maximum
            pick = key.size > 0 and key[k] > 0.0
            flags = ((_capi.BRANCH_FEASIBLE if r.feasible else 0) | (_capi.BRANCH_BOUNDED if r.bounded else 0) |
                     (_capi.BRANCH_OPTIMAL if r.optimal else 0) | (_capi.BRANCH_INTEGRAL if integral else 0))
            out[i] = (flags, r.unbounded_var_index, int(watched[k]) if pick else -1, r.height, r.obj_cell, float(v[k]) if pick else 0.0)
    return out


def pivot_digest(pairs):
    """FNV-1a-32 over the (row, col) arguments of every pivot."""
    h = 2166136261
    for r, c in np.asarray(pairs, dtype=np.int64).reshape(-1, 2):
        h = ((h ^ int(r)) * 16777619) & 0xFFFFFFFF
        h = ((h ^ int(c)) * 16777619) & 0xFFFFFFFF
    return "%x" % h


def pack_lds_bytes(height, width, n_optional=0):
    """jslpp_lds_bytes (include/jslpp_packed.h) restated: the dynamic LDS one LP of a pack needs -- the tableau with its row stride padded to
    an odd number of doubles, the pivot column, and the integer block [vibr | vibc | rbv | cbv | unrestricted flags] with every piece padded
    to 16 bytes.  What a library without the extension (the oracle) is asked instead; tests/test_packed_abi.py holds the two together.
    n_optional: the LP's optional objectives, one row of the same stride each behind the pivot column (jslps_lds_bytes,
    include/jslps_soft.h; tests/test_packed_soft_abi.py)."""
    h, w, no = int(height), int(width), int(n_optional)
    if h < 2 or w < 2 or no < 0:
        return 0
    pad4 = lambda n: (n + 3) & ~3  # noqa: E731
    n_idx = w + 2 * h + 2
    doubles = (h * (w | 1) + h + no * (w | 1) + 1) & ~1
    ints = pad4(h) + pad4(w) + 2 * pad4(n_idx) + pad4((n_idx + 3) // 4)
    return 8 * doubles + 4 * ints


def tree_lds_bytes(height, width, row_capacity, n_optional=0):
    """jslpt_lds_bytes (include/jslpt_tree.h) restated: pack_lds_bytes with the tableau and the maps sized for row_capacity rows
    (n_optional: jslps_tree_lds_bytes)"""
    h, w, rc = int(height), int(width), int(row_capacity)
    if h < 2 or w < 2 or rc < h:
        return 0
    return pack_lds_bytes(rc, w, n_optional)


def tree_cut_rows(height, width, n_int, lib=None, n_optional=0, limit=None):
    """the cut rows a model with n_int integer variables (and n_optional optional objectives) joins a tree pack with: 2 per integer variable
    -- the most a cut list can hold (branch-and-cut.ts:166-179) -- or the most that fit the LDS limit; 0 when not even one fits.
    limit: the pack's LDS limit in bytes (None: JSLPP_LDS_LIMIT; a pack with big_lds: JSLPB_LDS_LIMIT, include/jslpb_big_lds.h)"""
    limit = _capi.JSLPP_LDS_LIMIT if limit is None else int(limit)
    def fits(cut_rows):
        if n_optional and lib is not None and getattr(lib, "has_soft", False):
            b = int(lib.jslps_tree_lds_bytes(int(height), int(width), int(height) + cut_rows, int(n_optional)))
        elif not n_optional and lib is not None and getattr(lib, "has_tree", False):
            b = int(lib.jslpt_lds_bytes(int(height), int(width), int(height) + cut_rows))
        else:
            b = tree_lds_bytes(height, width, int(height) + cut_rows, n_optional)
        return 0 < b <= limit
    lo, hi = 0, 2 * int(n_int)
    if fits(hi):
        return hi
    while lo < hi:  # (the byte count is monotone in the row capacity)
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid - 1)
    return lo


def tree_mir_lds_bytes(height, width, row_capacity):
    """jslpc_tree_lds_bytes (include/jslpc_tree_mir.h) restated: tree_lds_bytes with variable.isInteger per variable index (one byte each,
    padded to 16) behind the integer block"""
    b = tree_lds_bytes(height, width, row_capacity)
    if b == 0:
        return 0
    n_idx = int(width) + 2 * int(row_capacity) + 2
    return b + 4 * (((n_idx + 3) // 4 + 3) & ~3)


MIR_ROW_HEADROOM = 320  # rows a MIR LP gets beyond its cut rows by default: 32 rounds of 10, as Solve gives an engine (solver._prepare)


def tree_mir_rows(height, width, n_int, lib=None, cut_rows=None):
    """(row_extra, cut_rows) a model with options.useMIRCuts and n_int integer variables joins a tree pack with (include/jslpc_tree_mir.h):
    row_extra = min(cut rows + MIR_ROW_HEADROOM, the most rows that fit the LDS limit) and cut_rows = min(2 per integer variable,
    row_extra); (0, 0) when not even one row fits.  cut_rows: the LP's own count instead of 2 per integer variable."""
    def fits(extra):
        if lib is not None and getattr(lib, "has_tree_mir", False):
            b = int(lib.jslpc_tree_lds_bytes(int(height), int(width), int(height) + extra))
        else:
            b = tree_mir_lds_bytes(height, width, int(height) + extra)
        return 0 < b <= _capi.JSLPP_LDS_LIMIT
    cuts = 2 * int(n_int) if cut_rows is None else int(cut_rows)
    lo, hi = 0, cuts + MIR_ROW_HEADROOM
    if not fits(hi):
        while lo < hi:  # (the byte count is monotone in the row capacity)
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid - 1)
        hi = lo
    return hi, min(cuts, hi)


INCREMENTAL_ROW_HEADROOM = 256  # rows an incremental LP gets beyond 2 per integer variable by default, as Solve gives an engine (solver._prepare)


def incremental_rows(height, width, n_int, lib=None, cut_rows=None):
    """(row_extra, cut_rows) a model with options.useIncremental and n_int integer variables joins a tree pack with
    (include/jslpi_tree_incremental.h): row_extra = min(2 per integer variable + INCREMENTAL_ROW_HEADROOM, the most rows that fit the LDS
    limit) and cut_rows = min(2 per integer variable, row_extra); (0, 0) when not even one row fits.  cut_rows: the LP's own count instead
    of 2 per integer variable."""
    def fits(extra):
        if lib is not None and getattr(lib, "has_tree_inc", False):
            b = int(lib.jslpi_tree_lds_bytes(int(height), int(width), int(height) + extra))
        else:
            b = tree_lds_bytes(height, width, int(height) + extra)
        return 0 < b <= _capi.JSLPP_LDS_LIMIT
    cuts = 2 * int(n_int) if cut_rows is None else int(cut_rows)
    lo, hi = 0, cuts + INCREMENTAL_ROW_HEADROOM
    if not fits(hi):
        while lo < hi:  # (the byte count is monotone in the row capacity)
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid - 1)
        hi = lo
    return hi, min(cuts, hi)


def checkpoint_bytes(height, width, row_capacity):
    """jslpi_checkpoint_bytes (include/jslpi_tree_incremental.h) restated: one checkpoint slot of an incremental LP -- a 16-byte header, the
    rows of the row capacity in 16-byte words, the whole integer block of tree_lds_bytes"""
    h, w, rc = int(height), int(width), int(row_capacity)
    if h < 2 or w < 2 or rc < h:
        return 0
    pad4 = lambda n: (n + 3) & ~3  # noqa: E731
    n_idx = w + 2 * rc + 2
    return 16 + 16 * ((rc * w + 1) // 2) + 4 * (pad4(rc) + pad4(w) + 2 * pad4(n_idx) + pad4((n_idx + 3) // 4))


class _TreeModel:
    """what branch_and_cut.branch_and_cut reads of a model, for an LP of a pack: its tolerance (0: none) and its sense, no timeout"""
    timeout = None

    def __init__(self, integers, check_cycles, mir=False, tolerance=0, minimize=True):
        self.tolerance = tolerance
        self.isMinimization = bool(minimize)
        self.integer_index_array = np.asarray(integers, dtype=np.int64)
        self.integer_index_set = frozenset(int(i) for i in integers)
        self.integerVariables = [{"index": int(i)} for i in integers]  # (what the enhanced service's selectBranchingVariable reads)
        self.checkForCycles = bool(check_cycles)
        self.useMIRCuts = bool(mir)


class _MirCounters:
    """what jslpc_pack_read_mir reports of a MIR LP, gathered around the calls of the host tree on the LP's twin (applyCuts, mirRound, save),
    with the kernel's bound on the rounds of one node enforced"""

    def __init__(self, tableau):
        from .branch_and_cut import TreeCapacity
        self.t, self.height0 = tableau, tableau.height0
        self.rounds = self.rows_added = self.simplexes = self.root_rows = self.node_rounds = 0
        self.tallest = self.height0
        apply_cuts, mir_round, save = tableau.applyCuts, tableau.mirRound, tableau.save

        def applyCuts(cuts, check_cycles=True):
            self.node_rounds = 0
            out = apply_cuts(cuts, check_cycles=check_cycles)
            self.simplexes += 1
            self.tallest = max(self.tallest, out[0].height)
            return out

        def mirRound(check_cycles=True):
            if self.node_rounds >= _capi.JSLPR_MAX_ROUNDS:
                raise TreeCapacity("mir rounds")
            out = mir_round(check_cycles=check_cycles)
            self.node_rounds += 1
            self.rounds += 1
            self.rows_added += out[0]
            self.simplexes += 1
            self.tallest = max(self.tallest, out[1].height)
            return out

        def save_root():
            save()
            self.root_rows = tableau.last.height - self.height0

        tableau.applyCuts, tableau.mirRound, tableau.save = applyCuts, mirRound, save_root

    def detach(self):
        for name in ("applyCuts", "mirRound", "save"):
            self.t.__dict__.pop(name, None)

    def record(self):
        return (self.rounds, self.rows_added, self.simplexes, self.root_rows, self.tallest - self.height0)


def pack_fits(height, width, lib=None, n_optional=0, limit=None):
    """whether a tableau of this shape (with n_optional optional objectives) can join a TableauPack: its LDS image stays within the 64 KiB
    the pack kernels are launched with -- or within `limit` bytes (a pack with big_lds: JSLPB_LDS_LIMIT, include/jslpb_big_lds.h)"""
    if n_optional and lib is not None and getattr(lib, "has_soft", False):
        b = int(lib.jslps_lds_bytes(int(height), int(width), int(n_optional)))
    elif not n_optional and lib is not None and getattr(lib, "has_pack", False):
        b = int(lib.jslpp_lds_bytes(int(height), int(width)))
    else:
        b = pack_lds_bytes(height, width, n_optional)
    return 0 < b <= (_capi.JSLPP_LDS_LIMIT if limit is None else int(limit))


class TableauPack:
    """Many small independent LPs in one object (include/jslpp_packed.h): one arena, one upload, one launch per kernel build that solves
    every LP with its whole tableau in LDS, one read-back.  `lps` is a list of (matrix, var_index_by_row, var_index_by_col, unrestricted);
    `precision` one tolerance or one per LP.  trace_cap: pivot pairs recorded per LP; max_pivots > 0 caps the pivots per LP and call.

    simplex() returns the results as ONE numpy structured array (_capi.RESULT_DTYPE, a field per jslp_simplex_result member) and keeps
    `status` (per-LP engine codes), `evaluation`, `feasible` and `bounded` as arrays; result(i) is LP i's SimplexResult.

    A library without the extension (the CPU oracle) gets a RESTATEMENT behind the same interface: one engine per LP, solved one after the
    other (max_pivots is then the engine's own cap) -- the host logic stays testable without a GPU.  A HIP library without the extension is
    an error, never a fallback.

    optional_objectives: one entry per LP, None or that LP's n x width optional objectives (include/jslps_soft.h), as Tableau takes them;
    optional_objectives(i) reads LP i's rows back after a solve.

    mir: one flag per LP of a pack with trees (include/jslpc_tree_mir.h): the LP's model has options.useMIRCuts, and every node of its tree
    runs its MIR-cut loop.  Such an LP's rows -- the root's MIR rows, a node's cuts, the node's MIR rows -- come out of a row capacity of
    height + row_extra (one number or one per LP; default: cut_rows + MIR_ROW_HEADROOM, capped by what fits the LDS limit), its cut lists
    still hold at most cut_rows cuts, and its integer variables are also its variable.isInteger.  `mir` (_capi.MIR_TREE_DTYPE: rounds,
    rows_added, simplexes, root_rows, rows_high_water) is the read-back of the last branch_and_cut(), zero for the other LPs; `is_mir` holds
    the flags.  Not together with optional objectives.

    node_selection / branching: one entry per LP of a pack with trees (include/jslpe_tree_enhanced.h): None, or the model's
    options.nodeSelection ("best-first", "depth-first", "hybrid") / options.branching ("most-fractional", "pseudocost", "strong").  An LP
    with either is an ENHANCED LP: its tree is walked under the enhanced service (one of the two left None gets its default, hybrid /
    pseudocost); its depth-first stack and its heap share heap_cap.  `enhanced` (_capi.ENH_TREE_DTYPE: solutions_found, stack_high_water,
    moved_to_heap, pseudo_updates, scored_by_pseudocost, dropped_nodes) is the read-back of the last branch_and_cut(), zero for the other
    LPs; `is_enhanced` holds the flags.  Not for an LP with `mir` or with optional objectives.

    incremental: one flag per LP of a pack with trees (include/jslpi_tree_incremental.h): the LP's model has options.useIncremental, and its
    tree is walked under the incremental service -- the enhanced walk (node_selection / branching as above, hybrid / pseudocost when
    None; `strong` means pseudocost) with parent checkpoints on the device, at most max_checkpoints (one number or one per LP; default
    50, the reference's) per call.  Such an LP has ONE row capacity, height + row_extra (one number or one per LP; default:
    incremental_rows), which the cut rows of a node that starts from the root and the stacked rows of a chain of checkpoints share.
    `incremental` (_capi.INC_TREE_DTYPE: checkpoints_used, incremental_nodes, rows_high_water, checkpoint_rows_high_water) is the
    read-back of the last branch_and_cut(), zero for the other LPs; `is_incremental` holds the flags; `enhanced` and `tree` report for such
    an LP what they report for an enhanced one.  Not for an LP with `mir` or with optional objectives.

    NOTE the two meanings of one name, which include/jslpg_tree_tolerance.h's Python face was asked to have: the ARGUMENT `tolerance=` takes the
    models' options.tolerance VALUES; the ATTRIBUTE `pack.tolerance` is the RECORD array a tree call reads back.  The values given are kept
    as `pack.tolerances` (plural).
    tolerance / minimize: one entry per LP of a pack with trees (include/jslpg_tree_tolerance.h): the model's options.tolerance (None, a value
    <= 0 or NaN: none, as `tolerance > 0` decides in the reference; any other value as it is) and whether the model minimises (default:
    every LP does).  An LP with a tolerance ends its walk as the reference's services end theirs: one node after the incumbent came within
    bestPossibleEval * (1 +- tolerance).  `tolerance` (_capi.TOL_TREE_DTYPE: best_possible, threshold,
    stopped, left) is the read-back of the last branch_and_cut(), zero for the other LPs; such an LP runs in the TOL twin of its kind's build,
    a launch of its own beside the LPs without a tolerance; `tolerances` holds the values given (0: none),
    `is_tolerance` the flags, `has_tolerance` whether any LP has one.

    big_lds=True (include/jslpb_big_lds.h): the pack's LDS limit is JSLPB_LDS_LIMIT, 156 KiB, instead of 64 KiB.  An LP whose image stays
    within 64 KiB is the LP it was; a larger one runs in the large build of its kind (`big_threads` threads, a compute unit to itself):
    plain LPs and default-service trees, each with or without optional objectives.  A MIR, an enhanced or an incremental LP and any LP with a
    tolerance keeps the 64 KiB rule.  `lds_limit` is the pack's limit, `is_big` the flags of the large LPs."""

    def __init__(self, lps, precision=1e-8, lib=None, device=0, trace_cap=0, max_pivots=0, integers=None, cut_rows=None, heap_cap=None,
                 max_nodes=0, optional_objectives=None, mir=None, row_extra=None, node_selection=None, branching=None, incremental=None,
                 max_checkpoints=_capi.JSLPI_CHECKPOINTS_DEFAULT, tolerance=None, minimize=None, big_lds=False):
        self.lib = lib if lib is not None else _capi.load_hip()
        self.big_lds = bool(big_lds)
        self.lds_limit = _capi.JSLPB_LDS_LIMIT if self.big_lds else _capi.JSLPP_LDS_LIMIT
        self._lps = []
        for matrix, vibr, vibc, unr in lps:
            m = _capi.as_f64(matrix)
            if m.ndim != 2:
                raise ValueError("matrix must be height x width")
            vibr, vibc = _capi.as_i32(vibr), _capi.as_i32(vibc)
            if vibr.shape[0] != m.shape[0] or vibc.shape[0] != m.shape[1]:
                raise ValueError("index maps do not match the matrix shape")
            self._lps.append((m, vibr, vibc, _capi.as_i32(list(unr))))
        self.n = n = len(self._lps)
        if isinstance(precision, (int, float)):
            self.precision = np.full(n, float(precision), dtype=np.float64)
        else:
            self.precision = _capi.as_f64(list(precision))
            if self.precision.shape[0] != n:
                raise ValueError("TableauPack: %d precisions for %d LPs" % (self.precision.shape[0], n))
        self.heights = _capi.as_i32([m.shape[0] for m, _, _, _ in self._lps])
        self.widths = _capi.as_i32([m.shape[1] for m, _, _, _ in self._lps])
        self.trace_cap, self.max_pivots, self.device = int(trace_cap), int(max_pivots), int(device)
        # per LP its optional objectives (None: none), n_optional x width
        self._optional = [None] * n
        if optional_objectives is not None:
            if len(optional_objectives) != n:
                raise ValueError("TableauPack: %d optional-objective entries for %d LPs" % (len(optional_objectives), n))
            for i, oo in enumerate(optional_objectives):
                if oo is None or len(oo) == 0:
                    continue
                oo = _capi.as_f64(oo)
                if oo.ndim != 2 or oo.shape[1] != self.widths[i]:
                    raise ValueError("TableauPack: LP %d: optional objectives must be n x width" % i)
                self._optional[i] = oo
        self.n_optional = _capi.as_i32([0 if oo is None else oo.shape[0] for oo in self._optional])
        self.has_optional = bool(self.n_optional.any())
        self.results = np.zeros(n, dtype=_capi.RESULT_DTYPE)
        self.status = np.zeros(n, dtype=np.int32)
        self.evaluation = np.zeros(n, dtype=np.float64)
        self.feasible = np.ones(n, dtype=bool)
        self.bounded = np.ones(n, dtype=bool)
        self.device_ms = 0.0
        self._launches = 0
        self._h = None
        self._twins = None
        # a pack with trees (include/jslpt_tree.h): per LP its integer variables in model order, its cut rows and its heap
        self.is_tree = integers is not None
        self.tree = np.zeros(n, dtype=_capi.TREE_DTYPE)
        if self.is_tree:
            self.integers = [_capi.as_i32(list(iv)) for iv in integers]
            if len(self.integers) != n:
                raise ValueError("TableauPack: %d integer lists for %d LPs" % (len(self.integers), n))
            self.cut_rows = self._per_lp(cut_rows, [2 * iv.shape[0] for iv in self.integers])
            self.heap_cap = self._per_lp(heap_cap, [128] * n)
            if self.cut_rows.shape[0] != n or self.heap_cap.shape[0] != n:
                raise ValueError("TableauPack: cut_rows / heap_cap are one number or one per LP")
            self.max_nodes = int(max_nodes) if max_nodes else _capi.JSLPT_MAX_NODES_DEFAULT
            self.row_capacity = self.heights + self.cut_rows
        else:
            self.row_capacity = self.heights
        # MIR LPs (include/jslpc_tree_mir.h): the flags
        self.is_mir = np.zeros(n, dtype=bool)
        self.mir = np.zeros(n, dtype=_capi.MIR_TREE_DTYPE)
        if mir is not None and any(mir):
            if not self.is_tree:
                raise ValueError("TableauPack: `mir` needs `integers` (a pack with trees)")
            if len(mir) != n:
                raise ValueError("TableauPack: %d mir flags for %d LPs" % (len(mir), n))
            self.is_mir = np.array([bool(f) for f in mir], dtype=bool)
            # (a pack with incremental LPs is made by jslpi_tree_pack_create, which takes every kind of tree LP: there a MIR LP and an LP
            # with optional objectives may stand side by side, though never in one LP)
            if self.has_optional and (incremental is None or not any(incremental) or (self.is_mir & (self.n_optional > 0)).any()):
                raise ValueError("TableauPack: MIR LPs and optional objectives do not share a pack (include/jslpc_tree_mir.h)")
        self.has_mir = bool(self.is_mir.any())
        # enhanced LPs (include/jslpe_tree_enhanced.h): the codes as the create takes them (0: not given)
        self.node_selection = np.zeros(n, dtype=np.int32)
        self.branching = np.zeros(n, dtype=np.int32)
        self.enhanced = np.zeros(n, dtype=_capi.ENH_TREE_DTYPE)
        for what, given, names, codes in (("node_selection", node_selection, _capi.ENH_NODE_SELECTION, self.node_selection),
                                          ("branching", branching, _capi.ENH_BRANCHING, self.branching)):
            if given is None or not any(g is not None for g in given):
                continue
            if not self.is_tree:
                raise ValueError("TableauPack: `%s` needs `integers` (a pack with trees)" % what)
            if len(given) != n:
                raise ValueError("TableauPack: %d %s entries for %d LPs" % (len(given), what, n))
            for i, g in enumerate(given):
                if g is not None and g not in names:
                    raise ValueError("TableauPack: LP %d: %s is None or one of %s, not %r" % (i, what, ", ".join(names), g))
                codes[i] = 0 if g is None else names[g]
        # incremental LPs (include/jslpi_tree_incremental.h): the flags and max_checkpoints per LP
        self.is_incremental = np.zeros(n, dtype=bool)
        self.incremental = np.zeros(n, dtype=_capi.INC_TREE_DTYPE)
        self.max_checkpoints = np.zeros(n, dtype=np.int32)
        if incremental is not None and any(incremental):
            if not self.is_tree:
                raise ValueError("TableauPack: `incremental` needs `integers` (a pack with trees)")
            if len(incremental) != n:
                raise ValueError("TableauPack: %d incremental flags for %d LPs" % (len(incremental), n))
            self.is_incremental = np.array([bool(f) for f in incremental], dtype=bool)
            limits = self._per_lp(max_checkpoints, None)
            if limits.shape[0] != n:
                raise ValueError("TableauPack: max_checkpoints is one number or one per LP")
            self.max_checkpoints = np.where(self.is_incremental, limits, 0).astype(np.int32)
            for i in np.flatnonzero(self.is_incremental):
                if self.is_mir[i] or self.n_optional[i] > 0:
                    raise ValueError("TableauPack: LP %d: an incremental LP has neither `mir` nor optional objectives "
                                     "(include/jslpi_tree_incremental.h)" % i)
                if not 0 <= self.max_checkpoints[i] <= _capi.JSLPI_MAX_CHECKPOINTS:
                    raise ValueError("TableauPack: LP %d: max_checkpoints is between 0 and %d" % (i, _capi.JSLPI_MAX_CHECKPOINTS))
        self.has_incremental = bool(self.is_incremental.any())
        # options.tolerance (include/jslpg_tree_tolerance.h): the values (0: none), the models' sense, the record
        self.tolerances = np.zeros(n, dtype=np.float64)
        self.minimize = np.ones(n, dtype=np.int32)
        self.tolerance = np.zeros(n, dtype=_capi.TOL_TREE_DTYPE)
        if tolerance is not None:
            if len(tolerance) != n:
                raise ValueError("TableauPack: %d tolerance entries for %d LPs" % (len(tolerance), n))
            given = _capi.as_f64([0.0 if v is None else float(v) for v in tolerance])
            self.tolerances = np.where(given > 0, given, 0.0)  # (`tolerance > 0`: false for NaN)
        if minimize is not None:
            if len(minimize) != n:
                raise ValueError("TableauPack: %d minimize flags for %d LPs" % (len(minimize), n))
            self.minimize = _capi.as_i32([int(f) for f in minimize])
            for i in np.flatnonzero((self.minimize != 0) & (self.minimize != 1)):  # (refused here, whichever library and create are behind)
                raise _capi.EngineError("jslpg_tree_pack_create failed (%d): pack_create: LP %d: minimize is 0 (the model maximises) or 1"
                                        % (_capi.JSLP_ERR_ARG, i))
        self.is_tolerance = self.tolerances > 0
        self.has_tolerance = bool(self.is_tolerance.any())
        if self.has_tolerance and not self.is_tree:
            raise ValueError("TableauPack: `tolerance` needs `integers` (a pack with trees)")
        # row_extra per LP: a MIR or an incremental LP's row capacity beyond its height (-1: any other LP, whose row capacity is height + cut_rows)
        self.row_extra = np.full(n, -1, dtype=np.int32)
        own_rows = self.is_mir | self.is_incremental
        if own_rows.any():
            if row_extra is None:
                extra = [(incremental_rows if inc else tree_mir_rows)(h, w, 0, lib=self.lib, cut_rows=c)[0] if own else -1
                         for h, w, c, inc, own in zip(self.heights, self.widths, self.cut_rows, self.is_incremental, own_rows)]
            else:
                extra = self._per_lp(row_extra, None)
                if extra.shape[0] != n:
                    raise ValueError("TableauPack: row_extra is one number or one per LP")
            self.row_extra = np.where(own_rows, _capi.as_i32(extra), -1).astype(np.int32)
            self.row_capacity = np.where(own_rows, self.heights + self.row_extra, self.row_capacity).astype(np.int32)
        self.is_enhanced = (self.node_selection != 0) | (self.branching != 0) | self.is_incremental  # (an incremental LP is walked as one)
        self.has_enhanced = bool(self.is_enhanced.any())
        for i in np.flatnonzero(self.is_enhanced):
            if self.is_mir[i] or self.n_optional[i] > 0:
                raise ValueError("TableauPack: LP %d: an enhanced LP (node_selection / branching) has neither `mir` nor optional objectives "
                                 "(include/jslpe_tree_enhanced.h)" % i)
        if self.big_lds and self.lib.has_pack and not getattr(self.lib, "has_big_lds", False):
            raise _capi.EngineError("TableauPack: %s does not export the big-LDS extension (include/jslpb_big_lds.h)" % self.lib.path)
        self.big_threads = int(self.lib.jslpb_pack_big_threads()) if getattr(self.lib, "has_big_lds", False) else 0
        # the LDS image of every LP at its row capacity (a MIR LP: with its isInteger bytes), and which LPs are large
        self.lds_bytes = np.array([tree_mir_lds_bytes(h, w, rc) if mir_lp else pack_lds_bytes(rc, w, no) for h, w, rc, no, mir_lp
                                   in zip(self.heights, self.widths, self.row_capacity, self.n_optional, self.is_mir)], dtype=np.int64).reshape(n)
        self.is_big = self.lds_bytes > _capi.JSLPP_LDS_LIMIT
        if self.has_tolerance and self.lib.has_pack and not getattr(self.lib, "has_tree_tol", False):
            raise _capi.EngineError("TableauPack: %s does not export the tolerance extension (include/jslpg_tree_tolerance.h)" % self.lib.path)
        if self.has_incremental and self.lib.has_pack and not getattr(self.lib, "has_tree_inc", False):
            raise _capi.EngineError("TableauPack: %s does not export the incremental tree extension (include/jslpi_tree_incremental.h)" % self.lib.path)
        if self.has_enhanced and self.lib.has_pack and not getattr(self.lib, "has_tree_enh", False):
            raise _capi.EngineError("TableauPack: %s does not export the enhanced tree extension (include/jslpe_tree_enhanced.h)" % self.lib.path)
        if self.has_mir and self.lib.has_pack and not getattr(self.lib, "has_tree_mir", False):
            raise _capi.EngineError("TableauPack: %s does not export the MIR tree extension (include/jslpc_tree_mir.h)" % self.lib.path)
        if self.is_tree and self.lib.has_pack and not getattr(self.lib, "has_tree", False):
            raise _capi.EngineError("TableauPack: %s does not export the tree extension (include/jslpt_tree.h)" % self.lib.path)
        if self.has_optional and self.lib.has_pack and not getattr(self.lib, "has_soft", False):
            raise _capi.EngineError("TableauPack: %s does not export the optional-objective extension (include/jslps_soft.h)" % self.lib.path)
        if self.lib.has_pack:
            self._h = _capi.C.c_void_p()
            # the pack's composition picks the entry point and the tables it takes beyond the shapes; `said` is the name an error reports
            ptr = _capi.ptr_i32
            trees = [ptr(self.cut_rows), ptr(self.heap_cap)] if self.is_tree else []
            optional = ptr(self.n_optional) if self.has_optional else None
            flags = self.is_incremental.astype(np.int32)
            big = []
            if self.big_lds and self.is_tree:  # (jslpg_tree_pack_create's tables -- the tolerance pair NULL in a pack without one -- then big_lds)
                symbol = said = "jslpb_tree_pack_create"
                tables = trees + [optional, ptr(self.row_extra), ptr(self.node_selection), ptr(self.branching), ptr(flags), ptr(self.max_checkpoints),
                                  _capi.ptr_f64(self.tolerances) if self.has_tolerance else None, ptr(self.minimize) if self.has_tolerance else None]
                big = [1]
            elif self.big_lds:
                symbol = said = "jslpb_pack_create"
                tables = [optional]
                big = [1]
            elif self.has_tolerance:
                symbol = said = "jslpg_tree_pack_create"
                tables = trees + [optional, ptr(self.row_extra), ptr(self.node_selection), ptr(self.branching), ptr(flags), ptr(self.max_checkpoints),
                                  _capi.ptr_f64(self.tolerances), ptr(self.minimize)]
            elif self.has_incremental:
                symbol = said = "jslpi_tree_pack_create"
                tables = trees + [optional, ptr(self.row_extra), ptr(self.node_selection), ptr(self.branching), ptr(flags), ptr(self.max_checkpoints)]
            elif self.has_enhanced:
                symbol, said = "jslpe_tree_pack_create_mixed", "jslpe_tree_pack_create"
                tables = trees + [optional, ptr(self.row_extra) if self.has_mir else None, ptr(self.node_selection), ptr(self.branching)]
            elif self.has_optional:
                symbol = said = "jslps_tree_pack_create" if self.is_tree else "jslps_pack_create"
                tables = trees + [optional]
            elif self.has_mir:
                symbol = said = "jslpc_tree_pack_create"
                tables = trees + [ptr(self.row_extra)]
            else:
                symbol = said = "jslpt_pack_create" if self.is_tree else "jslpp_pack_create"
                tables = trees
            caps = [self.trace_cap, self.max_pivots] + ([self.max_nodes] if self.is_tree else [])
            self.lib.check(getattr(self.lib, symbol)(_capi.C.byref(self._h), self.device, n, ptr(self.heights), ptr(self.widths), _capi.ptr_f64(self.precision),
                                                     *tables, *caps, *big), said)
            try:
                for i, (m, vibr, vibc, unr) in enumerate(self._lps):
                    self.lib.check(self.lib.jslpp_pack_set(self._h, i, _capi.ptr_f64(m), _capi.ptr_i32(vibr), _capi.ptr_i32(vibc), _capi.ptr_i32(unr),
                                                           int(unr.shape[0])), "jslpp_pack_set")
                    if self.is_tree:
                        iv = self.integers[i]
                        self.lib.check(self.lib.jslpt_pack_set_integers(self._h, i, _capi.ptr_i32(iv), int(iv.shape[0])), "jslpt_pack_set_integers")
                    if self._optional[i] is not None:
                        self.lib.check(self.lib.jslps_pack_set_optional_objectives(self._h, i, _capi.ptr_f64(self._optional[i])),
                                       "jslps_pack_set_optional_objectives")
                self._lps = None  # (the pack's pinned image holds the inputs from here on)
                self.upload()
            except Exception:
                self.close()
                raise
        elif self.lib.backend == "oracle-c":
            for i, (h, w, rc, no) in enumerate(zip(self.heights, self.widths, self.row_capacity, self.n_optional)):
                if self.is_mir[i] and self.row_extra[i] < self.cut_rows[i]:
                    raise _capi.EngineError("jslpc_tree_pack_create failed (%d): pack_create: LP %d: row_extra of a MIR LP is at least its cut_rows"
                                            % (_capi.JSLP_ERR_ARG, i))
                if self.is_mir[i] and not 0 < tree_mir_lds_bytes(h, w, rc) <= _capi.JSLPP_LDS_LIMIT:
                    raise _capi.EngineError("jslpc_tree_pack_create failed (%d): pack_create: LP %d: the MIR LP's LDS image at its row capacity "
                                            "exceeds 64 KiB" % (_capi.JSLP_ERR_UNSUPPORTED, i))
                if self.is_incremental[i] and self.row_extra[i] < self.cut_rows[i]:
                    raise _capi.EngineError("jslpi_tree_pack_create failed (%d): pack_create: LP %d: row_extra of an incremental LP is its row "
                                            "capacity beyond height: at least its cut_rows" % (_capi.JSLP_ERR_ARG, i))
                if self.is_incremental[i] and not 0 < tree_lds_bytes(h, w, rc) <= _capi.JSLPP_LDS_LIMIT:
                    raise _capi.EngineError("jslpi_tree_pack_create failed (%d): pack_create: LP %d: the incremental LP's LDS image at its row "
                                            "capacity exceeds 64 KiB" % (_capi.JSLP_ERR_UNSUPPORTED, i))
                if self.is_enhanced[i] and len(set(self.integers[i].tolist())) != self.integers[i].shape[0]:
                    raise _capi.EngineError("jslpt_pack_set_integers failed (%d): pack_set_integers: LP %d: the integer variables of an enhanced "
                                            "LP are distinct" % (_capi.JSLP_ERR_ARG, i))
                if self.big_lds:  # (include/jslpb_big_lds.h: the library's refusals, in its words)
                    said = "jslpb_tree_pack_create" if self.is_tree else "jslpb_pack_create"
                    kind = ("enhanced LP's LDS image at its row capacity" if self.is_enhanced[i] else
                            "LDS image of the LP with a tolerance" if self.is_tolerance[i] else None)
                    if kind is not None and self.is_big[i]:
                        raise _capi.EngineError("%s failed (%d): pack_create: LP %d: the %s exceeds 64 KiB" % (said, _capi.JSLP_ERR_UNSUPPORTED, i, kind))
                    if not 0 < self.lds_bytes[i] <= _capi.JSLPB_LDS_LIMIT:
                        raise _capi.EngineError("%s failed (%d): pack_create: LP %d: the tableau's LDS image%s exceeds JSLPB_LDS_LIMIT, 156 KiB"
                                                % (said, _capi.JSLP_ERR_UNSUPPORTED, i, " at its row capacity" if self.is_tree else ""))
                    continue
                if self.is_tree and not 0 < tree_lds_bytes(h, w, rc, no) <= _capi.JSLPP_LDS_LIMIT:
                    raise _capi.EngineError("jslpt_pack_create failed (%d): pack_create: LP %d: the tableau's LDS image at its row capacity exceeds "
                                            "64 KiB" % (_capi.JSLP_ERR_UNSUPPORTED, i))
                if not self.is_tree and not pack_fits(h, w, n_optional=no):
                    raise _capi.EngineError("jslpp_pack_create failed (%d): pack_create: LP %d: the tableau's LDS image exceeds 64 KiB"
                                            % (_capi.JSLP_ERR_UNSUPPORTED, i))
            self._twins = [Tableau(m, vibr, vibc, unr, precision=float(p), row_capacity=int(rc), device=self.device, lib=self.lib,
                                   optional_objectives=oo, integer_variables=self.integers[i] if self.is_mir[i] else None)
                           for i, ((m, vibr, vibc, unr), p, rc, oo) in enumerate(zip(self._lps, self.precision, self.row_capacity, self._optional))]
        else:
            raise _capi.EngineError("TableauPack: %s does not export the pack extension (include/jslpp_packed.h)" % self.lib.path)

    def _per_lp(self, v, default):
        """one number or one per LP as an int32 array (its length is the caller's to check); None: the default"""
        return _capi.as_i32(default if v is None else ([v] * self.n if isinstance(v, (int, np.integer)) else list(v)))

    # ---- lifetime -------------------------------------------------------------------------------
    def close(self):
        if self._h is not None and self._h.value:
            self.lib.jslpp_pack_destroy(self._h)
        self._h = None
        for t in self._twins or ():
            t.close()
        self._twins = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.n

    @property
    def launches(self):
        """kernel launches of the last simplex(): at most one per kernel build (0 for the restatement)"""
        return self._launches

    def upload(self):
        """hand the LPs over again as they were given: one H2D copy; every LP's state, evaluation, counters and trace start afresh"""
        if self._twins is not None:
            for t, (m, vibr, vibc, unr), oo in zip(self._twins, self._lps, self._optional):
                t.upload(m, vibr, vibc, unr)
                if oo is not None:  # (an engine's upload keeps the rows it has: hand the LP's own over again)
                    self.lib.check(self.lib.jslp_engine_set_optional_objectives(t._h, int(oo.shape[0]), _capi.ptr_f64(oo)),
                                   "jslp_engine_set_optional_objectives")
                if t.integer_variables:  # (a MIR LP's variable.isInteger: an engine's upload forgets it with the model it replaces)
                    iv = _capi.as_i32(sorted(t.integer_variables))
                    self.lib.check(self.lib.jslp_engine_set_integer_variables(t._h, _capi.ptr_i32(iv), int(iv.shape[0])),
                                   "jslp_engine_set_integer_variables")
                t.evaluation, t.feasible, t.bounded = 0.0, True, True
        else:
            self.lib.check(self.lib.jslpp_pack_upload(self._h), "jslpp_pack_upload")
        self.evaluation[:] = 0.0
        self.feasible[:] = True
        self.bounded[:] = True

    def _flags(self, check_cycles):
        if isinstance(check_cycles, (bool, int, np.bool_)):
            return np.full(self.n, int(bool(check_cycles)), dtype=np.int32)
        flags = _capi.as_i32([int(bool(c)) for c in check_cycles])
        if flags.shape[0] != self.n:
            raise ValueError("TableauPack.simplex: %d check_cycles flags for %d LPs" % (flags.shape[0], self.n))
        return flags

    def simplex(self, check_cycles=True):
        """Tableau.simplex() of every LP.  An LP whose solve fails (pivot cap, history capacity) keeps its earlier result and scalars and gets
        the engine's code in `status`; the others are solved; the call then raises EngineError naming the first such LP."""
        flags = self._flags(check_cycles)
        out = self.results.copy()
        status = np.zeros(self.n, dtype=np.int32)
        if self._twins is not None:
            rc, msg = _capi.JSLP_OK, ""
            for i, (t, c) in enumerate(zip(self._twins, flags)):
                res = SimplexResult()
                st = self.lib.jslp_engine_simplex(t._h, int(c), _capi.C.byref(res))
                status[i] = st
                if st == _capi.JSLP_OK:
                    t._absorb(res)
                    out[i] = np.frombuffer(res, dtype=_capi.RESULT_DTYPE)[0]
                elif rc == _capi.JSLP_OK:
                    rc, msg = st, "pack_simplex: LP %d: %s" % (i, self.lib.jslp_last_error().decode())
            self._launches = 0
        else:
            ms = _capi.C.c_double()
            all_same = bool((flags == flags[0]).all()) if self.n else True
            rc = self.lib.jslpp_pack_simplex(self._h, None if (all_same and self.n and flags[0]) else _capi.ptr_i32(flags), out.ctypes.data,
                                             _capi.ptr_i32(status), _capi.C.byref(ms))
            msg = self.lib.jslp_last_error().decode() if rc != _capi.JSLP_OK else ""
            if rc != _capi.JSLP_OK and not status.any():  # refused before any work
                raise _capi.EngineError("jslpp_pack_simplex failed (%d): %s" % (rc, msg))
            self.device_ms = ms.value
            self._launches = int(self.lib.jslpp_pack_launches(self._h))
        return self._keep(out, status, rc, msg, "jslpp_pack_simplex")

    def _keep(self, out, status, rc, msg, what):
        """the end of simplex() and branch_and_cut(): the results and the scalars of the LPs that were solved (an LP that failed leaves its own
        alone, as Tableau.simplex() does), then the call's error"""
        ok = status == _capi.JSLP_OK
        self.results = out
        self.status = status
        self.feasible[ok] = out["feasible"][ok] != 0
        self.bounded[ok] = out["bounded"][ok] != 0
        self.evaluation[ok] = out["evaluation"][ok]
        if rc != _capi.JSLP_OK:
            raise _capi.EngineError("%s failed (%d): %s" % (what, rc, msg))
        return out

    def _walk(self, i, t, check_cycles):
        """the restatement's tree of LP i on its twin engine `t`: the LP's (tree, mir, enhanced, incremental, tolerance) records"""
        from . import branch_and_cut as bc
        from . import incremental_branch_and_cut as ibc
        none_mir, none_enh, none_inc = (0, 0, 0, 0, 0), (0,) * 8, (0,) * 8
        t.simplexIters, t.bestPossibleEval = 0, 0.0  # (every call starts a Tableau.solve() of its own: tableau.ts:61, 87)
        tol = {}
        # (a NaN threshold -- 0 * Infinity -- is reported as THE quiet NaN, as jslpg_pack_read_tolerance reports it: its sign is the multiplier's whim)
        canon = lambda x: float("nan") if x != x else x  # noqa: E731
        tol_rec = lambda: (tol.get("best_possible", 0.0), canon(tol.get("threshold", 0.0)), tol.get("stopped", 0), tol.get("left", 0), 0, 0)  # noqa: E731
        if self.integers[i].shape[0] == 0:
            t.simplex(check_cycles=bool(check_cycles))
            if self.is_tolerance[i]:  # (the kernel's one turn: the threshold of the root's turn, bestPossibleEval from its simplex)
                tol.update(best_possible=float(t.bestPossibleEval), threshold=0.0 * self._factor(i))
            return (0, 0, t.last.height, 0, 0, 0), (0, 0, 1, 0, 0) if self.is_mir[i] else none_mir, none_enh, none_inc, tol_rec()
        model = _TreeModel(self.integers[i], check_cycles, mir=bool(self.is_mir[i]), tolerance=float(self.tolerances[i]),
                           minimize=bool(self.minimize[i]))
        if self.is_enhanced[i]:  # the enhanced or the incremental service on the LP's twin, its stack and heap sharing heap_cap
            boxes = ibc.CountingContainers(heap_cap=int(self.heap_cap[i]), cut_rows=int(self.cut_rows[i]), max_nodes=self.max_nodes)
            selection, rule = self.policy(i)
            if self.is_incremental[i]:  # (its checkpoints are the engine's)
                iterations, integral = ibc.incremental_branch_and_cut(t, model, node_selection=selection, branching=rule,
                                                                      max_checkpoints=int(self.max_checkpoints[i]), containers=boxes,
                                                                      tolerance_out=tol)
                inc_rec = (t.checkpoints_used, t.incremental_nodes, max(boxes.rows_high_water - t.height0, 0),
                           max(boxes.checkpoint_rows_high_water - t.height0, 0), 0, 0, 0, 0)
            else:
                iterations, integral = ibc.enhanced_branch_and_cut(t, model, node_selection=selection, branching=rule, containers=boxes,
                                                                   tolerance_out=tol)
                inc_rec = none_inc
            return ((iterations, int(integral), t.last.height, boxes.pushes, boxes.high_water, boxes.cuts_high_water), none_mir,
                    boxes.record() + (0, 0), inc_rec, tol_rec())
        heap = bc.CountingHeap(heap_cap=int(self.heap_cap[i]), cut_rows=int(self.cut_rows[i]))
        counters = _MirCounters(t) if self.is_mir[i] else None
        try:
            iterations, integral = bc.branch_and_cut(t, model, heap=heap, max_nodes=self.max_nodes, tolerance_out=tol)
            return ((iterations, int(integral), t.last.height, heap.pushes, heap.high_water, heap.cuts_high_water),
                    counters.record() if counters is not None else none_mir, none_enh, none_inc, tol_rec())
        finally:
            if counters is not None:
                counters.detach()

    def _factor(self, i):
        """acceptableThreshold / bestPossibleEval of LP i (branch-and-cut.ts:77-81)"""
        return 1 + float(self.tolerances[i]) if self.minimize[i] else 1 - float(self.tolerances[i])

    def branch_and_cut(self, check_cycles=True):
        """Tableau.solve() of every LP under the default branch-and-cut service, each tree walked by its LP's workgroup inside ONE launch per
        kernel build (include/jslpt_tree.h).  Returns the results like simplex() -- per LP the last relaxation evaluated -- and keeps `tree`
        (_capi.TREE_DTYPE: iterations, is_integral, final_height, nodes_pushed, heap_high_water, cuts_high_water), `status`, `evaluation`,
        `feasible` and `bounded`.  An LP that reaches a capacity keeps its earlier entries and gets JSLP_ERR_CAPACITY in `status`; the others
        are solved; the call then raises EngineError naming the first such LP.  The restatement walks branch_and_cut.branch_and_cut on one
        engine per LP with the same capacities enforced (max_pivots excepted: the engine's own cap).
        A MIR LP (`mir=`) runs every node's MIR loop, in the kernel as in the restatement (round by round, mirRound); `mir` keeps its
        counters; its capacities are the row capacity (`row_extra` in the message) and JSLPR_MAX_ROUNDS rounds of one node (`mir rounds`).
        An enhanced LP (`node_selection=` / `branching=`) is walked under the enhanced service, in the kernel as in the restatement
        (incremental_branch_and_cut.enhanced_branch_and_cut with CountingContainers); `enhanced` keeps its counters; in `tree` its
        heap_high_water counts stack and heap together and nodes_pushed the new branches.
        An incremental LP (`incremental=`) is walked under the incremental service, in the kernel as in the restatement
        (incremental_branch_and_cut.incremental_branch_and_cut with CountingContainers, the checkpoints being the twin engine's);
        `incremental` keeps its counters; a row that does not fit its row capacity is the capacity `row_extra`.
        An LP with a tolerance (`tolerance=`) ends its walk on the reference's toleranceFlag, in the kernel as in the restatement (the three
        host walks with the LP's tolerance and sense); `tolerance` keeps its record."""
        if not self.is_tree:
            raise _capi.EngineError("TableauPack.branch_and_cut: the pack was made without `integers`")
        flags = self._flags(check_cycles)
        out = self.results.copy()
        tree = self.tree.copy()
        mir = self.mir.copy()
        enhanced = self.enhanced.copy()
        incremental = self.incremental.copy()
        tolerance = self.tolerance.copy()
        status = np.zeros(self.n, dtype=np.int32)
        if self._twins is not None:
            from . import branch_and_cut as bc
            rc, msg = _capi.JSLP_OK, ""
            for i, (t, c) in enumerate(zip(self._twins, flags)):
                try:
                    tree[i], mir[i], enhanced[i], incremental[i], tolerance[i] = self._walk(i, t, c)
                    res = SimplexResult.from_buffer_copy(bytes(t.last))
                    res.evaluation = t.evaluation
                    out[i] = np.frombuffer(res, dtype=_capi.RESULT_DTYPE)[0]
                except (bc.TreeCapacity, _capi.EngineError) as e:
                    status[i] = _capi.JSLP_ERR_CAPACITY if isinstance(e, bc.TreeCapacity) or "(%d)" % _capi.JSLP_ERR_CAPACITY in str(e) else _capi.JSLP_ERR_DEVICE
                    if (self.is_mir[i] or self.is_incremental[i]) and "row capacity exceeded" in str(e):  # (an engine's refusal of a round's or a cut list's rows)
                        e = "branch_and_cut: row_extra reached (%s)" % e
                    if rc == _capi.JSLP_OK:
                        rc, msg = int(status[i]), "pack_branch_and_cut: LP %d: %s" % (i, e)
            self._launches = 0
        else:
            ms = _capi.C.c_double()
            all_same = bool((flags == flags[0]).all()) if self.n else True
            rc = self.lib.jslpt_pack_branch_and_cut(self._h, None if (all_same and self.n and flags[0]) else _capi.ptr_i32(flags), out.ctypes.data,
                                                    tree.ctypes.data, _capi.ptr_i32(status), _capi.C.byref(ms))
            msg = self.lib.jslp_last_error().decode() if rc != _capi.JSLP_OK else ""
            if rc != _capi.JSLP_OK and not status.any():  # refused before any work
                raise _capi.EngineError("jslpt_pack_branch_and_cut failed (%d): %s" % (rc, msg))
            self.device_ms = ms.value
            self._launches = int(self.lib.jslpp_pack_launches(self._h))
            if self.has_mir:
                self.lib.check(self.lib.jslpc_pack_read_mir(self._h, mir.ctypes.data), "jslpc_pack_read_mir")
            if self.has_enhanced:
                self.lib.check(self.lib.jslpe_pack_read_enhanced(self._h, enhanced.ctypes.data), "jslpe_pack_read_enhanced")
            if self.has_incremental:
                self.lib.check(self.lib.jslpi_pack_read_incremental(self._h, incremental.ctypes.data), "jslpi_pack_read_incremental")
            if self.has_tolerance:
                self.lib.check(self.lib.jslpg_pack_read_tolerance(self._h, tolerance.ctypes.data), "jslpg_pack_read_tolerance")
            else:  # (zeros for every LP that was solved, as the read-back and the restatement give an LP without tolerance)
                tolerance[status == _capi.JSLP_OK] = np.zeros((), dtype=_capi.TOL_TREE_DTYPE)
        self.tree, self.mir, self.enhanced, self.incremental, self.tolerance = tree, mir, enhanced, incremental, tolerance
        return self._keep(out, status, rc, msg, "jslpt_pack_branch_and_cut")

    def policy(self, i):
        """(node selection, branching) LP i's tree is walked under, by name, with the defaults filled in; None for an LP under the default
        service"""
        if not self.is_enhanced[i]:
            return None
        names = lambda table, code, default: next(k for k, v in table.items() if v == (code or table[default]))  # noqa: E731
        return (names(_capi.ENH_NODE_SELECTION, int(self.node_selection[i]), "hybrid"),
                names(_capi.ENH_BRANCHING, int(self.branching[i]), "pseudocost"))

    def result(self, i):
        """LP i's result of the last simplex() as a SimplexResult"""
        return SimplexResult.from_buffer_copy(self.results[i].tobytes())

    # ---- read-back --------------------------------------------------------------------------------
    def read_rhs(self, i):
        """RHS column and varIndexByRow of LP i after the last simplex() (copies; native: out of the pack's pinned result block)"""
        if self._twins is not None:
            return self._twins[i].read_rhs()
        rhs, rows, offs = _capi._f64p(), _capi._i32p(), _capi._P(_capi.C.c_int64)()
        self.lib.check(self.lib.jslpp_pack_read_rhs(self._h, _capi.C.byref(rhs), _capi.C.byref(rows), _capi.C.byref(offs)), "jslpp_pack_read_rhs")
        a, b = int(offs[i]), int(offs[i + 1])
        if self.is_tree:  # (the LP's block is sized by its row capacity: the final tableau's rows are valid)
            b = a + int(self.results[i]["height"])
        return (np.ctypeslib.as_array(rhs, shape=(int(offs[self.n]),))[a:b].copy(),
                np.ctypeslib.as_array(rows, shape=(int(offs[self.n]),))[a:b].copy())

    def optional_objectives(self, i):
        """LP i's optional objectives after the last solve (n_optional x width; native: out of the pack's pinned result block)"""
        no, w = int(self.n_optional[i]), int(self.widths[i])
        if self._twins is not None:
            return self._twins[i].optional_objectives()[:no].copy()
        rows = np.zeros((no, w), dtype=np.float64)
        if self.has_optional:
            n = _capi.C.c_int32()
            self.lib.check(self.lib.jslps_pack_get_optional_objectives(self._h, int(i), _capi.ptr_f64(rows) if no else None, _capi.C.byref(n)),
                           "jslps_pack_get_optional_objectives")
        return rows

    def download(self, i):
        if self._twins is not None:
            return self._twins[i].download()
        h, w = int(self.heights[i]), int(self.widths[i])
        n = w + 2 * int(self.row_capacity[i]) + 2  # (the maps are sized for the LP's row capacity)
        m = np.empty((h, w), dtype=np.float64)
        vibr, vibc = np.empty(h, dtype=np.int32), np.empty(w, dtype=np.int32)
        rbv, cbv = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        self.lib.check(self.lib.jslpp_pack_download(self._h, int(i), _capi.ptr_f64(m), _capi.ptr_i32(vibr), _capi.ptr_i32(vibc), _capi.ptr_i32(rbv),
                                                    _capi.ptr_i32(cbv)), "jslpp_pack_download")
        return m, vibr, vibc, rbv, cbv

    def pivot_trace(self, i):
        if self._twins is not None:
            return self._twins[i].pivot_trace()
        n = _capi.C.c_int64()
        self.lib.check(self.lib.jslpp_pack_pivot_trace(self._h, int(i), None, 0, _capi.C.byref(n)), "jslpp_pack_pivot_trace")
        buf = np.empty(2 * max(n.value, 1), dtype=np.int32)
        self.lib.check(self.lib.jslpp_pack_pivot_trace(self._h, int(i), _capi.ptr_i32(buf), n.value, _capi.C.byref(n)), "jslpp_pack_pivot_trace")
        return buf[:2 * n.value].reshape(-1, 2)
