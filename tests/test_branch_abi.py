"""The branch-record extension's boundary (no compute, runs without a GPU): include/jslpx_branch.h, the ctypes table BRANCH_SYMBOLS and the
jslpx_ exports of the product and test libraries agree; the extension stays out of jslp_engine.h and the oracle; and on the CPU the oracle's
records (restated from its compact read-back) keep the layout and the JSLP_ERR_ARG contract of the HIP entry points."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from jslpsolver_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslpx_branch.h")
CHAOS = os.path.join(ROOT, "jslpsolver_amd", "csrc", "libjslp_hip_chaos.so")


def declared_in_header(path=HEADER, prefix="jslpx_"):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, text))


def exported(path, prefix="jslpx_"):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith(prefix)}


def built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def test_header_and_binding_declare_the_same_extension():
    assert declared_in_header() == set(_capi.BRANCH_SYMBOLS)
    assert len(_capi.BRANCH_SYMBOLS) == 5
    assert not declared_in_header(os.path.join(ROOT, "include", "jslp_engine.h"))  # the drop-in boundary stays as it is
    assert not set(_capi.BRANCH_SYMBOLS) & set(_capi.SYMBOLS)


def test_product_and_test_libraries_export_the_extension():
    assert exported(built(_capi.HIP_LIB_PATH)) == declared_in_header()
    assert exported(built(CHAOS)) == declared_in_header()


def test_oracle_does_not_export_the_extension(oracle_lib):
    assert exported(oracle_lib.path) == set()
    assert not oracle_lib.has_branch


def test_record_layout():
    assert ctypes.sizeof(_capi.BranchRecord) == 32 == _capi.BRANCH_RECORD_DTYPE.itemsize
    assert [(n, _capi.BranchRecord.__dict__[n].offset) for n, _ in _capi.BranchRecord._fields_] == \
        [(n, _capi.BRANCH_RECORD_DTYPE.fields[n][1]) for n in _capi.BRANCH_RECORD_DTYPE.names]
    lib = _capi.Library(built(_capi.HIP_LIB_PATH))
    assert lib.has_branch and lib.jslpx_branch_record_bytes() == 32
    text = open(HEADER).read()
    assert re.search(r"JSLPX_BRANCH_FEASIBLE 1\b", text) and re.search(r"JSLPX_BRANCH_INTEGRAL 8\b", text)


def test_hip_entry_points_without_watched_variables_fail_with_err_arg():
    """no engine needs to exist for the argument checks: a null engine is refused with JSLP_ERR_ARG, never dereferenced"""
    lib = _capi.Library(built(_capi.HIP_LIB_PATH))
    recs = np.zeros(1, dtype=_capi.BRANCH_RECORD_DTYPE)
    offs = np.zeros(2, dtype=np.int32)
    assert lib.jslpx_engine_relax_batch_branch(None, 1, _capi.ptr_i32(offs), None, None, None, 1, recs.ctypes.data) == _capi.JSLP_ERR_ARG
    assert lib.jslpx_engine_relax_batch_branch_device(None, 1, _capi.ptr_i32(offs), None, None, None, 1, None) == _capi.JSLP_ERR_ARG
    assert lib.jslpx_engine_results_from_branch_records(None, None, 1, None) == _capi.JSLP_ERR_ARG


def _small_milp_tableau(lib):
    from jslpsolver_amd.engine import Tableau
    from jslpsolver_amd.model import Model
    model = {"optimize": "v", "opType": "max", "constraints": {"a": {"max": 10.5}, "b": {"max": 7.25}},
             "variables": {"x": {"v": 3, "a": 2, "b": 1}, "y": {"v": 2, "a": 1, "b": 1}}, "ints": {"x": 1, "y": 1}}
    m = Model(model)
    matrix, vibr, vibc = m.build_tableau()
    t = Tableau(matrix, vibr, vibc, m.unrestricted, precision=m.precision, row_capacity=matrix.shape[0] + 8, lib=lib)
    return t, m


def test_oracle_records_need_watched_variables(oracle_lib):
    t, m = _small_milp_tableau(oracle_lib)
    t.applyCuts([])
    t.save()
    with pytest.raises(_capi.EngineError, match=r"\(-1\)"):
        t.applyCutsBatchBranch([[]])
    t.close()


def test_oracle_records_restate_the_compact_read_back(oracle_lib):
    """the CPU form of the records: branch_record_from_watched over the oracle's compact read-back, and the same decisions as the
    tree's own isIntegral / most_fractional_var on the full read-back of the same nodes"""
    from jslpsolver_amd.branch_and_cut import _rows_by_var, is_integral, most_fractional_var
    t, m = _small_milp_tableau(oracle_lib)
    t.applyCuts([])
    t.save()
    t.set_watched_variables(m.integer_index_array)
    x = int(m.integer_index_array[0])
    nodes = [[], [{"type": "max", "varIndex": x, "value": 3.0}], [{"type": "min", "varIndex": x, "value": 4.0}],
             [{"type": "min", "varIndex": x, "value": 40.0}]]  # the last one is infeasible
    results, recs = t.applyCutsBatchBranch(nodes)
    assert recs.dtype == _capi.BRANCH_RECORD_DTYPE and len(recs) == len(nodes) == len(results)
    full, rhs, vibr = t.applyCutsBatch(nodes)
    for i in range(len(nodes)):
        h = full[i].height
        assert recs["height"][i] == h and results[i].height == h
        assert bool(recs["flags"][i] & _capi.BRANCH_FEASIBLE) == bool(full[i].feasible)
        assert results[i].optimal == full[i].optimal and (not full[i].optimal or results[i].evaluation == full[i].evaluation)
        rows = _rows_by_var(vibr[i, :h])
        assert bool(recs["flags"][i] & _capi.BRANCH_INTEGRAL) == is_integral(m, rhs[i, :h], rows, t.precision)
        k, v = most_fractional_var(m, rhs[i, :h], rows)
        assert recs["branch_var_index"][i] == (-1 if k is None else k)
        assert np.float64(recs["branch_var_value"][i]).view(np.int64) == np.float64(v).view(np.int64)
    assert not recs["flags"][3] & _capi.BRANCH_FEASIBLE
    t.close()


def test_hip_library_without_the_extension_raises(oracle_lib, monkeypatch):
    """a HIP library that lacks the jslpx_ symbols is an error, never a quiet fall-back to the restatement"""
    t, m = _small_milp_tableau(oracle_lib)
    monkeypatch.setattr(type(oracle_lib), "backend", property(lambda self: "hip-gfx950"))
    with pytest.raises(_capi.EngineError, match="branch-record extension"):
        t.applyCutsBatchBranch([[]])
    monkeypatch.undo()
    t.close()
