"""The fp32 sweep extension's boundary (runs without a GPU): include/jslpf_f32.h, the ctypes table F32_SYMBOLS and the jslpf_ exports of the
product and test libraries agree; the extension stays out of jslp_engine.h, out of the oracle and apart from the other tables; the
argument checks of jslpf_simplex_f32_sweep refuse bad calls before touching a device; Tableau.simplex_f32_sweep on the oracle raises."""
import ctypes
import os

import numpy as np
import pytest

from jslpsolver_amd import _capi
from jslpsolver_amd.engine import Tableau
from test_many_abi import CHAOS, ROOT, built, declared_in_header, exported

HEADER = os.path.join(ROOT, "include", "jslpf_f32.h")


def test_header_and_binding_declare_the_same_extension():
    assert declared_in_header(HEADER, "jslpf_") == set(_capi.F32_SYMBOLS) == {"jslpf_simplex_f32_sweep"}
    assert not declared_in_header(os.path.join(ROOT, "include", "jslp_engine.h"), "jslpf_")  # the drop-in boundary stays as it is
    assert "jslpf_" not in open(os.path.join(ROOT, "include", "jslp_engine.h")).read()
    for other in (_capi.SYMBOLS, _capi.BRANCH_SYMBOLS, _capi.MANY_SYMBOLS):
        assert not set(_capi.F32_SYMBOLS) & set(other)
    text = open(HEADER).read()
    for name, value in (("JSLPF_PATH_AUTO", _capi.JSLPF_PATH_AUTO), ("JSLPF_PATH_SELECT_UPDATE", _capi.JSLPF_PATH_SELECT_UPDATE),
                        ("JSLPF_PATH_ONE_LAUNCH", _capi.JSLPF_PATH_ONE_LAUNCH), ("JSLPF_MAX_RUNS", _capi.JSLPF_MAX_RUNS)):
        assert ("#define %s " % name) in text and int(text.split("#define %s " % name)[1].split()[0]) == value
    assert (_capi.JSLPF_PATH_AUTO, _capi.JSLPF_PATH_SELECT_UPDATE, _capi.JSLPF_PATH_ONE_LAUNCH, _capi.JSLPF_MAX_RUNS) == (0, 1, 2, 64)


def test_product_and_test_libraries_export_the_extension():
    assert exported(built(_capi.HIP_LIB_PATH), "jslpf_") == declared_in_header(HEADER, "jslpf_")
    assert exported(built(CHAOS), "jslpf_") == declared_in_header(HEADER, "jslpf_")
    assert _capi.Library(_capi.HIP_LIB_PATH).has_f32
    assert _capi.Library(CHAOS).has_f32


def test_oracle_does_not_export_the_extension(oracle_lib):
    assert exported(oracle_lib.path, "jslpf_") == set()
    assert not oracle_lib.has_f32
    assert "jslpf_" not in open(os.path.join(ROOT, "oracle", "jslp_oracle.c")).read()


def _call(lib, e, precisions, n, path=_capi.JSLPF_PATH_AUTO, out=True):
    prec = None if precisions is None else _capi.ptr_f64(_capi.as_f64(precisions))
    res = (_capi.SimplexResult * 64)() if out else None
    taken = ctypes.c_int32(-7)
    ms = ctypes.c_double(-7.0)
    rc = lib.jslpf_simplex_f32_sweep(e, prec, n, 1, path, res, None, None, 0, None, ctypes.byref(taken), ctypes.byref(ms))
    assert (taken.value, ms.value) == (-7, -7.0), "a refused call writes nothing"
    return rc


def test_argument_errors_without_a_device():
    """each refused with its code before any engine is looked at or any device touched: the engine here is NULL throughout"""
    lib = _capi.Library(built(_capi.HIP_LIB_PATH))
    ok = [1e-3, 1e-5]
    assert _call(lib, None, ok, -1) == _capi.JSLP_ERR_ARG
    assert _call(lib, None, [1e-5] * 65, 65) == _capi.JSLP_ERR_ARG
    assert _call(lib, None, None, 2) == _capi.JSLP_ERR_ARG
    assert _call(lib, None, ok, 2, out=False) == _capi.JSLP_ERR_ARG
    for path in (-1, 3, 99):
        assert _call(lib, None, ok, 2, path=path) == _capi.JSLP_ERR_ARG
        assert b"path" in lib.jslp_last_error()
    for bad in (0.0, -1e-5, float("nan")):
        assert _call(lib, None, [1e-3, bad], 2) == _capi.JSLP_ERR_ARG
        assert b"run 1" in lib.jslp_last_error()
    # nothing to do is no error, whatever the engine; bad arguments still are
    assert _call(lib, None, None, 0, out=False) == _capi.JSLP_OK
    assert _call(lib, None, None, 0, path=7, out=False) == _capi.JSLP_ERR_ARG
    # a null engine: the engine state is wrong, not the arguments
    assert _call(lib, None, ok, 2) == _capi.JSLP_ERR_STATE
    assert _call(lib, None, [1e-5] * 64, 64) == _capi.JSLP_ERR_STATE
    assert b"null engine" in lib.jslp_last_error()


def test_sweep_on_the_oracle_raises(oracle_lib):
    m = np.array([[0.0, 3.0, 2.0], [4.0, 1.0, 1.0], [6.0, 1.0, 3.0]])
    t = Tableau(m, np.array([-1, 2, 3], dtype=np.int32), np.array([-1, 0, 1], dtype=np.int32), lib=oracle_lib)
    with pytest.raises(_capi.EngineError, match=r"include/jslpf_f32\.h"):
        t.simplex_f32_sweep([1e-3, 1e-5])
    t.close()
