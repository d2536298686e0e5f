"""The pack extension's boundary (runs without a GPU): include/jslpp_packed.h, the ctypes table PACK_SYMBOLS and the jslpp_ exports of the
product and test libraries agree; the extension stays out of jslp_engine.h, out of the oracle and apart from the other tables; create
refuses bad arguments and tableaus beyond the LDS limit before touching a device; jslpp_lds_bytes is a pure, monotone function."""
import ctypes
import os

import numpy as np

from jslpsolver_amd import _capi
from jslpsolver_amd.engine import pack_fits, pack_lds_bytes
from test_many_abi import built, declared_in_header, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslpp_packed.h")
CHAOS = os.path.join(ROOT, "jslpsolver_amd", "csrc", "libjslp_hip_chaos.so")
PREFIX = "jslpp_"


def _hip():
    return _capi.Library(built(_capi.HIP_LIB_PATH))


def test_header_and_binding_declare_the_same_extension():
    declared = declared_in_header(HEADER, PREFIX)
    assert declared == set(_capi.PACK_SYMBOLS) and len(declared) == 12
    assert not declared_in_header(os.path.join(ROOT, "include", "jslp_engine.h"), PREFIX)  # the drop-in boundary stays as it is
    for other in (_capi.SYMBOLS, _capi.MANY_SYMBOLS, _capi.BRANCH_SYMBOLS, _capi.F32_SYMBOLS, _capi.MIR_SYMBOLS):
        assert not set(_capi.PACK_SYMBOLS) & set(other)


def test_product_and_test_libraries_export_the_extension():
    assert exported(built(_capi.HIP_LIB_PATH), PREFIX) == declared_in_header(HEADER, PREFIX)
    assert exported(built(CHAOS), PREFIX) == declared_in_header(HEADER, PREFIX)
    assert _hip().has_pack


def test_oracle_does_not_export_the_extension(oracle_lib):
    assert exported(oracle_lib.path, PREFIX) == set()
    assert not oracle_lib.has_pack


def _create(lib, n, heights, widths, precisions, trace_cap=0, max_pivots=0):
    h = ctypes.c_void_p()
    hs = None if heights is None else _capi.ptr_i32(_capi.as_i32(heights))
    ws = None if widths is None else _capi.ptr_i32(_capi.as_i32(widths))
    ps = None if precisions is None else _capi.ptr_f64(_capi.as_f64(precisions))
    rc = lib.jslpp_pack_create(ctypes.byref(h), 0, n, hs, ws, ps, trace_cap, max_pivots)
    return rc, h


def test_argument_errors_without_a_device():
    """refused before any device call: this host has no GPU, and a call that reached the device would answer JSLP_ERR_DEVICE"""
    lib = _hip()
    assert _create(lib, -1, [3], [3], [1e-8])[0] == _capi.JSLP_ERR_ARG
    assert _create(lib, 1, None, [3], [1e-8])[0] == _capi.JSLP_ERR_ARG
    assert _create(lib, 1, [3], None, [1e-8])[0] == _capi.JSLP_ERR_ARG
    assert _create(lib, 1, [3], [3], None)[0] == _capi.JSLP_ERR_ARG
    assert lib.jslpp_pack_create(None, 0, 1, None, None, None, 0, 0) == _capi.JSLP_ERR_ARG
    assert _create(lib, 2, [3, 1], [3, 3], [1e-8, 1e-8])[0] == _capi.JSLP_ERR_ARG
    assert b"LP 1" in lib.jslp_last_error()
    assert _create(lib, 2, [3, 3], [1, 3], [1e-8, 1e-8])[0] == _capi.JSLP_ERR_ARG
    assert b"LP 0" in lib.jslp_last_error()
    assert _create(lib, 1, [3], [3], [1e-8], trace_cap=-1)[0] == _capi.JSLP_ERR_ARG
    assert _create(lib, 1, [3], [3], [1e-8], max_pivots=-1)[0] == _capi.JSLP_ERR_ARG
    # Sudoku4x4's shape does not fit: the refusal names the LP, and nothing was created
    rc, h = _create(lib, 3, [3, 4, 193], [3, 4, 65], [1e-8] * 3)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and not h.value
    assert b"LP 2" in lib.jslp_last_error() and b"64 KiB" in lib.jslp_last_error()
    rc, h = _create(lib, 1, [2 ** 20], [2 ** 20], [1e-8])  # (a byte count that would not fit 32 bits)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and b"LP 0" in lib.jslp_last_error()
    # the other entry points refuse a null pack
    assert lib.jslpp_pack_upload(None) == _capi.JSLP_ERR_ARG
    assert lib.jslpp_pack_simplex(None, None, None, None, None) == _capi.JSLP_ERR_ARG
    assert lib.jslpp_pack_size(None) == 0 and lib.jslpp_pack_launches(None) == 0
    lib.jslpp_pack_destroy(None)


def test_lds_bytes_is_pure_and_monotone():
    lib = _hip()
    assert lib.jslpp_lds_bytes(193, 65) > 65536  # Sudoku4x4
    assert lib.jslpp_lds_bytes(36, 101) <= 65536  # the LargeFarmMIP root
    assert lib.jslpp_lds_bytes(1, 5) == 0 and lib.jslpp_lds_bytes(5, 1) == 0
    sizes = list(range(2, 70)) + [87, 88, 100, 128, 129, 193, 256, 257, 1024, 1025]
    table = np.array([[lib.jslpp_lds_bytes(h, w) for w in sizes] for h in sizes], dtype=np.int64)
    assert (table > 0).all() and (table % 16 == 0).all()
    assert (np.diff(table, axis=0) > 0).all()   # a row more always costs
    assert (np.diff(table, axis=1) >= 0).all()  # a column more never saves (the odd stride makes W and W + 1 equal for even W)
    assert (table[:, -1] > table[:, 0]).all()
    # every cell of the tableau is in it, and the padding stays small
    for h, w in ((2, 2), (3, 3), (64, 64), (87, 87), (36, 101), (257, 20), (20, 257)):
        b = lib.jslpp_lds_bytes(h, w)
        assert 8 * h * w < b <= 8 * h * (w + 2) + 16 * (w + 3 * h + 2) + 128
    # the Python restatement the oracle path routes by
    for h in sizes:
        for w in sizes:
            assert pack_lds_bytes(h, w) == lib.jslpp_lds_bytes(h, w)
    assert pack_fits(87, 87) and not pack_fits(88, 88) and not pack_fits(193, 65) and not pack_fits(1, 9)
