"""The optional-objective extension's boundary (runs without a GPU): include/jslps_soft.h, the ctypes table SOFT_SYMBOLS and the jslps_
exports of the product and test libraries agree, and the extension stays out of every other header and table; the byte counts are pure,
monotone functions that equal the pack's own at n_optional == 0 and that engine.py restates; create refuses a negative count and an LP
that its optional rows push beyond the LDS limit before touching a device."""
import ctypes
import os

import numpy as np

from jslpsolver_amd import _capi
from jslpsolver_amd.engine import pack_fits, pack_lds_bytes, tree_cut_rows, tree_lds_bytes
from test_many_abi import built, declared_in_header, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslps_soft.h")
CHAOS = os.path.join(ROOT, "jslpsolver_amd", "csrc", "libjslp_hip_chaos.so")
PREFIX = "jslps_"
LIMIT = 65536


def _hip():
    return _capi.Library(built(_capi.HIP_LIB_PATH))


def test_header_and_binding_declare_the_same_extension():
    declared = declared_in_header(HEADER, PREFIX)
    assert declared == set(_capi.SOFT_SYMBOLS) and len(declared) == 6
    for other in ("jslp_engine.h", "jslpp_packed.h", "jslpt_tree.h"):
        assert not declared_in_header(os.path.join(ROOT, "include", other), PREFIX)
    for other in (_capi.SYMBOLS, _capi.MANY_SYMBOLS, _capi.BRANCH_SYMBOLS, _capi.F32_SYMBOLS, _capi.MIR_SYMBOLS, _capi.PACK_SYMBOLS, _capi.TREE_SYMBOLS):
        assert not set(_capi.SOFT_SYMBOLS) & set(other)


def test_product_and_test_libraries_export_the_extension(oracle_lib):
    assert exported(built(_capi.HIP_LIB_PATH), PREFIX) == declared_in_header(HEADER, PREFIX)
    assert exported(built(CHAOS), PREFIX) == declared_in_header(HEADER, PREFIX)
    assert _hip().has_soft
    assert exported(oracle_lib.path, PREFIX) == set() and not oracle_lib.has_soft


SIZES = list(range(2, 40)) + [63, 64, 65, 87, 88, 100, 101, 102, 128, 129, 193, 257]


def test_byte_counts_are_pure_monotone_and_restated():
    lib = _hip()
    for h in SIZES:
        for w in SIZES:
            assert lib.jslps_lds_bytes(h, w, 0) == lib.jslpp_lds_bytes(h, w)
            assert lib.jslps_tree_lds_bytes(h, w, h + 3, 0) == lib.jslpt_lds_bytes(h, w, h + 3)
            for no in (0, 1, 2, 3, 7):
                assert pack_lds_bytes(h, w, no) == lib.jslps_lds_bytes(h, w, no)
                assert tree_lds_bytes(h, w, h + 5, no) == lib.jslps_tree_lds_bytes(h, w, h + 5, no)
    assert lib.jslps_lds_bytes(5, 5, -1) == 0 and lib.jslps_tree_lds_bytes(5, 5, 6, -1) == 0 and pack_lds_bytes(5, 5, -1) == 0
    assert lib.jslps_lds_bytes(1, 5, 1) == 0 and lib.jslps_lds_bytes(5, 1, 1) == 0 and lib.jslps_tree_lds_bytes(5, 5, 4, 1) == 0
    cube = np.array([[[lib.jslps_lds_bytes(h, w, no) for no in range(6)] for w in SIZES] for h in SIZES], dtype=np.int64)
    assert (cube > 0).all() and (cube % 16 == 0).all()
    assert (np.diff(cube, axis=0) > 0).all()   # a row more always costs
    assert (np.diff(cube, axis=1) >= 0).all()  # a column more never saves
    assert (np.diff(cube, axis=2) >= 0).all() and (cube[:, :, 2:] > cube[:, :, :-2]).all()  # an optional row is a row of the odd stride
    # an optional row costs what its cells cost: 8 bytes per cell of the padded stride, within the 16-byte rounding
    for h, w in ((7, 6), (9, 8), (12, 14), (40, 65), (24, 102)):
        for no in (1, 2, 3):
            extra = lib.jslps_lds_bytes(h, w, no) - lib.jslps_lds_bytes(h, w, 0)
            assert abs(extra - 8 * no * (w | 1)) <= 8
    tree = np.array([[lib.jslps_tree_lds_bytes(20, 30, rc, no) for no in range(5)] for rc in range(20, 40)], dtype=np.int64)
    assert (np.diff(tree, axis=0) > 0).all() and (np.diff(tree, axis=1) >= 0).all() and (tree[:, 2:] > tree[:, :-2]).all()


def test_routing_helpers_take_a_row_count():
    lib = _hip()
    assert pack_fits(87, 87) and pack_fits(87, 87, lib=lib) and not pack_fits(87, 87, n_optional=3) and not pack_fits(87, 87, lib=lib, n_optional=3)
    assert pack_fits(12, 14, n_optional=3) and pack_fits(12, 14, lib=lib, n_optional=3)
    # cut rows and optional rows share the 64 KiB: the more of one, the fewer of the other
    rows = [tree_cut_rows(60, 65, 200, n_optional=no) for no in (0, 1, 2, 3, 10, 50)]
    assert rows == [tree_cut_rows(60, 65, 200, lib=lib, n_optional=no) for no in (0, 1, 2, 3, 10, 50)]
    assert all(a > b for a, b in zip(rows, rows[1:])) and rows[0] == tree_cut_rows(60, 65, 200) and rows[-1] >= 1
    assert tree_cut_rows(9, 8, 3, n_optional=2) == 6  # 2 per integer variable when everything fits


def _create(lib, heights, widths, n_optional, tree=False):
    n = len(heights)
    h = ctypes.c_void_p()
    hs, ws, ps = _capi.ptr_i32(_capi.as_i32(heights)), _capi.ptr_i32(_capi.as_i32(widths)), _capi.ptr_f64(_capi.as_f64([1e-8] * n))
    no = None if n_optional is None else _capi.ptr_i32(_capi.as_i32(n_optional))
    if tree:
        ones = _capi.as_i32([1] * n)
        rc = lib.jslps_tree_pack_create(ctypes.byref(h), 0, n, hs, ws, ps, _capi.ptr_i32(ones), _capi.ptr_i32(ones), no, 0, 0, 0)
    else:
        rc = lib.jslps_pack_create(ctypes.byref(h), 0, n, hs, ws, ps, no, 0, 0)
    return rc, h


def test_refusals_without_a_device():
    """refused before any device call: this host has no GPU, and a call that reached the device would answer JSLP_ERR_DEVICE"""
    lib = _hip()
    # a shape the pack takes as it is and not with three optional rows
    h, w = 87, 87
    assert 0 < lib.jslpp_lds_bytes(h, w) <= LIMIT < lib.jslps_lds_bytes(h, w, 3)
    rc, p = _create(lib, [7, h, h], [6, w, w], [1, 0, 3])
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and not p.value
    assert b"LP 2" in lib.jslp_last_error() and b"64 KiB" in lib.jslp_last_error()
    rc, p = _create(lib, [7, 40], [6, 65], [1, 2 ** 30])  # (a byte count that would not fit 32 bits)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and b"LP 1" in lib.jslp_last_error()
    # the same with cut rows: one cut row fits without the optional rows
    assert 0 < lib.jslpt_lds_bytes(86, 87, 87) <= LIMIT < lib.jslps_tree_lds_bytes(86, 87, 87, 3)
    rc, p = _create(lib, [9, 86], [8, 87], [2, 3], tree=True)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and not p.value and b"LP 1" in lib.jslp_last_error()
    # a negative count names its LP
    rc, p = _create(lib, [7, 7], [6, 6], [1, -1])
    assert rc == _capi.JSLP_ERR_ARG and b"LP 1" in lib.jslp_last_error()
    rc, p = _create(lib, [7, 7], [6, 6], [1, -1], tree=True)
    assert rc == _capi.JSLP_ERR_ARG and b"LP 1" in lib.jslp_last_error()
    # the argument errors of the plain creates come first, as before
    assert lib.jslps_pack_create(None, 0, 1, None, None, None, None, 0, 0) == _capi.JSLP_ERR_ARG
    assert _create(lib, [7, 1], [6, 6], None)[0] == _capi.JSLP_ERR_ARG and b"LP 1" in lib.jslp_last_error()
    # the other entry points refuse a null pack
    assert lib.jslps_pack_set_optional_objectives(None, 0, None) == _capi.JSLP_ERR_ARG
    assert lib.jslps_pack_get_optional_objectives(None, 0, None, None) == _capi.JSLP_ERR_ARG
