"""The MIR tree extension's boundary (runs without a GPU): include/jslpc_tree_mir.h, the ctypes table TREE_MIR_SYMBOLS and the jslpc_
exports of the product and test libraries agree; the extension stays out of the other headers and out of the oracle; create refuses bad
arguments and row capacities beyond the LDS limit before touching a device; jslpc_tree_lds_bytes is a pure, monotone function that equals
its restatement."""
import ctypes
import os

import numpy as np

from jslpsolver_amd import _capi
from jslpsolver_amd.engine import tree_lds_bytes, tree_mir_lds_bytes, tree_mir_rows
from test_many_abi import built, declared_in_header, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslpc_tree_mir.h")
CHAOS = os.path.join(ROOT, "jslpsolver_amd", "csrc", "libjslp_hip_chaos.so")
PREFIX = "jslpc_"


def _hip():
    return _capi.Library(built(_capi.HIP_LIB_PATH))


def test_header_and_binding_declare_the_same_extension():
    declared = declared_in_header(HEADER, PREFIX)
    assert declared == set(_capi.TREE_MIR_SYMBOLS) and len(declared) == 3
    for other in ("jslp_engine.h", "jslpp_packed.h", "jslpt_tree.h", "jslps_soft.h", "jslpm_many.h", "jslpx_branch.h", "jslpr_mir.h", "jslpf_f32.h"):
        assert not declared_in_header(os.path.join(ROOT, "include", other), PREFIX)
    for other in (_capi.SYMBOLS, _capi.MANY_SYMBOLS, _capi.BRANCH_SYMBOLS, _capi.F32_SYMBOLS, _capi.MIR_SYMBOLS, _capi.PACK_SYMBOLS, _capi.TREE_SYMBOLS,
                  _capi.SOFT_SYMBOLS):
        assert not set(_capi.TREE_MIR_SYMBOLS) & set(other)
    assert ctypes.sizeof(ctypes.c_int32) * 5 == _capi.MIR_TREE_DTYPE.itemsize == 20
    assert _capi.MIR_TREE_DTYPE.names == ("rounds", "rows_added", "simplexes", "root_rows", "rows_high_water")
    text = open(HEADER).read()
    order = [text.index("int32_t %s;" % name) for name in _capi.MIR_TREE_DTYPE.names]  # the struct's members, in the dtype's order
    assert order == sorted(order)


def test_product_and_test_libraries_export_the_extension():
    assert exported(built(_capi.HIP_LIB_PATH), PREFIX) == declared_in_header(HEADER, PREFIX)
    assert exported(built(CHAOS), PREFIX) == declared_in_header(HEADER, PREFIX)
    assert _hip().has_tree_mir


def test_oracle_does_not_export_the_extension(oracle_lib):
    assert exported(oracle_lib.path, PREFIX) == set()
    assert not oracle_lib.has_tree_mir


def _create(lib, n, heights, widths, cut_rows, heap_cap, row_extra, trace_cap=0, max_pivots=0, max_nodes=0):
    h = ctypes.c_void_p()
    arr = lambda a: None if a is None else _capi.ptr_i32(_capi.as_i32(a))  # noqa: E731
    ps = _capi.ptr_f64(_capi.as_f64([1e-8] * max(n, 1)))
    rc = lib.jslpc_tree_pack_create(ctypes.byref(h), 0, n, arr(heights), arr(widths), ps, arr(cut_rows), arr(heap_cap), arr(row_extra), trace_cap,
                                    max_pivots, max_nodes)
    return rc, h


def test_argument_errors_without_a_device():
    """refused before any device call: this host has no GPU, and a call that reached the device would answer JSLP_ERR_DEVICE"""
    lib = _hip()
    assert _create(lib, 1, [3], [3], [2], [4], None)[0] == _capi.JSLP_ERR_ARG
    assert _create(lib, 1, [3], [3], None, [4], [2])[0] == _capi.JSLP_ERR_ARG
    assert _create(lib, 1, [3], [3], [2], None, [2])[0] == _capi.JSLP_ERR_ARG
    # 0 <= row_extra < cut_rows names the LP (a negative one makes a plain tree LP)
    assert _create(lib, 2, [3, 3], [3, 3], [2, 2], [4, 4], [2, 1])[0] == _capi.JSLP_ERR_ARG
    assert b"LP 1" in lib.jslp_last_error() and b"row_extra" in lib.jslp_last_error()
    assert _create(lib, 2, [3, 3], [3, 3], [2, 2], [4, 4], [0, 5])[0] == _capi.JSLP_ERR_ARG
    assert b"LP 0" in lib.jslp_last_error()
    assert _create(lib, 1, [3], [3], [2], [0], [2])[0] == _capi.JSLP_ERR_ARG
    # Knapsack_1 (52 x 51, 50 integer variables): the most rows that fit as a MIR LP, one fewer than as a plain tree LP's 96
    extra, cuts = tree_mir_rows(52, 51, 50, lib=lib)
    assert (extra, cuts) == tree_mir_rows(52, 51, 50) == (95, 95)
    assert lib.jslpc_tree_lds_bytes(52, 51, 52 + extra) <= 65536 < lib.jslpc_tree_lds_bytes(52, 51, 52 + extra + 1)
    rc, h = _create(lib, 2, [3, 52], [3, 51], [4, 20], [8, 8], [4, extra + 1])
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and not h.value
    assert b"LP 1" in lib.jslp_last_error() and b"64 KiB" in lib.jslp_last_error()
    # ... and a plain LP of such a pack is held against the plain byte count
    rc, h = _create(lib, 2, [3, 52], [3, 51], [4, 97], [8, 8], [4, -1])
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and b"LP 1" in lib.jslp_last_error()
    rc, h = _create(lib, 1, [2 ** 20], [2 ** 20], [1], [1], [2 ** 20])  # (a byte count that would not fit 32 bits)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and b"LP 0" in lib.jslp_last_error()
    assert lib.jslpc_pack_read_mir(None, None) == _capi.JSLP_ERR_ARG


def test_lds_bytes_against_its_restatement():
    lib = _hip()
    sizes = [2, 3, 4, 5, 7, 8, 16, 31, 32, 33, 51, 52, 63, 64, 65, 66, 87, 88, 100, 128, 129, 257]
    extra = [0, 1, 2, 3, 4, 7, 8, 20, 63, 64, 65, 100, 320]
    table = np.array([[[lib.jslpc_tree_lds_bytes(h, w, h + e) for e in extra] for w in sizes] for h in sizes], dtype=np.int64)
    assert (table > 0).all() and (table % 16 == 0).all()
    assert (np.diff(table, axis=0) > 0).all()   # a row more always costs
    assert (np.diff(table, axis=1) >= 0).all()  # a column more never saves
    assert (np.diff(table, axis=2) > 0).all()   # a row of capacity more always costs
    for i, h in enumerate(sizes):
        for j, w in enumerate(sizes):
            for k, e in enumerate(extra):
                assert table[i, j, k] == tree_mir_lds_bytes(h, w, h + e)
                grown = table[i, j, k] - lib.jslpt_lds_bytes(h, w, h + e)  # the flags: one byte per variable index, padded to 16
                n_idx = w + 2 * (h + e) + 2
                assert grown == (n_idx + 15) // 16 * 16 and tree_lds_bytes(h, w, h + e) == lib.jslpt_lds_bytes(h, w, h + e)
    assert lib.jslpc_tree_lds_bytes(1, 5, 5) == 0 and lib.jslpc_tree_lds_bytes(5, 1, 5) == 0 and lib.jslpc_tree_lds_bytes(5, 5, 4) == 0
    assert tree_mir_lds_bytes(1, 5, 5) == 0 and tree_mir_lds_bytes(5, 1, 5) == 0 and tree_mir_lds_bytes(5, 5, 4) == 0
    # the routing rule: 2 per integer variable + 320, or the most that fit, or nothing; the cut rows never beyond the rows
    assert tree_mir_rows(3, 3, 2, lib=lib) == (324, 4) and tree_mir_rows(88, 88, 3, lib=lib) == (0, 0)
    for h, w, n_int in ((52, 51, 50), (60, 65, 40), (80, 80, 10), (30, 20, 6)):
        r, c = tree_mir_rows(h, w, n_int, lib=lib)
        assert (r, c) == tree_mir_rows(h, w, n_int) and 0 < r <= 2 * n_int + 320 and c == min(2 * n_int, r)
        assert lib.jslpc_tree_lds_bytes(h, w, h + r) <= 65536
        assert r == 2 * n_int + 320 or lib.jslpc_tree_lds_bytes(h, w, h + r + 1) > 65536
