"""include/jslpi_tree_incremental.h at the boundary (runs without a GPU): the header, its ctypes table and the exports agree; the create
refuses bad arguments before any device call, naming the LP; the byte counts agree with their Python restatements."""
import ctypes
import os

import pytest

from jslpsolver_amd import _capi
from jslpsolver_amd.engine import checkpoint_bytes, incremental_rows, tree_lds_bytes
from test_many_abi import built, declared_in_header, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslpi_tree_incremental.h")
CHAOS = os.path.join(ROOT, "jslpsolver_amd", "csrc", "libjslp_hip_chaos.so")
PREFIX = "jslpi_"


@pytest.fixture(scope="module")
def lib():
    return _capi.Library(built(_capi.HIP_LIB_PATH))


def test_header_binding_and_libraries_agree(oracle_lib, lib):
    declared = declared_in_header(HEADER, PREFIX)
    assert declared == set(_capi.TREE_INC_SYMBOLS) == {"jslpi_tree_pack_create", "jslpi_tree_lds_bytes", "jslpi_checkpoint_bytes",
                                                       "jslpi_pack_read_incremental"}
    for other in ("jslp_engine.h", "jslpp_packed.h", "jslpt_tree.h", "jslps_soft.h", "jslpc_tree_mir.h", "jslpe_tree_enhanced.h", "jslpm_many.h",
                  "jslpx_branch.h", "jslpr_mir.h", "jslpf_f32.h"):
        assert not declared_in_header(os.path.join(ROOT, "include", other), PREFIX)
    assert _capi.INC_TREE_DTYPE.itemsize == 32
    text = open(HEADER).read()
    order = [text.index("int32_t %s;" % name) for name in _capi.INC_TREE_DTYPE.names[:4]]  # the struct's members, in the dtype's order
    assert order == sorted(order)
    assert "#define JSLPI_MAX_CHECKPOINTS %d " % _capi.JSLPI_MAX_CHECKPOINTS in text
    assert "#define JSLPI_CHECKPOINTS_DEFAULT %d " % _capi.JSLPI_CHECKPOINTS_DEFAULT in text and _capi.JSLPI_CHECKPOINTS_DEFAULT == 50
    assert exported(built(_capi.HIP_LIB_PATH), PREFIX) == declared and exported(built(CHAOS), PREFIX) == declared
    assert lib.has_tree_inc
    assert exported(oracle_lib.path, PREFIX) == set() and not oracle_lib.has_tree_inc


def _create(lib, n, heights, widths, cut_rows, heap_cap, row_extra, incremental, max_checkpoints, node_selection=None, branching=None,
            n_optional=None):
    h = ctypes.c_void_p()
    arr = lambda a: None if a is None else _capi.ptr_i32(_capi.as_i32(a))  # noqa: E731
    zeros = [0] * n
    rc = lib.jslpi_tree_pack_create(ctypes.byref(h), 0, n, arr(heights), arr(widths), _capi.ptr_f64(_capi.as_f64([1e-8] * max(n, 1))), arr(cut_rows),
                                    arr(heap_cap), arr(n_optional), arr(row_extra), arr(zeros if node_selection is None else node_selection),
                                    arr(zeros if branching is None else branching), arr(incremental), arr(max_checkpoints), 0, 0, 0)
    return rc, h, lib.jslp_last_error()


def test_create_argument_errors_without_a_device(lib):
    """refused before any device call: this host has no GPU, and a call that reached the device would answer JSLP_ERR_DEVICE"""
    two = dict(n=2, heights=[3, 3], widths=[4, 4], cut_rows=[2, 2], heap_cap=[4, 4])
    # null tables
    assert _create(lib, row_extra=[-1, 5], incremental=None, max_checkpoints=[0, 50], **two)[0] == _capi.JSLP_ERR_ARG
    assert _create(lib, row_extra=[-1, 5], incremental=[0, 1], max_checkpoints=None, **two)[0] == _capi.JSLP_ERR_ARG
    for kw, word in ((dict(row_extra=[-1, 5], incremental=[0, 2], max_checkpoints=[0, 50]), b"incremental is 0 or 1"),
                     (dict(row_extra=[-1, 5], incremental=[0, -1], max_checkpoints=[0, 50]), b"incremental is 0 or 1"),
                     (dict(row_extra=[-1, 5], incremental=[0, 1], max_checkpoints=[0, 65]), b"max_checkpoints"),
                     (dict(row_extra=[-1, 5], incremental=[0, 1], max_checkpoints=[0, -1]), b"max_checkpoints"),
                     (dict(row_extra=[-1, 1], incremental=[0, 1], max_checkpoints=[0, 50]), b"row_extra"),   # below cut_rows
                     (dict(row_extra=[-1, -1], incremental=[0, 1], max_checkpoints=[0, 50]), b"row_extra"),
                     (dict(row_extra=None, incremental=[0, 1], max_checkpoints=[0, 50]), b"row_extra"),
                     (dict(row_extra=[-1, 5], incremental=[0, 1], max_checkpoints=[0, 50], n_optional=[1, 1]), b"optional"),
                     (dict(row_extra=[-1, 5], incremental=[0, 1], max_checkpoints=[0, 50], node_selection=[0, 4]), b"node_selection"),
                     (dict(row_extra=[-1, 5], incremental=[0, 1], max_checkpoints=[0, 50], branching=[0, -1]), b"branching")):
        rc, h, msg = _create(lib, **dict(two, **kw))
        assert rc == _capi.JSLP_ERR_ARG and not h.value and b"LP 1" in msg and word in msg, (kw, msg)
    # max_checkpoints is read for an incremental LP only; a MIR LP beside an incremental one keeps its own rules
    rc, h, msg = _create(lib, row_extra=[1, 5], incremental=[0, 1], max_checkpoints=[99, 50], **two)
    assert rc == _capi.JSLP_ERR_ARG and b"LP 0" in msg and b"MIR" in msg  # (LP 0 is a MIR LP whose row_extra is below its cut_rows)
    rc, h, msg = _create(lib, row_extra=[5, 5], incremental=[0, 1], max_checkpoints=[0, 50], n_optional=[1, 0], **two)
    assert rc == _capi.JSLP_ERR_ARG and b"LP 0" in msg and b"optional" in msg
    assert lib.jslpi_pack_read_incremental(None, None) == _capi.JSLP_ERR_ARG


def test_the_64_kib_refusal_names_the_lp(lib):
    # Knapsack_1 (52 x 51) holds 96 rows beyond its own, as a tree LP and as an incremental one
    assert lib.jslpi_tree_lds_bytes(52, 51, 52 + 96) <= 65536 < lib.jslpi_tree_lds_bytes(52, 51, 52 + 97)
    assert incremental_rows(52, 51, 50, lib=lib) == incremental_rows(52, 51, 50) == (96, 96)
    assert incremental_rows(3, 4, 2, lib=lib) == incremental_rows(3, 4, 2) == (260, 4)
    rc, h, msg = _create(lib, 2, [3, 52], [4, 51], [4, 96], [8, 8], [10, 97], [1, 1], [50, 50])
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and not h.value and b"LP 1" in msg and b"64 KiB" in msg and b"row_extra" in msg
    # exactly at the limit the create goes on to the device (none here, or a pack there)
    rc, h, msg = _create(lib, 2, [3, 52], [4, 51], [4, 96], [8, 8], [10, 96], [1, 1], [50, 50])
    assert rc in (_capi.JSLP_OK, _capi.JSLP_ERR_DEVICE), msg
    if rc == _capi.JSLP_OK:
        lib.jslpp_pack_destroy(h)
    # an absurd shape must not overflow before it is compared
    rc, h, msg = _create(lib, 1, [2 ** 30], [2 ** 30], [0], [8], [2 ** 30], [1], [50])
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and b"LP 0" in msg


def test_byte_counts_agree_with_their_restatements(lib):
    for h, w in ((2, 2), (2, 5), (3, 4), (4, 3), (7, 5), (52, 51), (10, 101), (33, 2)):
        for extra in (0, 1, 2, 3, 7, 96, 260):
            rc = h + extra
            assert lib.jslpi_tree_lds_bytes(h, w, rc) == lib.jslpt_lds_bytes(h, w, rc) == tree_lds_bytes(h, w, rc) > 0
            b = lib.jslpi_checkpoint_bytes(h, w, rc)
            assert b == checkpoint_bytes(h, w, rc) and b % 16 == 0
            # a 16-byte header, the rows in 16-byte words (half a word of padding when rc * w is odd), the integer block of the LDS image
            doubles = (rc * (w | 1) + rc + 1) & ~1
            assert b == 16 + 8 * (rc * w + (rc * w & 1)) + (tree_lds_bytes(h, w, rc) - 8 * doubles)
    for bad in ((1, 4, 4), (3, 1, 4), (3, 4, 2)):
        assert lib.jslpi_tree_lds_bytes(*bad) == 0 and lib.jslpi_checkpoint_bytes(*bad) == 0 and checkpoint_bytes(*bad) == 0
    # solve_packed's budget: 50 checkpoints of an LP at the LDS limit stay near 50 x 64 KiB
    assert 50 * lib.jslpi_checkpoint_bytes(52, 51, 148) <= 50 * 65536
