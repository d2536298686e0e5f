"""include/jslpb_big_lds.h without a GPU: the header, its ctypes table and the exports agree; the byte counts the 156 KiB limit rests on; the
creates refuse bad arguments and images beyond the limit of their kind before any device call; solve_packed(big_lds=True) adds the models the
64 KiB rules leave out and moves no other; TableauPack(big_lds=True) on the CPU oracle lifts the limit of the restatement."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import tree_pack_util as U
from jslpsolver_amd import Solve, _capi, generators, solver
from jslpsolver_amd.engine import TableauPack, pack_fits, pack_lds_bytes, tree_cut_rows, tree_lds_bytes
from test_many_abi import built, declared_in_header, exported
from test_packed_gpu import _engine_state, _pack_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslpb_big_lds.h")
CHAOS = os.path.join(ROOT, "jslpsolver_amd", "csrc", "libjslp_hip_chaos.so")
PREFIX = "jslpb_"
LIMIT = 159744


@pytest.fixture(scope="module")
def lib():
    return _capi.Library(built(_capi.HIP_LIB_PATH))


def test_header_binding_and_libraries_agree(oracle_lib, lib):
    declared = declared_in_header(HEADER, PREFIX)
    assert declared == set(_capi.BIG_SYMBOLS) == {"jslpb_pack_create", "jslpb_tree_pack_create", "jslpb_pack_big_threads"}
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "jslpb_big_lds.h":
            assert not declared_in_header(os.path.join(ROOT, "include", other), PREFIX), other
    assert exported(built(_capi.HIP_LIB_PATH), PREFIX) == declared and exported(built(CHAOS), PREFIX) == declared
    assert exported(oracle_lib.path, PREFIX) == set() and not oracle_lib.has_big_lds
    assert lib.has_big_lds and lib.jslpb_pack_big_threads() in (256, 512, 1024)
    assert "#define JSLPB_LDS_LIMIT %d" % LIMIT in open(HEADER).read() and _capi.JSLPB_LDS_LIMIT == LIMIT == 160 * 1024 - 4096


def test_the_byte_counts_the_limit_rests_on(lib):
    for count in (pack_lds_bytes, lambda h, w: int(lib.jslpp_lds_bytes(h, w))):
        assert count(87, 87) == 64336 <= 65536 < 66480 == count(88, 88)
        assert count(138, 138) == 159424 <= LIMIT < 160592 == count(139, 139)
        assert count(193, 65) == 107072
        assert count(288, 65) == 159296 <= LIMIT < 159872 == count(289, 65)
    assert tree_lds_bytes(52, 51, 252) == int(lib.jslpt_lds_bytes(52, 51, 252)) == 111088
    # Sudoku4x4 (193 x 65, 64 integer variables) gets exactly 95 cut rows under the larger limit and none under the 64 KiB one
    assert tree_cut_rows(193, 65, 64, limit=LIMIT) == tree_cut_rows(193, 65, 64, lib=lib, limit=LIMIT) == 95
    assert tree_cut_rows(193, 65, 64) == tree_cut_rows(193, 65, 64, lib=lib) == 0
    assert pack_fits(138, 138, limit=LIMIT) and pack_fits(138, 138, lib=lib, limit=LIMIT) and not pack_fits(139, 139, limit=LIMIT)
    assert pack_fits(87, 87) and not pack_fits(88, 88) and not pack_fits(88, 88, lib=lib)


def _arr(a):
    return None if a is None else _capi.ptr_i32(_capi.as_i32(a))


def _create(lib, heights, widths, big_lds, n_optional=None):
    h, n = ctypes.c_void_p(), len(heights)
    rc = lib.jslpb_pack_create(ctypes.byref(h), 0, n, _arr(heights), _arr(widths), _capi.ptr_f64(_capi.as_f64([1e-8] * n)), _arr(n_optional), 0, 0, big_lds)
    assert not h.value
    return rc, lib.jslp_last_error().decode()


def _tree_create(lib, big_lds, **kw):
    """two LPs: a 3 x 4 one and Knapsack_1's shape, 52 x 51, at row capacity 252 (an image of 111 088 bytes)"""
    d = dict(heights=[3, 52], widths=[4, 51], cut_rows=[2, 200], heap_cap=[4, 4], n_optional=None, row_extra=[-1, -1], node_selection=[0, 0],
             branching=[0, 0], incremental=[0, 0], max_checkpoints=[0, 0], tolerance=None, minimize=None)
    d.update(kw)
    h = ctypes.c_void_p()
    rc = lib.jslpb_tree_pack_create(ctypes.byref(h), 0, 2, _arr(d["heights"]), _arr(d["widths"]), _capi.ptr_f64(_capi.as_f64([1e-8, 1e-8])), _arr(d["cut_rows"]),
                                    _arr(d["heap_cap"]), _arr(d["n_optional"]), _arr(d["row_extra"]), _arr(d["node_selection"]), _arr(d["branching"]),
                                    _arr(d["incremental"]), _arr(d["max_checkpoints"]),
                                    None if d["tolerance"] is None else _capi.ptr_f64(_capi.as_f64(d["tolerance"])), _arr(d["minimize"]), 0, 0, 0, big_lds)
    assert not h.value
    return rc, lib.jslp_last_error().decode()


def test_refusals_before_any_device_call(lib):
    """this host has no GPU: a call that reached the device would answer JSLP_ERR_DEVICE"""
    for big_lds in (2, -1, 256):
        rc, msg = _create(lib, [138], [138], big_lds)
        assert rc == _capi.JSLP_ERR_ARG and "big_lds" in msg
        rc, msg = _tree_create(lib, big_lds)
        assert rc == _capi.JSLP_ERR_ARG and "big_lds" in msg
    rc, msg = _create(lib, [139], [139], 1)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and "LP 0" in msg and "JSLPB_LDS_LIMIT" in msg
    rc, msg = _create(lib, [3, 139], [4, 139], 1)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and "LP 1" in msg
    rc, msg = _create(lib, [137], [138], 1, n_optional=[2])  # (two optional rows carry the image over the limit: jslps_lds_bytes)
    assert pack_lds_bytes(137, 138, 2) > LIMIT >= pack_lds_bytes(137, 138, 1) and rc == _capi.JSLP_ERR_UNSUPPORTED and "LP 0" in msg
    rc, msg = _create(lib, [3, 1 << 30], [4, 1 << 30], 1)  # (the pre-filter: an absurd shape is refused before its byte count is taken)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and "LP 1" in msg
    # big_lds = 0 is the older twin, word for word: 88 x 88 is beyond ITS limit
    rc, msg = _create(lib, [88], [88], 0)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and msg == "pack_create: LP 0: the tableau's LDS image exceeds 64 KiB (jslpp_lds_bytes): solve it through a jslp_engine"
    rc, msg = _tree_create(lib, 0)
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and "LP 1" in msg and "exceeds 64 KiB (jslpt_lds_bytes)" in msg
    # the kinds without a large build keep the 64 KiB rule, each refusal naming the LP and its kind
    for kind, kw in (("MIR LP", dict(row_extra=[-1, 200])), ("enhanced LP", dict(node_selection=[0, 2])), ("enhanced LP", dict(branching=[0, 1])),
                     ("incremental LP", dict(incremental=[0, 1], max_checkpoints=[0, 8], row_extra=[-1, 200])),
                     ("LP with a tolerance", dict(tolerance=[0.0, 0.05])), ("LP with a tolerance", dict(tolerance=[0.0, 0.05], minimize=[1, 0]))):
        rc, msg = _tree_create(lib, 1, **kw)
        assert rc == _capi.JSLP_ERR_UNSUPPORTED and "LP 1" in msg and kind in msg and "64 KiB" in msg, (kind, msg)
    rc, msg = _tree_create(lib, 1, cut_rows=[2, 1000])
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and "LP 1" in msg and "JSLPB_LDS_LIMIT" in msg
    # and what passes every argument check reaches the device question (none here)
    for rc, msg in (_create(lib, [138, 88, 3], [138, 88, 4], 1), _tree_create(lib, 1), _tree_create(lib, 1, tolerance=[0.05, 0.0])):
        assert rc == _capi.JSLP_ERR_DEVICE and "no HIP device" in msg


def _dense(h, w, seed=4242):
    m, vibr, vibc = generators.dense_resource_allocation_tableau(seed + 131 * h + w, w - 1, h - 1)
    assert m.shape == (h, w)
    return (m, vibr, vibc, []), 1e-8, True


def test_restatement_on_the_oracle(oracle_lib):
    items = [_dense(88, 88), _dense(138, 138), _dense(5, 7)]
    pack = TableauPack([lp for lp, _, _ in items], lib=oracle_lib, trace_cap=4096, big_lds=True)
    assert pack.big_lds and pack.lds_limit == LIMIT and pack.is_big.tolist() == [True, True, False] and pack.lds_bytes.tolist()[:2] == [66480, 159424]
    pack.simplex(check_cycles=True)
    for i, (lp, p, c) in enumerate(items):
        assert _pack_state(pack, i) == _engine_state(oracle_lib, lp, p, c), i
    pack.close()
    with pytest.raises(_capi.EngineError, match=r"jslpp_pack_create failed \(-6\).*LP 0.*64 KiB"):
        TableauPack([items[0][0]], lib=oracle_lib)
    with pytest.raises(_capi.EngineError, match=r"jslpb_pack_create failed \(-6\).*LP 1.*JSLPB_LDS_LIMIT"):
        TableauPack([items[0][0], _dense(139, 139)[0]], lib=oracle_lib, big_lds=True)
    knap = U.Item(U.fixture("Knapsack_1")["model"], cut_rows=200)
    for kind, kw in (("enhanced LP", dict(node_selection=["depth-first"])), ("LP with a tolerance", dict(tolerance=[0.05]))):
        with pytest.raises(_capi.EngineError, match=r"jslpb_tree_pack_create failed \(-6\).*LP 0.*%s.*64 KiB" % kind):
            TableauPack([knap.lp], lib=oracle_lib, integers=[knap.integers], cut_rows=[200], big_lds=True, **kw)
    with pytest.raises(_capi.EngineError, match=r"\(-6\).*LP 0.*MIR LP.*64 KiB"):
        TableauPack([knap.lp], lib=oracle_lib, integers=[knap.integers], cut_rows=[200], mir=[True], row_extra=[200], big_lds=True)
    with pytest.raises(_capi.EngineError, match=r"\(-6\).*LP 0.*incremental LP.*64 KiB"):
        TableauPack([knap.lp], lib=oracle_lib, integers=[knap.integers], cut_rows=[200], incremental=[True], row_extra=[200], big_lds=True)


def _routed(monkeypatch):
    """every TableauPack solve_packed makes from here on: (tree pack?, big_lds, per LP (height, width, cut rows or None, thread class))"""
    seen = []
    plain = solver.TableauPack

    class Spy(plain):
        def __init__(self, lps, **kw):
            plain.__init__(self, lps, **kw)
            cuts = self.cut_rows.tolist() if self.is_tree else [None] * self.n
            cls = ["large" if b else 64 if int(rc) * int(w) <= 2048 else 256 for b, rc, w in zip(self.is_big, self.row_capacity, self.widths)]
            seen.append((self.is_tree, self.big_lds, list(zip(self.heights.tolist(), self.widths.tolist(), cuts, cls))))

    monkeypatch.setattr(solver, "TableauPack", Spy)
    return seen


def test_routing_with_and_without_the_keyword(oracle_lib, monkeypatch):
    names = U.TREE_FIXTURES + ["Sudoku4x4", "Fertilizer", "Relaxed", "Berlin_Air_Lift_Problem", "Wiki_1", "LargeFarmMIP", "Vendor_Selection"]
    models = [U.fixture(n)["model"] for n in names]
    big_lp = generators.resource_allocation_model(7, 110, 100, density=0.9)  # an LP whose tableau is beyond 64 KiB and within 156 KiB
    m, _, _ = solver._parse(big_lp, None, 2)[1:]
    assert 65536 < pack_lds_bytes(*m.shape) <= LIMIT
    models.append(big_lp)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(mm, lib=oracle_lib)) for mm in models]
        seen = _routed(monkeypatch)
        assert [repr(r) for r in solver.solve_packed(models, lib=oracle_lib)] == want
        before = list(seen)
        del seen[:]
        assert [repr(r) for r in solver.solve_packed(models, lib=oracle_lib, big_lds=True)] == want
    assert all(not big for _, big, _ in before) and all("large" not in [c for _, _, _, c in lps] for _, _, lps in before)
    assert len(before) == len(seen) == 2
    for (tree0, _, lps0), (tree1, big1, lps1) in zip(before, seen):
        # every model that was packed keeps its pack, its place, its cut rows and its thread class; the keyword only adds large LPs
        assert tree0 == tree1 and big1 and [x for x in lps1 if x[3] != "large"] == lps0 and len(lps1) == len(lps0) + 1
    assert (193, 65, 95, "large") in seen[1][2] and [x for x in seen[0][2] if x[3] == "large"] == [m.shape + (None, "large")]
    sudoku = U.fixture("Sudoku4x4")
    got = solver.solve_packed([sudoku["model"]], lib=oracle_lib, big_lds=True)[0]
    assert list(got.keys()) == sudoku["resultKeys"] and got == Solve(sudoku["model"], lib=oracle_lib)
    with pytest.raises(TypeError):
        solver.solve_packed(models, lib=oracle_lib, big=True)


def test_a_model_with_a_tolerance_keeps_the_64_kib_rule(oracle_lib, monkeypatch):
    sudoku = dict(U.fixture("Sudoku4x4")["model"], options={"tolerance": 0.05})
    seen = _routed(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = solver.solve_packed([sudoku], lib=oracle_lib, big_lds=True, tolerance=True)
        assert repr(got[0]) == repr(Solve(sudoku, lib=oracle_lib)) and seen == []
