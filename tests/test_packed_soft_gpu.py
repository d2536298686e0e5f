"""Optional objectives in the pack kernels on the MI355X (include/jslps_soft.h): k_simplex_packed<.., OPT> and k_tree_packed<.., OPT>.

The yardsticks are the reference's recorded runs (fuzz_soft records, the fixtures' goldens), the CPU oracle through jslp_engine_* (behind
TableauPack's restatement) and, for trees, the Python host tree on the oracle; the pack on the GPU is never compared with itself.  The inputs
are tests/soft_pack_util.py's, whose coverage of the new code tests/test_packed_soft_cpu.py asserts.  The JSLP_DEBUG_LAUNCH lines say which
builds ran and with how many LPs."""
import ctypes
import re
import warnings

import numpy as np
import pytest

import golden_util as G
import soft_pack_util as S
import tree_pack_util as U
from jslpsolver_amd import Solve, _capi, solver

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[jslp\] launch (k_simplex_packed|k_tree_packed)<(\d+)(,opt 1)?> n (\d+) lds (\d+)")
LDS_LIMIT = 65536


def _launches(capfd):
    return [(k, int(t), bool(o), int(n), int(b)) for k, t, o, n, b in LAUNCH.findall(capfd.readouterr().err)]


def _check_lines(lines, kernel, items, pack):
    """at most four launches, one per build; their n sum to the pack; the LPs without optional rows are in the opt-less lines"""
    assert 1 <= len(lines) <= 4 and pack.launches == len(lines) and len({(t, o) for _, t, o, _, _ in lines}) == len(lines), lines
    assert all(k == kernel and b <= LDS_LIMIT for k, _, _, _, b in lines), lines
    assert sum(n for _, _, o, n, _ in lines if o) == sum(it.n_optional > 0 for it in items), lines
    assert sum(n for _, _, o, n, _ in lines if not o) == sum(it.n_optional == 0 for it in items), lines


def test_recorded_lps_and_fixtures_in_one_mixed_pack(hip_lib, oracle_lib, monkeypatch, capfd):
    """sets A and C next to LPs without optional objectives: the recorded runs, the goldens, and the oracle engine byte for byte"""
    records, _ = S.soft_records()
    plain, _ = S.plain_records()
    la, _ = S.items_a()
    fixtures = [S.SoftItem(U.fixture(n)["model"]) for n in S.SOFT_FIXTURES + S.PLAIN_LP_FIXTURES]
    items = list(la) + [S.SoftItem(c["model"]) for c in plain] + fixtures
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = S.solve_lps(hip_lib, items)
    lines = _launches(capfd)
    _check_lines(lines, "k_simplex_packed", items, pack)
    assert any(o for _, _, o, _, _ in lines) and any(not o for _, _, o, _, _ in lines)
    host = S.solve_lps(oracle_lib, items)
    S.assert_same(S.lp_states(pack), S.lp_states(host), "sets A + C")
    for i, c in enumerate(list(records) + list(plain)):
        U.check_record(pack, i, items[i], c["nPivots"], c["digest"], c["iter"], c["keys"], c["result"], (c["gen"], c["seed"]))
    for k, n in enumerate(S.SOFT_FIXTURES + S.PLAIN_LP_FIXTURES):
        g, i = U.fixture(n), len(items) - len(fixtures) + k
        U.check_record(pack, i, items[i], g["nPivots"], g["pivotDigest"], None, g["resultKeys"], g["result"], n)
    pack.close()
    host.close()


def test_recorded_trees_in_one_mixed_pack(hip_lib, oracle_lib, monkeypatch, capfd):
    """set A's MILPs next to MILPs without optional objectives: the recorded runs and the host tree byte for byte"""
    _, records = S.soft_records()
    _, plain = S.plain_records()
    _, ma = S.items_a()
    items = list(ma) + [S.SoftItem(c["model"]) for c in plain]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = S.solve_trees(hip_lib, items)
    lines = _launches(capfd)
    _check_lines(lines, "k_tree_packed", items, pack)
    host = S.solve_trees(oracle_lib, items)
    S.assert_same(S.tree_states(pack), S.tree_states(host), "set A trees")
    for i, c in enumerate(list(records) + list(plain)):
        U.check_record(pack, i, items[i], c["nPivots"], c["digest"], c["iter"], c["keys"], c["result"], (c["gen"], c["seed"]))
    assert int(pack.tree["iterations"].max()) == 41
    pack.close()
    host.close()


def test_rows_that_decide(hip_lib, oracle_lib):
    """set B, the main cost row zero: the pricing tie-break names the pivots (73 of 116 LPs) and the tree tie-break the incumbents (30 of 66
    trees reach it, 10 win it), against the oracle engine and the host tree byte for byte"""
    lb, mb = S.items_b()
    pack, host = S.solve_lps(hip_lib, lb), S.solve_lps(oracle_lib, lb)
    S.assert_same(S.lp_states(pack), S.lp_states(host), "set B LPs")
    pack.close()
    host.close()
    pack, host = S.solve_trees(hip_lib, mb), S.solve_trees(oracle_lib, mb)
    S.assert_same(S.tree_states(pack), S.tree_states(host), "set B trees")
    pack.close()
    host.close()


def test_shape_edges(hip_lib, oracle_lib, monkeypatch, capfd):
    """rows of 63 / 64 / 65 cells and the first width with partial pricing, in both builds; trees whose height crosses 64 rows"""
    items = S.dense_lp_items()
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = S.solve_lps(hip_lib, items)
    lines = _launches(capfd)
    assert sorted((t, o, n) for _, t, o, n, _ in lines) == [(64, True, 4), (256, True, 4)], lines
    assert max(b for _, _, _, _, b in lines) == max(hip_lib.jslps_lds_bytes(*it.lp[0].shape, it.n_optional) for it in items)
    host = S.solve_lps(oracle_lib, items)
    S.assert_same(S.lp_states(pack), S.lp_states(host), "dense LPs")
    assert all(r["optimal"] for r in host.results)
    # solved twice without an upload: the second call continues from the rows the first wrote back into the image
    pack.simplex()
    host.simplex()
    S.assert_same(S.lp_states(pack), S.lp_states(host), "dense LPs, a second call")
    pack.close()
    host.close()
    trees = S.dense_tree_items()
    capfd.readouterr()
    pack = S.solve_trees(hip_lib, trees)
    lines = _launches(capfd)
    assert sorted((t, o, n) for _, t, o, n, _ in lines) == [(64, True, 1), (256, True, 1)], lines
    host = S.solve_trees(oracle_lib, trees)
    S.assert_same(S.tree_states(pack), S.tree_states(host), "dense trees")
    pack.close()
    host.close()


def test_the_lds_limit(hip_lib, oracle_lib):
    h, w = 40, 65
    n_opt = 1
    while hip_lib.jslps_lds_bytes(h, w, n_opt + 1) <= LDS_LIMIT:
        n_opt += 1
    assert hip_lib.jslps_lds_bytes(h, w, n_opt) <= LDS_LIMIT < hip_lib.jslps_lds_bytes(h, w, n_opt + 1) and n_opt > 40
    fits, small = S.dense_soft(h, w, n_opt, 1), S.dense_soft(10, 63, 1, 2)
    pack, host = S.solve_lps(hip_lib, [small, fits]), S.solve_lps(oracle_lib, [small, fits])
    S.assert_same(S.lp_states(pack), S.lp_states(host), "the most optional rows that fit")
    pack.close()
    host.close()
    with pytest.raises(_capi.EngineError, match=r"\(-6\).*LP 1.*64 KiB"):
        S.lp_pack(hip_lib, [small, S.dense_soft(h, w, n_opt + 1, 1)])


def test_state_errors(hip_lib):
    it = S.dense_soft(10, 63, 2, 2)
    m, vibr, vibc, unr = it.lp
    h = ctypes.c_void_p()
    dims = [_capi.ptr_i32(_capi.as_i32(x)) for x in ([10, 10], [63, 63])]
    hip_lib.check(hip_lib.jslps_pack_create(ctypes.byref(h), 0, 2, dims[0], dims[1], _capi.ptr_f64(_capi.as_f64([1e-8, 1e-8])),
                                            _capi.ptr_i32(_capi.as_i32([0, 2])), 16, 0), "jslps_pack_create")
    try:
        for i in range(2):
            hip_lib.check(hip_lib.jslpp_pack_set(h, i, _capi.ptr_f64(_capi.as_f64(m)), _capi.ptr_i32(_capi.as_i32(vibr)),
                                                 _capi.ptr_i32(_capi.as_i32(vibc)), None, 0), "jslpp_pack_set")
        # rows reserved and not set: the upload names the LP
        assert hip_lib.jslpp_pack_upload(h) == _capi.JSLP_ERR_STATE
        assert b"LP 1" in hip_lib.jslp_last_error() and b"optional" in hip_lib.jslp_last_error()
        assert hip_lib.jslps_pack_set_optional_objectives(h, 0, _capi.ptr_f64(it.optional)) == _capi.JSLP_ERR_ARG  # none reserved for LP 0
        assert hip_lib.jslps_pack_set_optional_objectives(h, 1, None) == _capi.JSLP_ERR_ARG
        hip_lib.check(hip_lib.jslps_pack_set_optional_objectives(h, 1, _capi.ptr_f64(it.optional)), "jslps_pack_set_optional_objectives")
        hip_lib.check(hip_lib.jslpp_pack_upload(h), "jslpp_pack_upload")
        # the read-back before any solve is a state error, not a crash
        rows, n = np.full((2, 63), 7.0), ctypes.c_int32(-1)
        assert hip_lib.jslps_pack_get_optional_objectives(h, 1, _capi.ptr_f64(rows), ctypes.byref(n)) == _capi.JSLP_ERR_STATE
        assert (rows == 7.0).all() and n.value == -1
        assert hip_lib.jslps_pack_get_optional_objectives(h, 2, _capi.ptr_f64(rows), ctypes.byref(n)) == _capi.JSLP_ERR_ARG
        out = np.zeros(2, dtype=_capi.RESULT_DTYPE)
        hip_lib.check(hip_lib.jslpp_pack_simplex(h, None, out.ctypes.data, None, None), "jslpp_pack_simplex")
        assert hip_lib.jslpp_pack_launches(h) == 2
        hip_lib.check(hip_lib.jslps_pack_get_optional_objectives(h, 1, _capi.ptr_f64(rows), ctypes.byref(n)), "get")
        assert n.value == 2 and not (rows == 7.0).any()
        hip_lib.check(hip_lib.jslps_pack_get_optional_objectives(h, 0, None, ctypes.byref(n)), "get")
        assert n.value == 0
    finally:
        hip_lib.jslpp_pack_destroy(h)


def _mixed_models():
    lps, milps = S.soft_records()
    plain_lps, plain_milps = S.plain_records()
    cases = lps[:40] + milps[:30] + plain_lps + plain_milps
    return cases, [c["model"] for c in cases] + [U.fixture(n)["model"] for n in S.SOFT_FIXTURES + ["Sudoku4x4"]]


def test_solve_packed_routes_soft_models_into_the_opt_builds(hip_lib, oracle_lib, monkeypatch, capfd):
    cases, models = _mixed_models()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [Solve(m, lib=oracle_lib) for m in models]
        monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
        capfd.readouterr()
        got = solver.solve_packed(models, lib=hip_lib)
        err = capfd.readouterr().err
    assert [repr(g) for g in got] == [repr(w) for w in want]
    for c, g in zip(cases, got):  # the reference's recorded results
        assert list(g.keys()) == c["keys"]
        for k, v in c["result"].items():
            ref = v if isinstance(v, bool) else G.num(v)
            assert g[k] == ref or (isinstance(ref, float) and np.isnan(ref) and np.isnan(g[k])), (c["seed"], k)
    lines = [(k, int(t), bool(o), int(n), int(b)) for k, t, o, n, b in LAUNCH.findall(err)]
    soft = {k: sum(n for kk, _, o, n, _ in lines if kk == k and o) for k in ("k_simplex_packed", "k_tree_packed")}
    plain = {k: sum(n for kk, _, o, n, _ in lines if kk == k and not o) for k in ("k_simplex_packed", "k_tree_packed")}
    assert soft == {"k_simplex_packed": 40 + 2, "k_tree_packed": 30} and plain == {"k_simplex_packed": 12, "k_tree_packed": 12}, lines
    assert all(b <= LDS_LIMIT for _, _, _, _, b in lines)
