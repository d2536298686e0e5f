"""jslpf_simplex_f32_sweep (include/jslpf_f32.h) on the GPU: the one-launch kernel k32_simplex_lds, one workgroup per tolerance, held bit
for bit to the fp32 restatement of the core (tests/fp32_reference.py) on every instance of test_fp32_exact's table and on the instances at
the kernel's own tile edges (test_f32_sweep_edges); the select + update path and single simplex_f32 calls agree with it; runs share
nothing; the fp64 state stays untouched; the LDS fit decides the path.  No tolerance anywhere."""
import numpy as np
import pytest

import fp32_reference as R
from jslpsolver_amd import _capi
from jslpsolver_amd.engine import Tableau
from test_f32_sweep_edges import EDGE_NAMES, FITS_H, edge_expected, edge_instance
from test_fp32_exact import ENDS_WITHOUT_CHECK, NAMES, PRECISIONS, _observed, _restated_live, _result_tuple, _state, expected, instance

pytestmark = pytest.mark.gpu

ALL_NAMES = NAMES + [n for n in EDGE_NAMES if n != "overflows"]  # ("overflows" cannot take the kernel: test_lds_fit_decides)
# (name, check, precisions): the check on everywhere; off only where the run ends without it (test_fp32_exact.CASES' rule)
SWEEPS = [(n, True, PRECISIONS) for n in ALL_NAMES]
SWEEPS += [(n, False, PRECISIONS) for n in ALL_NAMES if not n.startswith("cyc_")]
SWEEPS += [(n, False, tuple(ps)) for n, ps in ENDS_WITHOUT_CHECK.items()]
FIELDS = ("feasible", "bounded", "optimal", "unbounded_var_index", "pivots_phase1", "pivots_phase2", "cycle_phase", "height", "obj_cell bits",
          "rhs bits", "row map")


def _tableau(name, lib, **kw):
    m, vibr, vibc, unr = edge_instance(name)
    return Tableau(m, vibr, vibc, unr, precision=1e-8, lib=lib, **kw)


def _assert_run(run, o, before=0.0):
    res, rhs, rows = run
    for field, a, b in zip(FIELDS, _observed(res, rhs, rows), o.observable()):
        assert a == b, field
    assert R._bits(res.evaluation) == R._bits(o.evaluation(before))
    assert (res.cycle_start, res.cycle_length) == (0, 0)  # as jslp_engine_simplex_f32 leaves them


def _assert_sweep(t, wants, precisions, check, path="one_launch", taken=2, before=0.0):
    runs, path_taken, ms = t.simplex_f32_sweep(precisions, check_cycles=check, path=path)
    assert path_taken == taken and ms >= 0 and len(runs) == len(precisions)
    for run, o in zip(runs, wants):
        _assert_run(run, o, before)
    return runs


def _same_runs(a, b):
    assert len(a) == len(b)
    for (ra, rhsa, rowsa), (rb, rhsb, rowsb) in zip(a, b):
        assert _observed(ra, rhsa, rowsa) == _observed(rb, rhsb, rowsb)
        assert _result_tuple(ra) == _result_tuple(rb)


# ---- bit-for-bit parity of the one-launch kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,check,precisions", SWEEPS, ids=["%s-%s-%d" % (n, "check" if c else "nocheck", len(p)) for n, c, p in SWEEPS])
def test_one_launch_sweep_equals_restatement(hip_lib, monkeypatch, capfd, name, check, precisions):
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    t = _tableau(name, hip_lib)
    capfd.readouterr()
    _assert_sweep(t, [edge_expected(name, p, check) for p in precisions], precisions, check)
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[jslp] launch")]
    assert len(lines) == 1 and lines[0].startswith("[jslp] launch k32_simplex_lds<1024> n %d lds " % len(precisions)), lines
    t.close()


# ---- the paths agree ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tall", "wide", "unrestricted", "subnormal", "cyc_deg_137788"])
def test_paths_and_single_calls_agree(hip_lib, name):
    t = _tableau(name, hip_lib)
    wants = [expected(name, p, True) for p in PRECISIONS]
    one = _assert_sweep(t, wants, PRECISIONS, True, "one_launch", 2)
    loop = _assert_sweep(t, wants, PRECISIONS, True, "select_update", 1)
    _same_runs(one, loop)
    singles = []
    for p in PRECISIONS:
        res, rhs, rows, _ = t.simplex_f32(p, check_cycles=True)
        singles.append((res, rhs, rows))
    _same_runs(one, singles)
    t.close()


# ---- runs share nothing -------------------------------------------------------------------------------------------------------
def test_runs_of_one_launch_share_nothing(hip_lib):
    name, precisions = "cyc_deg_137788", (1e-7, 1e-3, 1e-7)
    wants = [expected(name, p, True) for p in precisions]
    assert wants[0].trace != wants[1].trace
    t = _tableau(name, hip_lib)
    runs = _assert_sweep(t, wants, precisions, True)
    _same_runs(runs[:1], runs[2:])
    t.close()


def test_sweep_of_one_and_of_sixty_four(hip_lib):
    t = _tableau("small0", hip_lib)
    _assert_sweep(t, [expected("small0", 1e-5, True)], (1e-5,), True)
    precisions = tuple(PRECISIONS[i % 3] for i in range(64))
    _assert_sweep(t, [expected("small0", p, True) for p in precisions], precisions, True)
    _assert_sweep(t, [expected("small0", 1e-3, True)], (1e-3,), True)  # (the grown arena serves a short sweep again)
    assert t.simplex_f32_sweep((), path="one_launch")[0] == []
    with pytest.raises(_capi.EngineError, match=r"\(-1\)"):
        t.simplex_f32_sweep((1e-5,) * 65, path="one_launch")
    t.close()


# ---- the engine's state -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tall", "wide"])
def test_fp64_state_is_untouched_and_the_next_fp64_solve_is_the_oracle(hip_lib, oracle_lib, name):
    t = _tableau(name, hip_lib)
    before = _state(t)
    hip_lib.check(hip_lib.jslp_engine_set_counting(t._h, 1), "jslp_engine_set_counting")
    _assert_sweep(t, [expected(name, p, True) for p in PRECISIONS], PRECISIONS, True)
    assert _state(t) == before
    counters = _capi.WorkCounters()
    hip_lib.check(hip_lib.jslp_engine_get_counters(t._h, _capi.C.byref(counters)), "jslp_engine_get_counters")
    assert not any(counters.as_dict().values()), "the runs are not counted"
    hip_lib.check(hip_lib.jslp_engine_set_counting(t._h, 0), "jslp_engine_set_counting")
    ref = _tableau(name, oracle_lib)
    assert _result_tuple(t.simplex()) == _result_tuple(ref.simplex())
    assert _state(t) == _state(ref)
    t.close()
    ref.close()


def test_sweep_right_after_an_upload(hip_lib):
    m, vibr, vibc, unr = instance("two_phase")
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, lib=hip_lib)
    _assert_sweep(t, [expected("two_phase", p, True) for p in PRECISIONS], PRECISIONS, True)
    assert t.simplex().optimal
    m2, vibr2, vibc2, unr2 = instance("infeasible")  # the same shape
    t.upload(m2, vibr2, vibc2, unr2)
    _assert_sweep(t, [expected("infeasible", p, True) for p in PRECISIONS], PRECISIONS, True)  # (upload() resets the evaluation to 0)
    t.close()


def test_sweep_on_a_live_tableau_that_has_grown(hip_lib):
    """as test_twin_on_a_live_tableau_that_has_grown: cuts append rows to the live tableau, so H exceeds what the fp32 arena first saw --
    after applyCuts (a solved tableau) and after addCutConstraints (rows with a negative RHS: a phase 1 in fp32)"""
    m, vibr, vibc, unr = instance("w513")
    H = m.shape[0]
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, row_capacity=H + 11, lib=hip_lib)
    _assert_sweep(t, [expected("w513", p, True) for p in PRECISIONS], PRECISIONS, True)
    assert t.simplex().optimal
    rhs, rows = t.read_rhs()
    basic = [(int(v), float(x)) for v, x in zip(rows[1:], rhs[1:]) if 0 <= v < m.shape[1] - 1 and x > 1.0]
    assert len(basic) >= 4
    res, _, _ = t.applyCuts([{"type": "max", "varIndex": v, "value": float(np.floor(x / 2))} for v, x in basic[:4]])
    assert res.height == H + 4
    _assert_sweep(t, [_restated_live(t, unr, p) for p in PRECISIONS], PRECISIONS, True, before=res.evaluation)
    rhs, rows = t.read_rhs()
    basic = [(int(v), float(x)) for v, x in zip(rows[1:], rhs[1:]) if 0 <= v < m.shape[1] - 1 and x > 1.0]
    t.addCutConstraints([{"type": "max", "varIndex": v, "value": float(np.floor(x / 2))} for v, x in basic[:5]])
    assert t.height == H + 9
    wants = [_restated_live(t, unr, p) for p in PRECISIONS]
    assert wants[1].it1 >= 1, "the appended rows start infeasible"
    _assert_sweep(t, wants, PRECISIONS, True, before=res.evaluation)
    t.close()


def test_single_calls_and_sweeps_take_turns(hip_lib):
    """the arena grows from one copy to three and copy 0 stays what simplex_f32 uses"""
    name = "cyc_deg_137788"
    t = _tableau(name, hip_lib)
    wants = [expected(name, p, True) for p in PRECISIONS]

    def single(i):
        res, rhs, rows, _ = t.simplex_f32(PRECISIONS[i], check_cycles=True)
        _assert_run((res, rhs, rows), wants[i])

    single(0)
    _assert_sweep(t, wants, PRECISIONS, True)
    single(2)
    _assert_sweep(t, wants[::-1], PRECISIONS[::-1], True)
    single(1)
    t.close()


# ---- the LDS fit decides the path ---------------------------------------------------------------------------------------------
def test_lds_fit_decides(hip_lib):
    fits = _tableau("fits", hip_lib)
    assert fits.row_capacity == FITS_H
    _assert_sweep(fits, [edge_expected("fits", p, True) for p in PRECISIONS], PRECISIONS, True, "auto", 2)
    fits.close()
    over = _tableau("overflows", hip_lib)
    for check in (True, False):
        _assert_sweep(over, [edge_expected("overflows", p, check) for p in PRECISIONS], PRECISIONS, check, "auto", 1)
    with pytest.raises(_capi.EngineError, match=r"\(%d\)" % _capi.JSLP_ERR_UNSUPPORTED):
        over.simplex_f32_sweep(PRECISIONS, path="one_launch")
    over.close()
    roomy = _tableau("fits", hip_lib, row_capacity=FITS_H + 1)  # the row capacity, not the live height, is what must fit
    with pytest.raises(_capi.EngineError, match=r"\(%d\)" % _capi.JSLP_ERR_UNSUPPORTED):
        roomy.simplex_f32_sweep(PRECISIONS, path="one_launch")
    roomy.close()


def test_refusals_that_need_the_engine(hip_lib):
    m, vibr, vibc, unr = instance("small0")
    oo = np.zeros((1, m.shape[1]))
    oo[0, 1:] = 1.0
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, lib=hip_lib, optional_objectives=oo)
    for path in ("auto", "select_update", "one_launch"):
        with pytest.raises(_capi.EngineError, match=r"\(%d\)" % _capi.JSLP_ERR_UNSUPPORTED):
            t.simplex_f32_sweep(PRECISIONS, path=path)
    t.close()
    t = _tableau("small0", hip_lib)
    H = m.shape[0]
    prec = _capi.as_f64(PRECISIONS)
    out = (_capi.SimplexResult * 3)()
    rhs = np.full((3, H), 7.0)
    rc = hip_lib.jslpf_simplex_f32_sweep(t._h, _capi.ptr_f64(prec), 3, 1, _capi.JSLPF_PATH_ONE_LAUNCH, out, _capi.ptr_f64(rhs), None, H - 1, None,
                                         None, None)
    assert rc == _capi.JSLP_ERR_ARG and b"stride" in hip_lib.jslp_last_error() and (rhs == 7.0).all()
    h = _capi.C.c_void_p()  # created, never uploaded
    hip_lib.check(hip_lib.jslp_engine_create(_capi.C.byref(h), 0, H, m.shape[1], H, 1e-8), "jslp_engine_create")
    assert hip_lib.jslpf_simplex_f32_sweep(h, _capi.ptr_f64(prec), 3, 1, 0, out, None, None, 0, None, None, None) == _capi.JSLP_ERR_STATE
    hip_lib.jslp_engine_destroy(h)
    _assert_sweep(t, [expected("small0", p, True) for p in PRECISIONS], PRECISIONS, True)  # the engine is none the worse
    t.close()
