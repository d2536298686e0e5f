"""The fp32 twin (jslp_engine_simplex_f32: f32::k_begin / k_select / k_update, k32_convert, k32_gather) bit for bit against an fp32
restatement of the core, tests/fp32_reference.py -- the same rules in IEEE binary32, every operation rounded once, both roundings of
`eliminate` kept.

CPU (not marked gpu): the restatement at float64 equals the oracle library bit for bit on every instance (that pins its structure, and
with it the float32 instantiation); every float32 run ends well below the cap; each instance does what it is in the table for (the
"edge facts"); each deliberately wrong variant of the restatement (fp32_reference.MUTANTS) changes what the ABI returns on some instance.
GPU: Tableau.simplex_f32 returns exactly what the restatement returns -- flags, pivot counts, cycle phase, unbounded variable, height,
objective cell, the RHS column and the row map, doubles as bit patterns, `evaluation` restated from the objective cell.  No tolerance.

Not pinned: the full final fp32 matrix and the fp32 pivot trace -- neither is observable through the ABI.

The instances are the smallest shapes at which the twin's code can go wrong (one dimension kept thin so the restatement stays fast):
  small0..5       14 x 11, the tableaus of test_fp32_twin.py
  tall            1030 x 40: second turn of the 1024-thread row loops, 129 row blocks of k_update, the last with 6 rows
  wide            30 x 1100: second turn of the column loops, ld 1104 = three 512-column tiles with a partial last one, partial pricing
  w512/w513/w497  ld exactly one tile / one tile + 16 columns / a padded tail inside the tile
  two_phase, infeasible, unbounded, unrestricted    the ends and rules of the core
  cyc_*           the small cycle goldens (integer data, exact in binary32): check on; check off where the run ends without it
  subnormal       RHS scaled into the binary32 subnormals
  tenths          data that binary32 cannot hold: k32_convert's narrowing matters
"""
import functools
import glob
import os
import sys

import numpy as np
import pytest

import fp32_reference as R
import golden_util as G
from jslpsolver_amd.engine import Tableau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resident_stress import int_instance  # noqa: E402  (the dense all-"<=" integer LP of the stress tool)

PRECISIONS = (1e-3, 1e-5, 1e-7)  # the sweep's
MAX_PIVOTS = 1500                # per instance, so that a GPU case stays at a few seconds
CAP = 3000                       # the restatement raises here; the engine's own iters_cap is 2e6 + 200 (rows + columns), far above

CYCLE_GOLDENS = sorted(p for p in glob.glob(os.path.join(G.GOLDEN, "cycles", "*.json.gz")) if "embedded" not in p and "late_" not in p)


# ---- the instance table ------------------------------------------------------------------------------------------------
def _ge_rows(m, rows):
    """x_j >= b as the row -x_j <= -b: a negative RHS, so phase 1 has work"""
    for r, j, b in rows:
        m[r, :] = 0.0
        m[r, 0] = -b
        m[r, j] = -1.0


def _small(seed, H=14, W=11):
    """test_fp32_twin._tableau's data"""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W))
    m[0, 1:] = rng.integers(1, 20, W - 1)
    m[1:, 1:] = rng.integers(1, 12, (H - 1, W - 1))
    m[1:, 0] = rng.integers(30, 90, H - 1)
    vibr = np.array([-1] + list(range(W - 1, W + H - 2)), dtype=np.int32)
    vibc = np.array([-1] + list(range(W - 1)), dtype=np.int32)
    return m, vibr, vibc, ()


def _tall():
    m, vibr, vibc = int_instance(1029, 39, 1)
    m[1025:, 0] = [67, 71, 59, 63, 75]  # the rows past 1024 bind first: their limits are the smallest
    _ge_rows(m, ((1026, 5, 1.0), (1028, 12, 1.0), (300, 20, 1.0)))  # ... and phase 1 leaves through rows past 1024 too
    return m, vibr, vibc, ()


def _wide():
    m, vibr, vibc = int_instance(29, 1099, 2)
    m[0, 1:901] = -m[0, 1:901]  # nothing prices in before column 901: the first 18 batches of partial pricing are empty
    _ge_rows(m, ((7, 1050, 2.0), (19, 1077, 1.0), (23, 400, 1.0)))  # phase 1 enters through columns past 1024 too
    return m, vibr, vibc, ()


def _width(W):
    m, vibr, vibc = int_instance(20, W - 1, 3)
    return m, vibr, vibc, ()


def _two_phase():
    m, vibr, vibc = int_instance(48, 30, 4, two_phase=True)
    return m, vibr, vibc, ()


def _infeasible():
    m, vibr, vibc = int_instance(48, 30, 5, two_phase=True)
    ge = int(np.nonzero(m[1:, 0] < 0)[0][0]) + 1  # x_j >= b ...
    j = int(np.nonzero(m[ge, 1:])[0][0]) + 1
    le = int(np.nonzero(m[1:, 0] > 0)[0][0]) + 1  # ... and x_j <= 3 in a "<=" row
    m[le, :] = 0.0
    m[le, j] = 1.0
    m[le, 0] = 3.0
    return m, vibr, vibc, ()


def _unbounded():
    m, vibr, vibc = int_instance(24, 18, 6)
    m[1:, 7] = -m[1:, 7]  # nothing limits variable 6 ...
    m[0, 7] = 3.0         # ... and it prices in late
    return m, vibr, vibc, ()


def _unrestricted():
    m, vibr, vibc = int_instance(24, 18, 7)
    rng = np.random.default_rng(107)
    unr = (2, 5, 11)
    for v in unr:  # negative costs on columns of mixed sign
        m[0, 1 + v] = -m[0, 1 + v]
        m[1:, 1 + v] = -m[1:, 1 + v] * rng.integers(0, 2, 24)
    return m, vibr, vibc, unr


def _subnormal():
    m, vibr, vibc, _ = _small(8)
    m[1:, 0] *= 2.0 ** -140  # 30..89 x 2^-140: subnormal in binary32 (the smallest normal is 2^-126), exact all the same
    return m, vibr, vibc, ()


def _tenths():
    m, vibr, vibc = int_instance(20, 15, 9)
    return m / 10.0, vibr, vibc, ()


def _golden(path):
    g = G.load(path)
    m, vibr, vibc = G.dense_tableau(g["tableau"])
    return m, vibr, vibc, tuple(g["tableau"]["unrestricted"])


BUILDERS = {"small%d" % s: functools.partial(_small, s) for s in range(6)}
BUILDERS.update({"tall": _tall, "wide": _wide, "w512": functools.partial(_width, 512), "w513": functools.partial(_width, 513),
                 "w497": functools.partial(_width, 497), "two_phase": _two_phase, "infeasible": _infeasible, "unbounded": _unbounded,
                 "unrestricted": _unrestricted, "subnormal": _subnormal, "tenths": _tenths})
BUILDERS.update({"cyc_" + G.ident(p): functools.partial(_golden, p) for p in CYCLE_GOLDENS})
NAMES = list(BUILDERS)
# with the check off a cycle golden cycles for ever, in the restatement as in the engine, except where fp32 leaves the cycle: chosen by
# the CPU run (test_float32_run_ends), fixed here
ENDS_WITHOUT_CHECK = {"cyc_deg_137788": PRECISIONS, "cyc_deg_233528": (1e-7,)}
CASES = [(n, p, True) for n in NAMES for p in PRECISIONS]
CASES += [(n, p, False) for n in NAMES for p in PRECISIONS if not n.startswith("cyc_")]
CASES += [(n, p, False) for n, ps in ENDS_WITHOUT_CHECK.items() for p in ps]


def _case_id(case):
    return "%s-%g-%s" % (case[0], case[1], "check" if case[2] else "nocheck")


@functools.lru_cache(maxsize=None)
def instance(name):
    m, vibr, vibc, unr = BUILDERS[name]()
    m.setflags(write=False)
    return m, vibr, vibc, tuple(unr)


@functools.lru_cache(maxsize=None)
def expected(name, precision, check):
    """the float32 restatement's outcome: computed once, shared by every test that needs it, never changed"""
    m, vibr, vibc, unr = instance(name)
    return R.solve(m, vibr, vibc, unr, precision, check, dtype=np.float32, max_pivots=CAP)


def _trace(name, precision=1e-5, check=True):
    return np.array(expected(name, precision, check).trace, dtype=np.int64).reshape(-1, 2)


# ---- CPU: the restatement is right --------------------------------------------------------------------------------------
def _result_tuple(r):
    return (r.feasible, r.bounded, r.optimal, r.unbounded_var_index, r.pivots_phase1, r.pivots_phase2, r.cycle_phase, r.cycle_start,
            r.cycle_length, r.height, R._bits(r.obj_cell), R._bits(r.evaluation))


# (a cycle golden with the check off has no end to compare: the check stays on for those)
@pytest.mark.parametrize("name,check", [(n, True) for n in NAMES] + [(n, False) for n in NAMES if not n.startswith("cyc_")],
                         ids=lambda v: v if isinstance(v, str) else ("check" if v else "nocheck"))
def test_restatement_at_float64_is_the_oracle(oracle_lib, name, check):
    """result struct, pivot trace, final matrix and both maps, bit for bit"""
    m, vibr, vibc, unr = instance(name)
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, lib=oracle_lib)
    res = t.simplex(check_cycles=check)
    o = R.solve(m, vibr, vibc, unr, 1e-8, check, dtype=np.float64, max_pivots=CAP)
    assert _result_tuple(res) == (o.feasible, o.bounded, o.optimal, o.unbounded_var_index, o.it1, o.it2, o.cycle_phase, o.cycle_start,
                                  o.cycle_length, o.height, R._bits(o.obj_cell), R._bits(o.evaluation(0.0)))
    assert [tuple(p) for p in t.pivot_trace().tolist()] == o.trace
    fm, fr, fc, _, _ = t.download()
    assert fm.tobytes() == o.matrix.tobytes()
    assert np.array_equal(fr, o.vibr) and np.array_equal(fc, o.vibc)
    rhs, rows = t.read_rhs()
    assert rhs.tobytes() == o.rhs.tobytes() and np.array_equal(rows, o.vibr)
    t.close()


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_float32_run_ends(case):
    o = expected(*case)  # (raises at CAP)
    assert o.it1 + max(o.it2, 0) <= MAX_PIVOTS


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("cyc_")])
def test_cycle_goldens_without_the_check_are_listed_right(name):
    """ENDS_WITHOUT_CHECK is the whole list: everywhere else the float32 run with the check off is still going at the cap"""
    m, vibr, vibc, unr = instance(name)
    for p in PRECISIONS:
        if p in ENDS_WITHOUT_CHECK.get(name, ()):
            continue
        with pytest.raises(R.PivotCapExceeded):
            R.solve(m, vibr, vibc, unr, p, False, dtype=np.float32, max_pivots=CAP)


# ---- CPU: the instances are not vacuous -----------------------------------------------------------------------------------
def test_tall_leaves_through_rows_past_1024_in_both_phases():
    """second turn of the 1024-thread row loops: phase 1's most-negative-RHS reduction and the ratio test"""
    o = expected("tall", 1e-5, True)
    tr = _trace("tall")
    assert o.it1 >= 2 and o.it2 >= 2
    assert (tr[:o.it1, 0] > 1024).any(), "phase 1"
    assert (tr[o.it1:, 0] > 1024).any(), "ratio test"


def test_tall_last_row_block_is_partial_and_pivots():
    H = instance("tall")[0].shape[0]
    assert H == 1030 and H % 8 == 6 and (H + 7) // 8 == 129
    assert (_trace("tall")[:, 0] >= 1024).any()


def test_wide_enters_through_columns_past_1024_in_both_phases():
    """second turn of the 1024-thread column loops: phase 1's quotient reduction and the pricing"""
    o = expected("wide", 1e-5, True)
    tr = _trace("wide")
    assert o.it1 >= 2 and o.it2 >= 2
    assert (tr[:o.it1, 1] > 1024).any(), "phase 1"
    assert (tr[o.it1:, 1] > 1024).any(), "pricing"


def test_wide_pivots_in_the_last_column_tile_on_both_lanes_of_a_pair():
    """ld 1104: k_update's third tile holds columns 1024..1103; has_pc on .x (even column) and on .y (odd column)"""
    W = instance("wide")[0].shape[1]
    assert (W + 15) // 16 * 16 == 1104
    pcs = _trace("wide")[:, 1]
    last = pcs[pcs >= 1024]
    assert (last % 2 == 0).any() and (last % 2 == 1).any()


def test_widths_sit_at_the_tile_edges():
    for name, ld in (("w512", 512), ("w513", 528), ("w497", 512)):
        W = instance(name)[0].shape[1]
        assert (W + 15) // 16 * 16 == ld
        pcs = _trace(name)[:, 1]
        assert len(pcs) >= 20 and (pcs % 2 == 0).any() and (pcs % 2 == 1).any()
    assert (_trace("w513")[:, 1] >= 496).any(), "a pivot column in the 16 columns past the first tile, or next to them"
    assert _trace("w512")[:, 1].max() >= 480


def test_partial_pricing_is_on_and_decides():
    for name in ("wide", "w512", "w513", "w497"):
        m, vibr, vibc, unr = instance(name)
        assert R.pricing_batch(m.shape[1]) == 50
        full = R.solve(m, vibr, vibc, unr, 1e-5, True, dtype=np.float32, max_pivots=CAP, full_pricing=True)
        assert full.trace != expected(name, 1e-5, True).trace, name


def test_two_phase_has_a_phase_1():
    o = expected("two_phase", 1e-5, True)
    assert o.it1 >= 5 and o.it2 >= 5 and o.optimal


def test_infeasible_end():
    o = expected("infeasible", 1e-5, True)
    assert (o.feasible, o.optimal, o.it2) == (0, 0, -1) and o.it1 >= 2 and o.cycle_phase == 0


def test_unbounded_end_names_its_variable():
    o = expected("unbounded", 1e-5, True)
    assert (o.feasible, o.bounded, o.optimal) == (1, 0, 0) and o.it2 >= 5
    assert 0 <= o.unbounded_var_index < 18 and o.evaluation() == float("-inf")  # (a structural variable: none of them is limited any more)


def test_unrestricted_variables_enter_on_a_negative_reduced_cost():
    o = expected("unrestricted", 1e-5, True)
    assert o.neg_unrestricted_entries >= 1 and o.optimal
    assert sum(expected(n, 1e-5, True).neg_unrestricted_entries for n in NAMES if n.startswith("cyc_unr")) >= 6


def test_a_cycle_is_detected_in_float32():
    hits = [n for n in NAMES if n.startswith("cyc_") and expected(n, 1e-5, True).cycle_phase == 2]
    assert "cyc_deg_35358" in hits and "cyc_unr_15" in hits and len(hits) >= 10
    for n in hits:
        o = expected(n, 1e-5, True)
        assert (o.feasible, o.optimal) == (0, 0)


def test_cycle_golden_data_is_exact_in_binary32():
    for n in NAMES:
        if n.startswith("cyc_"):
            m = instance(n)[0]
            assert np.array_equal(m.astype(np.float32).astype(np.float64), m), n


def test_precision_changes_the_trace_somewhere():
    changed = [n for n in NAMES if len({tuple(expected(n, p, True).trace) for p in PRECISIONS}) > 1]
    assert "cyc_deg_137788" in changed and "cyc_deg_233528" in changed


def test_subnormal_instance_ends_on_subnormal_rhs_cells():
    o = expected("subnormal", 1e-5, True)
    rhs = np.abs(o.rhs[1:])
    assert ((rhs > 0) & (rhs < float(np.finfo(np.float32).tiny))).any()


def test_tenths_are_not_binary32_numbers():
    m = instance("tenths")[0]
    assert not np.array_equal(m.astype(np.float32).astype(np.float64), m)


# ---- CPU: the observable tells a wrong twin from a right one ------------------------------------------------------------------
# the instances that must catch each mutant (chosen by the CPU run; the test below also counts every case that does)
CATCHES = {
    "wide": ("small3", "tall", "wide", "w512", "w513", "w497", "two_phase", "unbounded", "unrestricted", "tenths", "cyc_deg_137788"),
    "fused": ("small3", "tall", "wide", "w512", "w513", "w497", "two_phase", "unbounded", "unrestricted", "tenths", "cyc_deg_137788"),
    "recip": ("small3", "tall", "wide", "w512", "w513", "w497", "two_phase", "unbounded", "unrestricted", "tenths", "cyc_deg_137788"),
    "ftz": ("subnormal",),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_changes_what_the_abi_returns(mutant):
    caught = []
    for name in NAMES:
        m, vibr, vibc, unr = instance(name)
        try:
            x = R.solve(m, vibr, vibc, unr, 1e-5, True, dtype=np.float32, mutant=mutant, max_pivots=CAP)
        except R.PivotCapExceeded:
            continue  # (never counted as caught)
        if x.observable() != expected(name, 1e-5, True).observable():
            caught.append(name)
    print("mutant %s is caught by: %s" % (mutant, " ".join(caught)))
    assert set(CATCHES[mutant]) <= set(caught)


# ---- GPU: the twin is the restatement --------------------------------------------------------------------------------------
def _observed(res, rhs, rows):
    return (res.feasible, res.bounded, res.optimal, res.unbounded_var_index, res.pivots_phase1, res.pivots_phase2, res.cycle_phase,
            res.height, R._bits(res.obj_cell), np.asarray(rhs, dtype=np.float64).view(np.uint64).tolist(), np.asarray(rows).tolist())


def _assert_twin(t, o, precision, check, before=0.0):
    res, rhs, rows, ms = t.simplex_f32(precision, check_cycles=check)
    got, want = _observed(res, rhs, rows), o.observable()
    for field, a, b in zip(("feasible", "bounded", "optimal", "unbounded_var_index", "pivots_phase1", "pivots_phase2", "cycle_phase",
                            "height", "obj_cell bits", "rhs bits", "row map"), got, want):
        assert a == b, field
    assert R._bits(res.evaluation) == R._bits(o.evaluation(before))
    assert ms >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_twin_equals_restatement(hip_lib, case):
    name, precision, check = case
    m, vibr, vibc, unr = instance(name)
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, row_capacity=m.shape[0] + 4, lib=hip_lib)
    _assert_twin(t, expected(*case), precision, check)
    t.close()


def _state(t):
    return [a.tobytes() for a in t.download()] + [t.pivot_trace().tobytes()]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tall", "wide"])
def test_fp64_state_is_untouched_and_the_next_fp64_solve_is_the_oracle(hip_lib, oracle_lib, name):
    m, vibr, vibc, unr = instance(name)
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, lib=hip_lib)
    before = _state(t)
    _assert_twin(t, expected(name, 1e-5, True), 1e-5, True)
    assert _state(t) == before
    ref = Tableau(m, vibr, vibc, unr, precision=1e-8, lib=oracle_lib)
    assert _result_tuple(t.simplex()) == _result_tuple(ref.simplex())
    assert _state(t) == _state(ref)
    t.close()
    ref.close()


@pytest.mark.gpu
def test_two_precisions_on_one_engine(hip_lib):
    """nothing of the first call is left over for the second: each equals its own restatement (the traces differ: see
    test_precision_changes_the_trace_somewhere)"""
    name = "cyc_deg_137788"
    m, vibr, vibc, unr = instance(name)
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, lib=hip_lib)
    for p in (1e-7, 1e-3, 1e-7):
        _assert_twin(t, expected(name, p, True), p, True)
    t.close()
    m, vibr, vibc, unr = instance("wide")
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, lib=hip_lib)
    for p in (1e-3, 1e-7):
        _assert_twin(t, expected("wide", p, True), p, True)
    t.close()


def _restated_live(t, unr, precision, check=True):
    m, vibr, vibc, _, _ = t.download()
    return R.solve(m, vibr, vibc, unr, precision, check, dtype=np.float32, max_pivots=CAP)


@pytest.mark.gpu
def test_twin_on_a_live_tableau_that_has_grown(hip_lib):
    """the fp32 slot is allocated at the first call; cuts then append rows to the live tableau (no restore), so H exceeds what the slot
    first saw -- after applyCuts (a solved tableau) and after addCutConstraints (rows with a negative RHS: a phase 1 in fp32)"""
    m, vibr, vibc, unr = instance("w513")
    H = m.shape[0]
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, row_capacity=H + 11, lib=hip_lib)  # 21 rows = 3 row blocks -> 32 rows = 4
    _assert_twin(t, expected("w513", 1e-5, True), 1e-5, True)
    assert t.simplex().optimal
    rhs, rows = t.read_rhs()
    basic = [(int(v), float(x)) for v, x in zip(rows[1:], rhs[1:]) if 0 <= v < m.shape[1] - 1 and x > 1.0]
    assert len(basic) >= 4
    cuts = [{"type": "max", "varIndex": v, "value": float(np.floor(x / 2))} for v, x in basic[:4]]
    res, _, _ = t.applyCuts(cuts)
    assert res.height == H + 4 and t.height == H + 4
    _assert_twin(t, _restated_live(t, unr, 1e-5), 1e-5, True, before=res.evaluation)
    rhs, rows = t.read_rhs()
    basic = [(int(v), float(x)) for v, x in zip(rows[1:], rhs[1:]) if 0 <= v < m.shape[1] - 1 and x > 1.0]
    t.addCutConstraints([{"type": "max", "varIndex": v, "value": float(np.floor(x / 2))} for v, x in basic[:5]])
    assert t.height == H + 9
    o = _restated_live(t, unr, 1e-5)
    assert o.it1 >= 1, "the appended rows start infeasible"
    _assert_twin(t, o, 1e-5, True, before=res.evaluation)
    t.close()


@pytest.mark.gpu
def test_twin_right_after_an_upload(hip_lib):
    """no fp64 solve between upload() and the fp32 call: the twin reads what was uploaded, not what the engine solved before"""
    m, vibr, vibc, unr = instance("two_phase")
    t = Tableau(m, vibr, vibc, unr, precision=1e-8, lib=hip_lib)
    _assert_twin(t, expected("two_phase", 1e-5, True), 1e-5, True)
    assert t.simplex().optimal
    m2, vibr2, vibc2, unr2 = instance("infeasible")  # the same shape
    assert m2.shape == m.shape
    t.upload(m2, vibr2, vibc2, unr2)
    _assert_twin(t, expected("infeasible", 1e-5, True), 1e-5, True)  # (upload() resets the engine's evaluation to 0)
    t.close()
