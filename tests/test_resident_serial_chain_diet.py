"""The lean register-resident pivot loops of the 8-row geometries (<1024,2,8> and <512,4,8>, jslp_resident_pipe.hip.h) after the serial-chain
diet (profiles/serial_chain_diet.md).  Three items were built and measured there; each has its cases here:

  A  (merged) the pricing rounds' LDS atomics (price_row_pipe rounds 1-3, the phase-1 loop's step E1) are issued by the candidate lanes themselves
     (ds_min_i32 / ds_max_u64 under the lanes' own EXEC mask, drained in front of the barrier) instead of LLVM's scalar loop + one elected lane;
  B  (measured slower, profiles/serial_chain_diet_rejected.patch) column 0's LDS mirror (sm.rhsb) brought up to date by the NEXT pivot's ratio-test wave
     from one word thread 0 leaves in step N, instead of by wave 0 in step N;
  C  (measured level, same patch) the winner's workgroup `row / rows-per-workgroup` as a multiply-shift by a reciprocal prepared in front of the loop.
The cases of B and C stay: they pin the mirror and the winner's workgroup whoever keeps the one and however the other is computed, and the
multiply-shift's exactness for whoever tries it again.

Every GPU case runs a small LP through the FORCED resident path and is compared with the CPU oracle's solve of the same LP byte for byte -- the
pivot trace, the int64 views of every array of the final tableau, the result -- and asserts the launch line.  The oracle alone says what is expected.

A.  17 x 300 (and 17 x 101).  Lane t holds columns t CPT .. t CPT + CPT - 1; a wave holds 64 CPT columns (128 at two columns per lane: three waves
hold candidates).  Phase 2 prices partially, in batches of 50 columns, so a round of its atomics sees the lanes of ONE batch: 25-26 lanes at two
columns per lane -- 64 candidate lanes in one wave or two full waves cannot occur in phase 2 at any width (W <= 101 prices all columns at once: 50
lanes).  What can be planted there is: the winning batch FILLED (every column of the batch that crosses the waves' boundary a candidate -- all
equal: rounds 2 and 3 see every lane of it, the first column wins; ascending by single ulps: the last one wins), the one-batch width with all 100
columns equal (17 x 101: 50 lanes of wave 0), equal values at the two ends of a batch and in the last lane of one wave / the first of the next
(the first column wins), 1-ulp neighbours across that boundary in both orders, a single candidate in the last column (the lane next to the padded
lanes) and no candidate at all (optimal at once).  Phase 1 does not price in batches -- its second round sees every lane that holds the best
quotient -- so THERE the full-size cases exist and are planted: all 64 lanes of wave 0 tied, two full waves tied, lanes 0 and 63 of one wave tied,
the waves' boundary tied and 1 ulp apart, a single candidate in the last column, none (infeasible).  Both through JSLP_RES_CPT=4 as well.

B.  8 rows per workgroup (JSLP_RES_RPB=8): H = 8 one workgroup, H = 13 two with padding rows in the last, H = 16 two full ones.  A dense LP (the pending row
inside my workgroup and outside it, workgroup 0's row 0, the padding rows); a first pivot whose column has entries of 0 and 1e-17 (closed gates); a pivot
row whose right-hand side is 0 and 1e-17 (column 0's entry of the normalised row is zero / under the gate; the `kind == 1` verdict); several degenerate rows; the
column that just left entering again; a phase 1 in front (the switch re-initialises the mirror); exits with a pivot pending: at optimality (every
case) and at JSLP_TEST_ITERS_CAP = 3, followed by a SECOND capped solve from the handed-over tableau.

C.  17 x 129, rows per workgroup 1 (the default), 2, 3, 7, 8 (JSLP_RES_RPB), the first pivot's winner planted in the first and in the last workgroup.
CPU: the multiply-shift restated here equals the division for every row < 2^15 and every divisor <= 32 (exhaustive)."""
import hashlib
import re

import numpy as np
import pytest

from jslpsolver_amd.engine import Tableau

SEED = 737373
PREC = 1e-8
GEOM = {2: (1024, 2, 8), 4: (512, 4, 8)}  # JSLP_RES_CPT -> (lanes, columns per lane, rows)
KNOBS = ("JSLP_TEST_ITERS_CAP", "JSLP_FORCE_PATH", "JSLP_RES_CPT", "JSLP_RES_LEAN", "JSLP_RES_GEOM", "JSLP_RES_RPB", "JSLP_RES_WIDE_TALL", "JSLP_XL",
         "JSLP_NO_WGLDS", "JSLP_INJECT_RESIDENT_ABORT_US", "JSLP_FUSED_P1", "JSLP_TEST_RESIDENT_ABORT", "JSLP_TEST_RESIDENT_LATE_WAVE0", "JSLP_SPIN_LIMIT")
LAUNCH = re.compile(r"^\[jslp\] launch (.*)$", re.M)
BATCH = 50
V = 40.0
CE = 7  # the entering column of the crafted first pivots of B and C: first pricing batch, the largest cost


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _ulps(x, k):
    return float(np.int64(_bits(x) + k).view(np.float64))


def _hashes(arrays):
    return [hashlib.sha256(np.ascontiguousarray(x).view(np.int64).tobytes() if x.dtype == np.float64 else np.ascontiguousarray(x).tobytes()).hexdigest()
            for x in arrays]


def _answer(t, res):
    return (res.as_dict(), t.pivot_trace().tolist(), _hashes(t.download()), repr(t.evaluation))


def _same(got, want):
    assert got[1] == want[1], (got[1][:4], want[1][:4])
    for k in want[0]:
        x, y = got[0][k], want[0][k]
        assert x == y or (isinstance(x, float) and np.isnan(x) and np.isnan(y)), (k, x, y)
    assert got[2] == want[2]
    assert got[3] == want[3]


def _clean(monkeypatch, cpt, rpb=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_FORCE_PATH", "resident")
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    if cpt == 4:
        monkeypatch.setenv("JSLP_RES_CPT", "4")
    if rpb is not None and rpb > 1:
        monkeypatch.setenv("JSLP_RES_RPB", str(rpb))


def _solve(lib, inst, chk):
    A, vibr, vibc = inst
    t = Tableau(A, vibr, vibc, [], precision=PREC, lib=lib)
    try:
        return _answer(t, t.simplex(check_cycles=chk)), (t.get_counters() if hasattr(lib, "backend") else None)
    finally:
        t.close()


_ORACLE = {}


def _oracle(lib, key, make):
    if key not in _ORACLE:
        _ORACLE[key] = _solve(lib, make(), True)[0]
    return _ORACLE[key]


def _forced(lib, capfd, inst, cpt, H, rpb, chk=False):
    capfd.readouterr()
    got, cnt = _solve(lib, inst, chk)
    lines = [x for x in LAUNCH.findall(capfd.readouterr().err) if x.startswith("k_simplex_resident<")]
    head = "k_simplex_resident<%d,%d,%d> unr 0 lean 1 opt 0 chk %d xl 0 G %d rpb %d" % (GEOM[cpt] + (int(chk), (H + rpb - 1) // rpb, rpb))
    assert len(lines) == 1 and lines[0].startswith(head), (lines, head)
    assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), cnt
    return got


def _maps(H, W):
    m, n = H - 1, W - 1
    return np.array([-1] + list(range(n, n + m)), dtype=np.int32), np.array([-1] + list(range(n)), dtype=np.int32)


# ---- A: the pricing rounds -------------------------------------------------------------------------------------------------------------
PH, PW, PW1 = 17, 300, 101
P2_CASES = ("filled_tie", "filled_ulps", "one_batch_tie", "tie_batch_ends", "tie_wave_edge", "ulp_wave_edge", "ulp_wave_edge_rev", "single_last", "none")
P1_CASES = ("p1_full_wave", "p1_two_waves", "p1_tie_0_63", "p1_tie_wave_edge", "p1_ulp_wave_edge", "p1_single_last", "p1_none")
P1_ROW = 3  # the one ">=" row of the phase-1 cases


def _batch_of(col):
    return (col - 1) // BATCH


def pricing_instance(case, cpt):
    """-> (A, vibr, vibc), the first entering column (None: no pivot at all)"""
    W = PW1 if case == "one_batch_tie" else PW
    rng = np.random.default_rng(SEED + 11 * cpt)
    A = np.zeros((PH, W))
    A[1:, 1:] = rng.integers(1, 21, (PH - 1, W - 1))
    A[1:, 0] = rng.integers(100, 501, PH - 1)
    cost = -rng.integers(1, 20, W).astype(np.float64)  # nothing prices in unless the case says so
    cost[0] = 0.0
    edge = 64 * cpt  # the first column of wave 1
    b = _batch_of(edge)
    lo, hi = BATCH * b + 1, min(BATCH * (b + 1), W - 1)  # the batch across the waves' boundary
    first = None
    if case in P2_CASES:
        later = np.arange(hi + 1, W)
        if case not in ("one_batch_tie", "single_last", "none"):
            cost[later] = rng.integers(50, 1000, len(later))  # larger values in later batches lose
        if case == "filled_tie":
            cost[lo:hi + 1] = V
            first = lo
        elif case == "filled_ulps":
            cost[lo:hi + 1] = [_ulps(V, k) for k in range(hi + 1 - lo)]
            first = hi
        elif case == "one_batch_tie":
            cost[1:] = V
            first = 1
        elif case == "tie_batch_ends":
            cost[lo] = cost[hi] = V
            first = lo
        elif case == "tie_wave_edge":
            cost[edge - 1] = cost[edge] = V
            first = edge - 1
        elif case == "ulp_wave_edge":
            cost[edge - 1], cost[edge] = V, _ulps(V, 1)
            first = edge
        elif case == "ulp_wave_edge_rev":
            cost[edge - 1], cost[edge] = _ulps(V, 1), V
            first = edge - 1
        elif case == "single_last":
            cost[W - 1] = V
            first = W - 1
    else:  # phase 1: one ">=" row whose entries are -1 in the set S: a column's quotient -cost / coefficient is its cost
        A[1:, 0] = rng.integers(60000, 100001, PH - 1)
        A[P1_ROW, 1:] = 0.0
        A[P1_ROW, 0] = -10.0
        S = {"p1_full_wave": range(1, edge), "p1_two_waves": range(1, 2 * edge if 2 * edge < W else W), "p1_tie_0_63": (1, edge - 1),
             "p1_tie_wave_edge": (edge - 1, edge), "p1_ulp_wave_edge": (edge - 1, edge), "p1_single_last": (W - 1,), "p1_none": ()}[case]
        S = list(S)
        A[P1_ROW, S] = -1.0
        cost[S] = V
        if case == "p1_ulp_wave_edge":
            cost[edge] = _ulps(V, 1)
        first = None if not S else (edge if case == "p1_ulp_wave_edge" else S[0])
    A[0, :] = cost
    return (A,) + _maps(PH, W), first


A_CASES = [(cpt, case) for cpt in GEOM for case in P2_CASES + P1_CASES]
A_IDS = ["cpt%d-%s" % c for c in A_CASES]


def test_planted_columns_sit_where_the_cases_say():
    assert _bits(V) & 63 == 0 and _ulps(V, 1) > V
    for cpt, (T, _c, _rows) in GEOM.items():
        edge = 64 * cpt
        lane = lambda c: c // cpt  # noqa: E731
        assert lane(edge - 1) == 63 and lane(edge) == 64 and _batch_of(edge - 1) == _batch_of(edge)  # the last lane of wave 0, the first of wave 1, one batch
        assert lane(1) == 0 and lane(edge - 1) % 64 == 63
        assert (PW + 15) // 16 * 16 <= T * cpt and PW - 1 > 2 * BATCH and int(np.floor(np.sqrt(PW - 1))) <= BATCH  # partial pricing, batches of 50
        assert PW1 - 1 <= 2 * BATCH  # ... and none: one round over every column
        assert lane(PW - 1) < lane((PW + 15) // 16 * 16 - 1)  # padded lanes behind the last column's lane
        b = _batch_of(edge)
        assert lane(BATCH * b + 1) // 64 == 0 and lane(min(BATCH * (b + 1), PW - 1)) // 64 == 1  # the filled batch has lanes in two waves
    assert 2 * 64 * 2 < PW and 130 <= PW <= 300 and 9 <= PH <= 17


@pytest.mark.parametrize("cpt,case", A_CASES, ids=A_IDS)
def test_oracle_enters_the_planted_column_first(oracle_lib, cpt, case):
    inst, first = pricing_instance(case, cpt)
    res, trace = _oracle(oracle_lib, ("A", cpt, case), lambda: inst)[:2]
    assert res["cycle_phase"] == 0, res
    if case == "none":
        assert trace == [] and res["optimal"], (res, trace[:2])
    elif case == "p1_none":
        assert trace == [] and not res["feasible"], (res, trace[:2])
    elif case in P1_CASES:
        assert res["pivots_phase1"] >= 1 and tuple(trace[0]) == (P1_ROW, first), (res, trace[:2], first)
    else:
        assert res["pivots_phase1"] == 0 and trace[0][1] == first, (res, trace[:2], first)


@pytest.mark.gpu
@pytest.mark.parametrize("cpt,case", A_CASES, ids=A_IDS)
def test_pricing_rounds_equal_oracle(hip_lib, oracle_lib, monkeypatch, capfd, cpt, case):
    _clean(monkeypatch, cpt)
    inst, _first = pricing_instance(case, cpt)
    want = _oracle(oracle_lib, ("A", cpt, case), lambda: inst)
    _same(_forced(hip_lib, capfd, inst, cpt, PH, 1), want)


# ---- B: column 0's mirror ----------------------------------------------------------------------------------------------------------------
B_KINDS = ("dense", "closed_gate", "p0_zero", "p0_tiny", "deg_many", "reenter", "phase1")
B_HEIGHTS = (8, 13, 16)


def mirror_instance(kind, H, cpt):
    W = 64 * cpt + 1
    rng = np.random.default_rng(SEED + 1000 * H + W)
    A = np.zeros((H, W))
    A[1:, 1:] = rng.integers(1, 21, (H - 1, W - 1))
    A[0, 1:] = rng.integers(1, 51, W - 1)
    A[1:, 0] = rng.integers(100, 501, H - 1)
    want = None
    if kind == "phase1":
        A[1:, 0] = rng.integers(60000, 100001, H - 1)
        for r, c in ((2, 3), (H - 1, 5)):
            A[r, 1:] = 0.0
            A[r, c] = -1.0
            A[r, 0] = -float(rng.integers(5, 21))
    elif kind != "dense":
        A[0, CE] = 60.0   # the largest cost, but not by so much that the first pivot ends the solve
        A[1:, CE] = 20.0  # every row's quotient is a twentieth of its right-hand side
        A[3, 0] = 50.0    # ... the smallest, unless the case plants another
        want = (3, CE)
    if kind == "closed_gate":  # rows whose entry of the entering column is 0 / under the 1e-16 gate: their right-hand sides stay
        A[2, CE], A[5, CE], A[H - 1, CE] = 0.0, 1e-17, -1e-17
    elif kind == "p0_zero":
        A[3, 0] = 0.0
    elif kind == "p0_tiny":
        A[3, 0] = 1e-17
    elif kind == "deg_many":
        A[2, 0] = A[4, 0] = A[H - 1, 0] = 0.0
        want = (2, CE)
    elif kind == "reenter":  # a NEGATIVE pivot element (right-hand side inside (-precision, 0)): the column's new cost is the largest again
        A[4, :] = 0.0
        A[4, 0], A[4, CE] = -9e-9, -0.5
        want = (4, CE)
    return (A,) + _maps(H, W), want


B_CASES = [(cpt, kind, H) for cpt in GEOM for kind in B_KINDS for H in B_HEIGHTS]
B_IDS = ["cpt%d-%s-H%d" % c for c in B_CASES]


@pytest.mark.parametrize("cpt,kind,H", B_CASES, ids=B_IDS)
def test_oracle_makes_the_planted_first_pivot(oracle_lib, cpt, kind, H):
    inst, want = mirror_instance(kind, H, cpt)
    res, trace = _oracle(oracle_lib, ("B", cpt, kind, H), lambda: inst)[:2]
    assert res["cycle_phase"] == 0 and len(trace) >= 2, (res, trace[:3])  # (the second pivot's ratio test reads what the first made of column 0)
    if kind == "phase1":
        assert res["pivots_phase1"] >= 2 and res["pivots_phase2"] >= 1, res
    else:
        assert res["pivots_phase1"] == 0, res
    if want is not None:
        assert tuple(trace[0]) == want, (trace[:3], want)
    if kind == "reenter":
        assert trace[1][1] == CE, trace[:3]


@pytest.mark.gpu
@pytest.mark.parametrize("cpt,kind,H", B_CASES, ids=B_IDS)
def test_mirror_by_the_ratio_test_wave_equals_oracle(hip_lib, oracle_lib, monkeypatch, capfd, cpt, kind, H):
    _clean(monkeypatch, cpt, 8)
    inst, _want = mirror_instance(kind, H, cpt)
    want = _oracle(oracle_lib, ("B", cpt, kind, H), lambda: inst)
    _same(_forced(hip_lib, capfd, inst, cpt, H, 8, chk=kind in ("dense", "phase1")), want)


CAP = 3
_REPLAY = {}


def _replay(lib, cpt, H, n):
    """the hashes of what the oracle's own pivot() makes of the first n pivots of its trace"""
    if (cpt, H, n) not in _REPLAY:
        inst, _w = mirror_instance("dense", H, cpt)
        trace = _oracle(lib, ("B", cpt, "dense", H), lambda: inst)[1]
        assert len(trace) > n
        t = Tableau(*inst, [], precision=PREC, lib=lib)
        try:
            for pr, pc in trace[:n]:
                t.pivot(pr, pc)
            _REPLAY[(cpt, H, n)] = (trace[:n], _hashes(t.download()))
        finally:
            t.close()
    return _REPLAY[(cpt, H, n)]


@pytest.mark.parametrize("cpt,H", [(cpt, H) for cpt in GEOM for H in B_HEIGHTS])
def test_oracle_trace_outlasts_two_caps(oracle_lib, cpt, H):
    assert len(_replay(oracle_lib, cpt, H, 2 * CAP)[0]) == 2 * CAP and len(_replay(oracle_lib, cpt, H, CAP)[0]) == CAP


@pytest.mark.gpu
@pytest.mark.parametrize("cpt,H", [(cpt, H) for cpt in GEOM for H in B_HEIGHTS])
def test_capped_exit_then_a_second_solve_equal_the_truncated_replays(hip_lib, oracle_lib, monkeypatch, capfd, cpt, H):
    from jslpsolver_amd._capi import EngineError
    _clean(monkeypatch, cpt, 8)
    monkeypatch.setenv("JSLP_TEST_ITERS_CAP", str(CAP))
    trace1, hashes1 = _replay(oracle_lib, cpt, H, CAP)
    trace2, hashes2 = _replay(oracle_lib, cpt, H, 2 * CAP)
    inst, _w = mirror_instance("dense", H, cpt)
    capfd.readouterr()
    t = Tableau(*inst, [], precision=PREC, lib=hip_lib)
    try:
        with pytest.raises(EngineError, match="iteration"):
            t.simplex(check_cycles=False)
        got1 = (t.pivot_trace().tolist(), _hashes(t.download()))
        with pytest.raises(EngineError, match="iteration"):  # from the handed-over tableau: the mirror starts again from column 0 as the epilogue left it
            t.simplex(check_cycles=False)
        got2 = (t.pivot_trace().tolist(), _hashes(t.download()))
        cnt = t.get_counters()
    finally:
        t.close()
    lines = [x for x in LAUNCH.findall(capfd.readouterr().err) if x.startswith("k_simplex_resident<")]
    head = "k_simplex_resident<%d,%d,%d> unr 0 lean 1 opt 0 chk 0 xl 0 G %d rpb 8" % (GEOM[cpt] + ((H + 7) // 8,))
    assert len(lines) == 2 and all(x.startswith(head) for x in lines), (lines, head)
    assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (2, 0, 0), cnt
    assert got1[0] == trace1 and got1[1] == hashes1, (got1[0], trace1)
    assert got2[0] in (trace2, trace2[CAP:]) and got2[1] == hashes2, (got2[0], trace2)


# ---- C: from the verdict to the winner's workgroup ------------------------------------------------------------------------------------------
C_H = 17
C_RPB = (1, 2, 3, 7, 8)


def winner_instance(where, cpt):
    (A, vibr, vibc), _w = mirror_instance("closed_gate", C_H, cpt)  # (any crafted kind: column CE of twenties, the largest cost)
    A[1:, CE] = 20.0
    row = 1 if where == "first" else C_H - 1
    A[row, 0] = 1e-3  # the smallest quotient by far
    return (A, vibr, vibc), (row, CE)


C_CASES = [(cpt, rpb, where) for cpt in GEOM for rpb in C_RPB for where in ("first", "last")]
C_IDS = ["cpt%d-rpb%d-%s" % c for c in C_CASES]


def test_multiply_shift_equals_the_division():
    r = np.arange(1 << 15, dtype=np.uint64)
    for rpb in range(1, 33):
        m = np.uint64((1 << 27) // rpb + 1)
        assert int(m) < (1 << 32)
        lhs = ((r << np.uint64(5)) * m) >> np.uint64(32)  # __umulhi(r << 5, m): r << 5 < 2^20 and m <= 2^27 + 1 -- the product stays below 2^48
        assert np.array_equal(lhs, r // np.uint64(rpb)), rpb


@pytest.mark.parametrize("cpt,where", [(cpt, w) for cpt in GEOM for w in ("first", "last")])
def test_oracle_picks_the_planted_workgroup(oracle_lib, cpt, where):
    inst, want = winner_instance(where, cpt)
    res, trace = _oracle(oracle_lib, ("C", cpt, where), lambda: inst)[:2]
    assert res["pivots_phase1"] == 0 and res["cycle_phase"] == 0 and tuple(trace[0]) == want and len(trace) >= 2, (res, trace[:3])
    for rpb in C_RPB:
        assert want[0] // rpb == (1 // rpb if where == "first" else (C_H + rpb - 1) // rpb - 1)  # (one row per workgroup: workgroup 0 holds the cost row alone)


@pytest.mark.gpu
@pytest.mark.parametrize("cpt,rpb,where", C_CASES, ids=C_IDS)
def test_winner_found_in_the_planted_workgroup(hip_lib, oracle_lib, monkeypatch, capfd, cpt, rpb, where):
    _clean(monkeypatch, cpt, rpb)
    inst, _want = winner_instance(where, cpt)
    want = _oracle(oracle_lib, ("C", cpt, where), lambda: inst)
    _same(_forced(hip_lib, capfd, inst, cpt, C_H, rpb), want)
