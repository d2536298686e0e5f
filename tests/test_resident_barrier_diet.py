"""The lean register-resident loops of the 8-row geometries (<1024,2,8> and <512,4,8>, jslp_resident_pipe.hip.h) after the barrier diet
(profiles/barrier_diet.md): the gather closes in ONE plain barrier -- the polling wave's lane 0 stores its verdict ("the looks came home") next
to the winner, every thread reads both in one LDS word -- instead of the runtime's three-barrier vote.  The diet's second item, pricing in two
LDS-atomic rounds on packed keys, was measured slower and is not in the tree (profiles/barrier_diet_rejected.patch); its cases stay: they pin
the pricing's order where two candidates differ by single ulps, whatever form the reduction takes, and the key scheme itself for whoever
tries it again.

Every GPU case runs a small LP through the FORCED resident path and is checked against the CPU oracle's solve of the same LP bit for bit: the
pivot trace, the int64 views of every array of the final tableau, the result.  The oracle alone says what is expected.

Gather.  Heights 8 (one workgroup: a gather of one), 9 and 16 (two), 17 (three) at 8 rows per workgroup; widths one column past a wave's
last lane (64 CPT + 1) and W = ld (64 CPT + 16); a dense LP (phase 2 only) and one with two ">=" rows (the phase-1 loop, then phase 2); the
same with the host's abort request raised (JSLP_INJECT_RESIDENT_ABORT_US: whether or not the kernel meets it, the answer is the oracle's).
On the test build of the library: JSLP_TEST_RESIDENT_ABORT = 0, 1, 2 -- the last workgroup gives up at that pivot, the others' gathers fail:
the verdict word's first uses -- with a short JSLP_SPIN_LIMIT: rolled back, solved again, the oracle's answer, the abort counted; and
JSLP_TEST_RESIDENT_LATE_WAVE0 = 2, 3: a late polling wave holds everybody at the single barrier, no pivot is lost.

Pricing near ties, planted in the cost row so that the FIRST pivot is decided by them (17 x 330: partial pricing in batches of 50 columns,
the last one 29 columns short; 17 workgroups of one row).  `v` = 40.0, whose low six mantissa bits are zero:
  ulp1 / ulp63     v and v + 1 ulp / v + 63 ulp                                                      -> the larger (planted at the LATER column)
  ulp64            v + 63 ulp and v + 127 ulp: exactly 64 ulp apart                                  -> the larger (the later column)
  tie              equal values                                                                      -> the smaller column
    ... each with the two columns in one lane, in two lanes of one wave, and in two waves; larger values wait in later batches
  earlier_batch    a candidate one ulp above the precision against 1e300 and +Infinity in the next batch  -> the earlier batch
  last_batch       candidates only in the last, short batch (a tie and a near tie there)
  unr_negative     an unrestricted column of cost -(v + 1 ulp) against v: |reduced cost| decides, the sign travels with it
(1 / 63 / 64 ulp: values that share, and just do not share, the top 57 bits -- where a key that splits the value would go wrong.)

CPU part: the oracle enters the planted column first; and the two packed keys of the rejected patch, restated here, pick the lexicographic
(batch ascending, value descending, column ascending) winner over adversarial and random bit patterns."""
import hashlib
import re

import numpy as np
import pytest

from jslpsolver_amd.engine import Tableau

SEED = 626262
PREC = 1e-8
GEOM = {1: (1024, 2, 8), 2: (512, 4, 8)}  # JSLP_RES_GEOM -> (lanes, columns per lane, rows): the geometries that got the one-barrier gather
KNOBS = ("JSLP_TEST_ITERS_CAP", "JSLP_FORCE_PATH", "JSLP_RES_CPT", "JSLP_RES_LEAN", "JSLP_RES_GEOM", "JSLP_RES_RPB", "JSLP_RES_WIDE_TALL", "JSLP_XL",
         "JSLP_NO_WGLDS", "JSLP_INJECT_RESIDENT_ABORT_US", "JSLP_FUSED_P1", "JSLP_TEST_RESIDENT_ABORT", "JSLP_TEST_RESIDENT_LATE_WAVE0", "JSLP_SPIN_LIMIT")
LAUNCH = re.compile(r"^\[jslp\] launch (.*)$", re.M)
BATCH = 50


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


def _clean(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_FORCE_PATH", "resident")
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")


# ---- the gather's verdict --------------------------------------------------------------------------------------------------------
def gather_instance(kind, H, W):
    rng = np.random.default_rng(SEED + 1000 * H + W)
    m, n = H - 1, W - 1
    A = np.zeros((H, W))
    A[1:, 1:] = rng.integers(1, 21, (m, n)) + rng.integers(0, 64, (m, n)) / 64.0
    A[0, 1:] = rng.integers(1, 51, n)
    A[1:, 0] = rng.integers(100, 501, m)
    if kind == "phase1":  # two ">=" rows (negated: negative right-hand sides), one variable each
        A[1:, 0] = rng.integers(60000, 100001, m)
        for rr, c in ((2, 3), (H - 1, 5)):
            A[rr, 1:] = 0.0
            A[rr, c] = -1.0
            A[rr, 0] = -float(rng.integers(5, 21))
    vibr = np.array([-1] + list(range(n, n + m)), dtype=np.int32)
    vibc = np.array([-1] + list(range(n)), dtype=np.int32)
    return A, vibr, vibc


def _widths(cpt):
    return (64 * cpt + 1, 64 * cpt + 16)


GATHER_CASES = [(g, kind, H, W) for g in GEOM for H in (8, 9, 16, 17) for W in _widths(GEOM[g][1]) for kind in ("dense", "phase1")]
GATHER_IDS = ["g%d-%s-%dx%d" % c for c in GATHER_CASES]
HOOK_CASES = [(g, kind, 17, _widths(GEOM[g][1])[0]) for g in GEOM for kind in ("dense", "phase1")] + [(1, "dense", 8, _widths(2)[1])]
HOOK_IDS = ["g%d-%s-%dx%d" % c for c in HOOK_CASES]
_ORACLE = {}


def _gather_oracle(lib, kind, H, W):
    if (kind, H, W) not in _ORACLE:
        A, vibr, vibc = gather_instance(kind, H, W)
        t = Tableau(A, vibr, vibc, [], precision=PREC, lib=lib)
        try:
            _ORACLE[(kind, H, W)] = _answer(t, t.simplex(check_cycles=True))
        finally:
            t.close()
    return _ORACLE[(kind, H, W)]


def _gather_solve(lib, g, kind, H, W, chk, capfd):
    T, cpt, rows = GEOM[g]
    A, vibr, vibc = gather_instance(kind, H, W)
    capfd.readouterr()
    t = Tableau(A, vibr, vibc, [], precision=PREC, lib=lib)
    try:
        got = _answer(t, t.simplex(check_cycles=chk))
        cnt = t.get_counters()
    finally:
        t.close()
    lines = [x for x in LAUNCH.findall(capfd.readouterr().err) if x.startswith("k_simplex_resident<")]
    head = "k_simplex_resident<%d,%d,%d> unr 0 lean 1 opt 0 chk %d xl 0 G %d rpb %d" % (T, cpt, rows, int(chk), (H + rows - 1) // rows, rows)
    assert len(lines) >= 1 and lines[0].startswith(head), (lines, head)
    return got, cnt, lines


@pytest.mark.parametrize("g,kind,H,W", GATHER_CASES, ids=GATHER_IDS)
def test_oracle_runs_the_loops_the_case_names(oracle_lib, g, kind, H, W):
    res = _gather_oracle(oracle_lib, kind, H, W)[0]
    assert res["optimal"] and res["cycle_phase"] == 0 and res["pivots_phase2"] >= 3, res
    assert (res["pivots_phase1"] >= 2) if kind == "phase1" else (res["pivots_phase1"] == 0), res
    assert W > 64 * GEOM[g][1] and (W + 15) // 16 * 16 <= GEOM[g][0] * GEOM[g][1]


@pytest.mark.gpu
@pytest.mark.parametrize("host_abort", (False, True), ids=("plain", "hostabort"))
@pytest.mark.parametrize("g,kind,H,W", GATHER_CASES, ids=GATHER_IDS)
def test_gather_verdict_equals_oracle(hip_lib, oracle_lib, monkeypatch, capfd, g, kind, H, W, host_abort):
    _clean(monkeypatch)
    monkeypatch.setenv("JSLP_RES_GEOM", str(g))
    monkeypatch.setenv("JSLP_RES_RPB", str(GEOM[g][2]))
    if host_abort:
        monkeypatch.setenv("JSLP_INJECT_RESIDENT_ABORT_US", "1")
    want = _gather_oracle(oracle_lib, kind, H, W)
    got, cnt, lines = _gather_solve(hip_lib, g, kind, H, W, kind == "dense", capfd)  # (both builds: the dense solves run the cycle-check one)
    _same(got, want)
    if host_abort:  # (the word is looked at every 1024 pivots: a short solve may well finish before it is seen -- either way the answer stands)
        assert cnt["resident_aborts"] in (0, 1), cnt
    else:
        assert len(lines) == 1 and (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), (cnt, lines)


@pytest.mark.gpu
@pytest.mark.parametrize("abort_at", (0, 1, 2))
@pytest.mark.parametrize("g,kind,H,W", HOOK_CASES, ids=HOOK_IDS)
def test_failed_gather_rolls_back_to_the_oracles_answer(hip_hooks_lib, oracle_lib, monkeypatch, capfd, g, kind, H, W, abort_at):
    _clean(monkeypatch)
    monkeypatch.setenv("JSLP_RES_GEOM", str(g))
    monkeypatch.setenv("JSLP_RES_RPB", str(GEOM[g][2]))
    monkeypatch.setenv("JSLP_TEST_RESIDENT_ABORT", str(abort_at))
    monkeypatch.setenv("JSLP_SPIN_LIMIT", "4096")
    want = _gather_oracle(oracle_lib, kind, H, W)
    got, cnt, _lines = _gather_solve(hip_hooks_lib, g, kind, H, W, False, capfd)
    _same(got, want)
    assert cnt["resident_aborts"] >= 1, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("late", (2, 3))
@pytest.mark.parametrize("g,kind,H,W", HOOK_CASES, ids=HOOK_IDS)
def test_late_polling_wave_loses_no_pivot(hip_hooks_lib, oracle_lib, monkeypatch, capfd, g, kind, H, W, late):
    _clean(monkeypatch)
    monkeypatch.setenv("JSLP_RES_GEOM", str(g))
    monkeypatch.setenv("JSLP_RES_RPB", str(GEOM[g][2]))
    monkeypatch.setenv("JSLP_TEST_RESIDENT_LATE_WAVE0", str(late))
    want = _gather_oracle(oracle_lib, kind, H, W)
    got, cnt, lines = _gather_solve(hip_hooks_lib, g, kind, H, W, kind == "dense", capfd)
    _same(got, want)
    assert len(lines) == 1 and (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), (cnt, lines)


# ---- pricing near ties -----------------------------------------------------------------------------------------------------------
PH, PW = 17, 330
V = 40.0
SPOTS = ("lane", "lanes", "waves")
NEAR = {"ulp1": (0, 1), "ulp63": (0, 63), "ulp64": (63, 127), "tie": (0, 0)}  # ulps above V of the first / the second column


def _batch_of(col):
    return (col - 1) // BATCH


def _pair(cpt, spot):
    """two columns of one pricing batch (the one across the waves' boundary): in one lane (the last of wave 0) / in two lanes of wave 1 / in the last lane
    of wave 0 and the second lane of wave 1"""
    edge = 64 * cpt  # the first column of wave 1
    if spot == "lane":
        return edge - cpt, edge - cpt + 1
    if spot == "lanes":
        return edge + cpt, edge + 3 * cpt
    return edge - 1, edge + cpt


def pricing_instance(case, g):
    """-> (A, vibr, vibc, unrestricted variables, the first entering column)"""
    cpt = GEOM[g][1]
    rng = np.random.default_rng(SEED + 7 * g)
    m, n = PH - 1, PW - 1
    A = np.zeros((PH, PW))
    A[1:, 1:] = rng.integers(1, 21, (m, n))
    A[1:, 0] = rng.integers(100, 501, m)
    cost = -rng.integers(1, 20, PW).astype(np.float64)  # nothing prices in unless the case says so
    cost[0] = 0.0
    unr = []
    name, _, spot = case.partition("@")
    if name in NEAR:
        ca, cb = _pair(cpt, spot)
        assert _batch_of(ca) == _batch_of(cb)
        later = np.arange(BATCH * (_batch_of(cb) + 1) + 1, PW)
        cost[later] = rng.integers(50, 1000, len(later))  # larger values in later batches lose
        ka, kb = NEAR[name]
        cost[ca], cost[cb] = _ulps(V, ka), _ulps(V, kb)
        first = ca if name == "tie" else cb
    elif name == "earlier_batch":
        hi = BATCH * (_batch_of(64 * cpt) + 1)  # the last column of the batch across the waves' boundary; hi and hi + 1 .. share no batch
        cost[hi] = _ulps(PREC, 1)
        cost[hi + 1] = 1e300
        cost[hi + 2] = np.inf
        first = hi
    elif name == "last_batch":
        assert _batch_of(PW - 1) == 6 and (PW - 1) % BATCH == 29  # the short one
        cost[[PW - 5, PW - 2]] = _ulps(V, 5)
        cost[PW - 1] = _ulps(V, 4)
        cost[PW - 3] = PREC  # (at the precision: no candidate)
        first = PW - 5
    elif name == "unr_negative":
        unr = [0, 1, 2]  # variables 0..2 = columns 1..3
        A[2:PH - 1, 1:4] *= np.where(rng.random((PH - 3, 3)) < 0.5, -1.0, 1.0)  # bounded both ways
        cost[1:4] = [5.0, -_ulps(V, 1), 9.0]
        cost[40] = V
        first = 2
    else:
        raise ValueError(case)
    A[0, :] = cost
    vibr = np.array([-1] + list(range(n, n + m)), dtype=np.int32)
    vibc = np.array([-1] + list(range(n)), dtype=np.int32)
    return A, vibr, vibc, unr, first


PRICING_CASES = [(g, "%s@%s" % (k, s)) for g in GEOM for k in NEAR for s in SPOTS] + \
                [(g, k) for g in GEOM for k in ("earlier_batch", "last_batch", "unr_negative")]
PRICING_IDS = ["g%d-%s" % c for c in PRICING_CASES]
_PORACLE = {}


def _pricing_solve(lib, g, case, chk):
    A, vibr, vibc, unr, _first = pricing_instance(case, g)
    t = Tableau(A, vibr, vibc, unr, precision=PREC, lib=lib)
    try:
        return _answer(t, t.simplex(check_cycles=chk)), (t.get_counters() if hasattr(lib, "backend") else None)
    finally:
        t.close()


def _pricing_oracle(lib, g, case):
    if (g, case) not in _PORACLE:
        _PORACLE[(g, case)] = _pricing_solve(lib, g, case, True)[0]
    return _PORACLE[(g, case)]


@pytest.mark.parametrize("g,case", PRICING_CASES, ids=PRICING_IDS)
def test_oracle_enters_the_planted_column_first(oracle_lib, g, case):
    res, trace = _pricing_oracle(oracle_lib, g, case)[:2]
    first = pricing_instance(case, g)[4]
    assert res["pivots_phase1"] == 0 and res["cycle_phase"] == 0 and len(trace) >= 1 and trace[0][1] == first, (res, trace[:2], first)


def test_planted_values_sit_where_the_case_says():
    assert _bits(V) & 63 == 0
    for k, (ka, kb) in NEAR.items():
        a, b = _bits(_ulps(V, ka)), _bits(_ulps(V, kb))
        same_key = (a >> 6) == (b >> 6)
        assert same_key == (k != "ulp64") and b - a == {"ulp1": 1, "ulp63": 63, "ulp64": 64, "tie": 0}[k]
        if k == "ulp64":
            assert (b >> 6) - (a >> 6) == 1
    for g, (T, cpt, _rows) in GEOM.items():
        assert (PW + 15) // 16 * 16 <= T * cpt and PW - 1 > 2 * BATCH and int(np.floor(np.sqrt(PW - 1))) <= BATCH  # partial pricing, batches of 50
        lane = lambda c: c // cpt  # noqa: E731  (lane t holds columns t * cpt ... t * cpt + cpt - 1)
        for spot in SPOTS:
            ca, cb = _pair(cpt, spot)
            assert ca < cb < PW and _batch_of(ca) == _batch_of(cb)
            if spot == "lane":
                assert lane(ca) == lane(cb)
            elif spot == "lanes":
                assert lane(ca) != lane(cb) and lane(ca) // 64 == lane(cb) // 64
            else:
                assert lane(ca) // 64 == 0 and lane(cb) // 64 == 1
    assert _ulps(PREC, 1) > PREC and _ulps(PREC, 1) == np.nextafter(np.float64(PREC), np.float64(1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("g,case", PRICING_CASES, ids=PRICING_IDS)
def test_near_tie_pricing_equals_oracle(hip_lib, oracle_lib, monkeypatch, capfd, g, case):
    _clean(monkeypatch)
    unr = case == "unr_negative"
    if unr:  # (JSLP_RES_GEOM forces lean builds without unrestricted variables: the policy picks g1, or g2 with four columns per lane)
        if g == 2:
            monkeypatch.setenv("JSLP_RES_CPT", "4")
    else:
        monkeypatch.setenv("JSLP_RES_GEOM", str(g))
    want = _pricing_oracle(oracle_lib, g, case)
    capfd.readouterr()
    got, cnt = _pricing_solve(hip_lib, g, case, False)
    lines = [x for x in LAUNCH.findall(capfd.readouterr().err) if x.startswith("k_simplex_resident<")]
    head = "k_simplex_resident<%d,%d,%d> unr %d lean 1" % (GEOM[g] + (int(unr),))
    assert len(lines) == 1 and lines[0].startswith(head), (lines, head)
    _same(got, want)
    assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), cnt


# ---- the two packed keys of profiles/barrier_diet_rejected.patch alone (CPU) ----------------------------------------------------------------------------------------------------
BATCH_MAX = 127


def key1(batch, bits):
    return ((BATCH_MAX - batch) << 57) | (bits >> 6)


def key2(bits, col):
    return ((bits & 63) << 16) | (0xFFFF - col)


def two_round_winner(cands):
    """cands: [(batch, value bits, column)] -> (batch, value bits, column) as the two atomic maxima find it"""
    w1 = max(key1(b, v) for b, v, _c in cands)
    w2 = max(key2(v, c) for b, v, c in cands if key1(b, v) == w1)
    return (BATCH_MAX - (w1 >> 57), ((w1 & ((1 << 57) - 1)) << 6) | (w2 >> 16), 0xFFFF - (w2 & 0xFFFF))


def lexicographic_winner(cands):
    return min(cands, key=lambda t: (t[0], -t[1], t[2]))


def _check(cands):
    assert all(0 <= b <= BATCH_MAX and 0 < v < (1 << 63) and 1 <= c <= 0xFFFF for b, v, c in cands)
    assert all(key1(b, v) > 0 for b, v, _c in cands)  # 0 stays "no candidate"
    assert two_round_winner(cands) == lexicographic_winner(cands), cands


def test_two_keys_pick_the_lexicographic_winner():
    rng = np.random.default_rng(SEED)
    base = _bits(V)
    inf, tiny = _bits(np.inf), _bits(_ulps(1e-15, 1))  # the largest candidate there is; the smallest (precisions below 1e-15 never reach these kernels)
    assert tiny >> 6 > 0 and inf < (1 << 63)
    # all 64 low-bit patterns against each other, in both column orders, in the first and the last batch
    for lo_a in range(64):
        for lo_b in range(64):
            for b in (0, BATCH_MAX):
                _check([(b, base + lo_a, 7), (b, base + lo_b, 9)])
                _check([(b, base + lo_a, 4095), (b, base + lo_b, 1)])
    # adjacent truncated keys, exponent boundaries (the mantissa rolls over into the exponent), the extremes
    edges = [base + 63, base + 64, base + 127, base + 128, _bits(2.0) - 1, _bits(2.0), _bits(2.0) + 1, _bits(1.0) - 1, _bits(1.0),
             _bits(np.finfo(np.float64).max), inf, tiny, tiny + 1, tiny + 63, tiny + 64, _bits(1e300)]
    for va in edges:
        for vb in edges:
            _check([(3, va, 10), (3, vb, 11)])
            _check([(3, va, 11), (3, vb, 10)])
            _check([(0, va, 60), (1, vb, 61)])        # an earlier batch wins whatever the values
            _check([(BATCH_MAX, va, 60), (BATCH_MAX - 1, vb, 2)])
    _check([(0, tiny, 50), (1, _bits(1e300), 51), (1, inf, 52)])
    # random sets: clustered values (shared truncated keys, exact ties) and free ones
    for _ in range(3000):
        n = int(rng.integers(1, 12))
        cols = rng.choice(np.arange(1, 4096), n, replace=False)
        cands = []
        for c in cols:
            b = int(rng.choice([0, 1, 2, 126, BATCH_MAX]))
            if rng.random() < 0.7:
                v = base + int(rng.integers(0, 130))
            else:
                v = _bits(abs(rng.standard_normal()) * 10.0 ** int(rng.integers(-14, 300)) + 1e-15)
            cands.append((b, v, int(c)))
        _check(cands)
