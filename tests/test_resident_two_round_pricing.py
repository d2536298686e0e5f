"""The lean register-resident phase-2 loop of <1024,2,8> (jslp_resident_pipe.hip.h) prices the cost row in TWO LDS-atomic rounds on packed keys
(profiles/pricing_two_rounds.md; <512,4,8> was measured with them too and keeps three rounds -- the cases run at both widths: they pin the order, whatever
form the reduction takes):

  round 1   {127 - batch : 7 | value bits >> 6 : 57}         one 64-bit maximum over the candidate lanes' offers
  round 2   {value bits & 63 : 6 | 65535 - column : 16}      one 32-bit maximum among the lanes whose first key IS round 1's result

and must name the column the three rounds named: earliest batch, largest value in it, first column on ties.  The same change set measured the
winner's workgroup `row / rows-per-workgroup` as a multiply-shift (item B); its cases stay whether or not the form is in the tree.

Every GPU case runs a small LP through the FORCED resident path and is compared with the CPU oracle's solve of the same LP byte for byte -- the
pivot trace, the int64 views of every array of the final tableau, the result -- and asserts the launch line.  The oracle alone says what is expected.

Shapes.  17 x 300 at 8 rows per workgroup (JSLP_RES_RPB = 8: three workgroups) unless the case says otherwise; two columns per lane (a wave holds
128 columns: three waves hold candidates) and four (JSLP_RES_CPT = 4: two waves).  Phase 2 prices partially in batches of 50 columns: batches 0 .. 5, the
last one a column short.  The cost row is planted so that the FIRST pivot is decided by the case; every later pivot is checked through the trace too.
`V` = 40.0, whose low six mantissa bits are zero.

  split at bit 6   two candidates of one batch 1 / 63 / 64 / 65 ulp apart (and 1 ulp apart ACROSS the split: low bits 63 against 0) -- in one lane, in two
                   lanes of one wave, in two waves; the larger value in the later and in the earlier column.  63 ulp apart the two share the first key and
                   round 2's low bits decide, against the column order when the larger sits later; 64 apart the first keys are neighbours and the low bits
                   are equal; 65 apart the low bits (63 against 0) are OPPOSED to the value order
  low6_many        five lanes in two waves share the top 57 bits; the largest low bits occur twice, in the two LAST of the five columns
  ties             2 lanes across the wave edge; a whole batch of 50 columns (26 lanes at two columns per lane, in two waves): the first column wins
  batch order      a larger value in a later batch loses: the two inside one lane (columns 100 | 101: a batch edge between a lane's columns), inside
                   one wave, with the later batch's candidates on both sides of a wave edge (columns 127 / 128 / 129 at two columns per lane); the
                   highest batch id alone, and losing to the one before it
  corners          the only candidate in column 1; in the last column; both
  none             no candidate: optimal at once
  unrestricted     (the UNR build) a negative reduced cost whose magnitude is 1 ulp above / below / equal to a positive candidate's
  B                17 x 129 at H = 8, 16, 24 (one, two, three workgroups): the first pivot's winner in the first and the last row of each workgroup
                   (H = 8 is the only height with ONE workgroup of this geometry)
On the test build of the library the late waves and workgroups of JSLP_TEST_RESIDENT_LATE_WAVE0 = 2, 3 stretch every barrier of the two rounds: the
double-buffered words are reset one pivot ahead, a barrier away from every use.

Not here: the gather's fold under its own looks (item C of the same issue) was not built; the 64-lane tie lives in phase 1, whose loop is unchanged.

CPU: the planted columns sit where the cases say; the oracle enters them first; tools/pricing_lanes.py, whose replay restates the two keys, names the
oracle's entering column at every pivot and ends on the oracle's tableau bit for bit at n = 100 and 200."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from jslpsolver_amd.engine import Tableau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 575757
PREC = 1e-8
GEOM = {2: (1024, 2, 8), 4: (512, 4, 8)}  # JSLP_RES_CPT -> (lanes, columns per lane, rows)
KNOBS = ("JSLP_TEST_ITERS_CAP", "JSLP_FORCE_PATH", "JSLP_RES_CPT", "JSLP_RES_LEAN", "JSLP_RES_GEOM", "JSLP_RES_RPB", "JSLP_RES_WIDE_TALL", "JSLP_XL",
         "JSLP_NO_WGLDS", "JSLP_INJECT_RESIDENT_ABORT_US", "JSLP_FUSED_P1", "JSLP_TEST_RESIDENT_ABORT", "JSLP_TEST_RESIDENT_LATE_WAVE0", "JSLP_SPIN_LIMIT")
LAUNCH = re.compile(r"^\[jslp\] launch (.*)$", re.M)
BATCH = 50
RPB = 8
V = 40.0
PH, PW = 17, 300
TOP_BATCH = 5


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


def _clean(monkeypatch, cpt):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_FORCE_PATH", "resident")
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    monkeypatch.setenv("JSLP_RES_RPB", str(RPB))
    if cpt == 4:
        monkeypatch.setenv("JSLP_RES_CPT", "4")


def _solve(lib, inst, chk):
    A, vibr, vibc, unr = inst
    t = Tableau(A, vibr, vibc, unr, precision=PREC, lib=lib)
    try:
        return _answer(t, t.simplex(check_cycles=chk)), (t.get_counters() if hasattr(lib, "backend") else None)
    finally:
        t.close()


_ORACLE = {}


def _oracle(lib, key, make):
    if key not in _ORACLE:
        _ORACLE[key] = _solve(lib, make(), True)[0]
    return _ORACLE[key]


def _forced(lib, capfd, inst, cpt, H):
    capfd.readouterr()
    got, cnt = _solve(lib, inst, False)
    lines = [x for x in LAUNCH.findall(capfd.readouterr().err) if x.startswith("k_simplex_resident<")]
    head = "k_simplex_resident<%d,%d,%d> unr %d lean 1 opt 0 chk 0 xl 0 G %d rpb %d" % (GEOM[cpt] + (int(bool(inst[3])), (H + RPB - 1) // RPB, RPB))
    assert len(lines) == 1 and lines[0].startswith(head), (lines, head)
    assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), cnt
    return got


def _maps(H, W):
    m, n = H - 1, W - 1
    return np.array([-1] + list(range(n, n + m)), dtype=np.int32), np.array([-1] + list(range(n)), dtype=np.int32)


def _batch_of(col):
    return (col - 1) // BATCH


# ---- A: the two rounds ---------------------------------------------------------------------------------------------------------------------
SPOTS = ("lane", "lanes", "waves")
# ulps above V of the SMALLER and the LARGER value
NEAR = {"ulp1": (0, 1), "ulp63": (0, 63), "ulp64": (63, 127), "ulp65": (63, 128), "ulp1x": (63, 64)}
ORDERS = ("later", "earlier")  # where the larger value sits


def _pair(cpt, spot):
    """two columns of one pricing batch (the one across the waves' edge): in one lane (the last of wave 0) / in two lanes of wave 1 / in the last lane
    of wave 0 and the second lane of wave 1"""
    edge = 64 * cpt  # the first column of wave 1
    if spot == "lane":
        return edge - cpt, edge - cpt + 1
    if spot == "lanes":
        return edge + cpt, edge + 3 * cpt
    return edge - 1, edge + cpt


def _blank(cpt, H=PH, W=PW):
    rng = np.random.default_rng(SEED + 13 * cpt + H)
    A = np.zeros((H, W))
    A[1:, 1:] = rng.integers(1, 21, (H - 1, W - 1))
    A[1:, 0] = rng.integers(100, 501, H - 1)
    cost = -rng.integers(1, 20, W).astype(np.float64)  # nothing prices in unless the case says so
    cost[0] = 0.0
    return rng, A, cost


def pricing_instance(case, cpt):
    """-> (A, vibr, vibc, unrestricted variables), the first entering column (None: no pivot at all)"""
    rng, A, cost = _blank(cpt)
    edge = 64 * cpt
    unr = []
    name, _, where = case.partition("@")

    def later_batches_lose(col):  # larger values in every later batch
        later = np.arange(BATCH * (_batch_of(col) + 1) + 1, PW)
        cost[later] = rng.integers(50, 1000, len(later))

    if name in NEAR:
        spot, order = where.split("-")
        ca, cb = _pair(cpt, spot)
        lo, hi = (_ulps(V, k) for k in NEAR[name])
        cost[ca], cost[cb] = (lo, hi) if order == "later" else (hi, lo)
        later_batches_lose(cb)
        first = cb if order == "later" else ca
    elif name == "low6_many":
        cols = [edge - cpt - 1, edge - 1, edge + cpt, edge + 2 * cpt, edge + 3 * cpt]
        for col, k in zip(cols, (3, 17, 59, 60, 60)):
            cost[col] = _ulps(V, k)
        later_batches_lose(cols[-1])
        first = cols[3]
    elif name == "tie2":
        cost[edge - 1] = cost[edge] = V
        later_batches_lose(edge)
        first = edge - 1
    elif name == "tie_batch":  # batch 2: columns 101 .. 150 -- 26 lanes at two columns per lane, lanes 50 .. 75: both sides of lane 63 | 64
        cost[2 * BATCH + 1:3 * BATCH + 1] = V
        later_batches_lose(3 * BATCH)
        first = 2 * BATCH + 1
    elif name == "batch_in_lane":  # columns 100 | 101: batch 1 | batch 2, one lane at either width
        cost[2 * BATCH], cost[2 * BATCH + 1] = V, 1e6
        later_batches_lose(2 * BATCH + 1)
        first = 2 * BATCH
    elif name == "batch_in_wave":
        cost[BATCH + 10], cost[2 * BATCH + 10] = _ulps(PREC, 1), np.inf
        first = BATCH + 10
    elif name == "batch_wave_edge":  # the earlier batch's candidate in wave 0; the later batch's on both sides of the waves' edge
        b = _batch_of(edge - 1)
        cost[BATCH * b] = V
        cost[edge - 1], cost[edge], cost[edge + 1] = 1e3, 1e300, 1e6
        first = BATCH * b
    elif name == "top_batch_only":
        cost[BATCH * TOP_BATCH + 10], cost[PW - 1] = V, _ulps(V, 1)
        first = PW - 1
    elif name == "top_batch_loses":
        cost[BATCH * TOP_BATCH] = V
        cost[BATCH * TOP_BATCH + 1:] = 1e9
        first = BATCH * TOP_BATCH
    elif name == "corner_first":
        cost[1] = V
        first = 1
    elif name == "corner_last":
        cost[PW - 1] = V
        first = PW - 1
    elif name == "corner_both":
        cost[1], cost[PW - 1] = V, 1e12
        first = 1
    elif name == "none":
        first = None
    elif name.startswith("unr_"):
        unr = [0, 1, 2]  # variables 0..2 = columns 1..3
        A[2:PH - 1, 1:4] *= np.where(rng.random((PH - 3, 3)) < 0.5, -1.0, 1.0)  # bounded both ways
        neg, pos = {"unr_neg_wins": (_ulps(V, 1), V), "unr_pos_wins": (V, _ulps(V, 1)), "unr_tie": (V, V)}[name]
        cost[1:4] = [5.0, -neg, 9.0]
        cost[40] = pos
        first = 40 if name == "unr_pos_wins" else 2
    else:
        raise ValueError(case)
    A[0, :] = cost
    return (A,) + _maps(PH, PW) + (unr,), first


P_NAMES = ["%s@%s-%s" % (k, s, o) for k in NEAR for s in SPOTS for o in ORDERS] + \
          ["low6_many", "tie2", "tie_batch", "batch_in_lane", "batch_in_wave", "batch_wave_edge", "top_batch_only", "top_batch_loses",
           "corner_first", "corner_last", "corner_both", "none", "unr_neg_wins", "unr_pos_wins", "unr_tie"]
P_CASES = [(cpt, case) for cpt in GEOM for case in P_NAMES]
P_IDS = ["cpt%d-%s" % c for c in P_CASES]
LATE_NAMES = ["ulp63@waves-later", "ulp65@waves-earlier", "low6_many", "tie_batch", "batch_wave_edge", "top_batch_only", "unr_neg_wins"]
LATE_CASES = [(cpt, case, late) for cpt in GEOM for case in LATE_NAMES for late in (2, 3)]
LATE_IDS = ["cpt%d-%s-late%d" % c for c in LATE_CASES]


def test_planted_values_and_columns_sit_where_the_cases_say():
    assert _bits(V) & 63 == 0
    want = {"ulp1": (1, True), "ulp63": (63, True), "ulp64": (64, False), "ulp65": (65, False), "ulp1x": (1, False)}
    for k, (ka, kb) in NEAR.items():
        a, b = _bits(_ulps(V, ka)), _bits(_ulps(V, kb))
        assert (b - a, (a >> 6) == (b >> 6)) == want[k]
    a, b = (_bits(_ulps(V, k)) for k in NEAR["ulp65"])
    assert (b >> 6) > (a >> 6) and (b & 63) < (a & 63)  # the low bits opposed to the value order
    a, b = (_bits(_ulps(V, k)) for k in NEAR["ulp64"])
    assert (b >> 6) - (a >> 6) == 1 and (b & 63) == (a & 63)
    assert 129 <= PW <= 300 and 9 <= PH <= 24 and (PH + RPB - 1) // RPB == 3
    assert PW - 1 > 2 * BATCH and int(np.floor(np.sqrt(PW - 1))) <= BATCH and _batch_of(PW - 1) == TOP_BATCH  # partial pricing, batches of 50
    assert _ulps(PREC, 1) > PREC
    for cpt, (T, _c, _rows) in GEOM.items():
        lane = lambda c: c // cpt  # noqa: E731  (lane t holds columns t * cpt ... t * cpt + cpt - 1)
        edge = 64 * cpt
        assert (PW + 15) // 16 * 16 <= T * cpt and lane(PW - 1) // 64 >= 1 and (cpt != 2 or lane(PW - 1) // 64 == 2)
        for spot in SPOTS:
            ca, cb = _pair(cpt, spot)
            assert ca < cb < PW and _batch_of(ca) == _batch_of(cb)
            if spot == "lane":
                assert lane(ca) == lane(cb)
            elif spot == "lanes":
                assert lane(ca) != lane(cb) and lane(ca) // 64 == lane(cb) // 64
            else:
                assert lane(ca) // 64 == 0 and lane(cb) // 64 == 1
        assert lane(2 * BATCH) == lane(2 * BATCH + 1) and _batch_of(2 * BATCH) + 1 == _batch_of(2 * BATCH + 1)  # a batch edge inside a lane
        assert lane(BATCH + 10) // 64 == lane(2 * BATCH + 10) // 64 and _batch_of(BATCH + 10) < _batch_of(2 * BATCH + 10)
        b = _batch_of(edge - 1)
        assert _batch_of(edge + 1) == b and _batch_of(BATCH * b) == b - 1 and lane(BATCH * b) // 64 == 0 and lane(edge - 1) // 64 == 0 and lane(edge) // 64 == 1
        (A, _r, _c2, _u), _f = pricing_instance("low6_many", cpt)
        cols = np.nonzero((A[0] >= V) & (A[0] <= _ulps(V, 63)))[0]
        assert len(cols) == 5 and len({_bits(A[0, c]) >> 6 for c in cols}) == 1 and len({lane(c) for c in cols}) == 5 and len({_batch_of(c) for c in cols}) == 1 and len({lane(c) // 64 for c in cols}) == 2
        (A, _r, _c2, _u), _f = pricing_instance("tie_batch", cpt)
        lanes = {lane(c) for c in np.nonzero(A[0] == V)[0]}
        assert len(lanes) == (26 if cpt == 2 else 13) and (cpt != 2 or {x // 64 for x in lanes} == {0, 1})
    assert (64 * 2 - 1, 64 * 2, 64 * 2 + 1) == (127, 128, 129)


@pytest.mark.parametrize("cpt,case", P_CASES, ids=P_IDS)
def test_oracle_enters_the_planted_column_first(oracle_lib, cpt, case):
    inst, first = pricing_instance(case, cpt)
    res, trace = _oracle(oracle_lib, ("A", cpt, case), lambda: inst)[:2]
    assert res["cycle_phase"] == 0 and res["pivots_phase1"] == 0, res
    if first is None:
        assert trace == [] and res["optimal"], (res, trace[:2])
    else:
        assert trace[0][1] == first, (res, trace[:2], first)


@pytest.mark.gpu
@pytest.mark.parametrize("cpt,case", P_CASES, ids=P_IDS)
def test_two_round_pricing_equals_oracle(hip_lib, oracle_lib, monkeypatch, capfd, cpt, case):
    _clean(monkeypatch, cpt)
    inst, _first = pricing_instance(case, cpt)
    want = _oracle(oracle_lib, ("A", cpt, case), lambda: inst)
    _same(_forced(hip_lib, capfd, inst, cpt, PH), want)


@pytest.mark.gpu
@pytest.mark.parametrize("cpt,case,late", LATE_CASES, ids=LATE_IDS)
def test_two_round_pricing_with_late_waves_equals_oracle(hip_hooks_lib, oracle_lib, monkeypatch, capfd, cpt, case, late):
    _clean(monkeypatch, cpt)
    monkeypatch.setenv("JSLP_TEST_RESIDENT_LATE_WAVE0", str(late))
    inst, _first = pricing_instance(case, cpt)
    want = _oracle(oracle_lib, ("A", cpt, case), lambda: inst)
    _same(_forced(hip_hooks_lib, capfd, inst, cpt, PH), want)


# ---- B: the winner's workgroup ---------------------------------------------------------------------------------------------------------------
BW = 129
CE = 7  # the entering column of the crafted first pivot: first pricing batch, the largest cost
B_CASES = [(cpt, H, g, where) for cpt in GEOM for H in (8, 16, 24) for g in range(H // RPB) for where in ("first", "last")]
B_IDS = ["cpt%d-H%d-wg%d-%s" % c for c in B_CASES]


def winner_instance(cpt, H, g, where):
    _rng, A, cost = _blank(cpt, H, BW)
    cost[1:] = np.abs(cost[1:])
    cost[CE] = 100.0
    A[1:, CE] = 20.0
    row = max(1, RPB * g) if where == "first" else RPB * g + RPB - 1  # (workgroup 0's row 0 is the cost row)
    A[row, 0] = 1e-3  # the smallest quotient by far
    A[0, :] = cost
    return (A,) + _maps(H, BW) + ([],), (row, CE)


@pytest.mark.parametrize("cpt,H,g,where", B_CASES, ids=B_IDS)
def test_oracle_picks_the_planted_row(oracle_lib, cpt, H, g, where):
    inst, want = winner_instance(cpt, H, g, where)
    res, trace = _oracle(oracle_lib, ("B", cpt, H, g, where), lambda: inst)[:2]
    assert res["pivots_phase1"] == 0 and res["cycle_phase"] == 0 and tuple(trace[0]) == want and len(trace) >= 2, (res, trace[:3])
    assert want[0] // RPB == g and want[0] < H and (where == "first" or want[0] % RPB == RPB - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("cpt,H,g,where", B_CASES, ids=B_IDS)
def test_winner_found_in_the_planted_workgroup(hip_lib, oracle_lib, monkeypatch, capfd, cpt, H, g, where):
    _clean(monkeypatch, cpt)
    inst, _want = winner_instance(cpt, H, g, where)
    want = _oracle(oracle_lib, ("B", cpt, H, g, where), lambda: inst)
    _same(_forced(hip_lib, capfd, inst, cpt, H), want)


# ---- tools/pricing_lanes.py: the replay that restates the two keys ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (100, 200))
def test_pricing_lanes_replay_names_the_oracles_columns(oracle_lib, n):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pricing_lanes.py"), "3a", str(n)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [x for x in out.stdout.splitlines() if x.startswith("| 3a n = %d " % n)]
    assert len(rows) == 2, out.stdout
    three, two = ([c.strip() for c in r.strip("|").split("|")] for r in rows)
    assert three[-2:] == ["every pivot", "bit for bit"] and two[-1] == "every pivot", rows
    # every candidate lane / the waves' earliest batches / round 2: "mean / p99 / max" per workgroup and in the busiest wave
    every, every_w, early, early_w, second, second_w = ([float(x) for x in c.split("/")] for c in two[2:8])
    for a in (every, every_w, early, early_w, second, second_w):
        assert 1.0 <= a[0] <= a[2] and a[1] <= a[2]
    assert early[0] <= every[0] and early[2] <= every[2] and second[0] <= early[0] and every_w[2] <= 64
    assert every_w[0] <= every[0] and early_w[0] <= early[0]
