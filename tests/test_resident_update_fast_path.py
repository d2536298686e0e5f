"""The pending pivot's row update of the lean register-resident loops (JSLP_XL_UPDATE_PASS, jslp_resident_pipe.hip.h): ONE uniform test per
pass -- is every row's gate `|k| > 1e-16` open, or the row padding? -- in front of a gate-free arm; a closed gate anywhere sends the
workgroup through the gated arm (profiles/update_fast_path.md).  Small LPs through the FORCED resident path, each against the CPU oracle's
solve of the same LP: same pivot trace, every array of the final tableau equal bit for bit (the int64 views: a +0 / -0 flip fails), same
result.  The oracle alone says what is expected.

Shapes.  `JSLP_RES_GEOM` picks the instance: <1024,2,8> and <512,4,8> (the geometries that got the gate-free arm) and <512,4,16> once (code that
must not change); `JSLP_RES_RPB` = ROWS packs the rows.  Heights for 8 rows per workgroup: 8 (one full workgroup), 9 / 12 / 15 (the last
workgroup has 1 / 4 / 7 live rows: its padding rows go through the gate-free arm), 16 (two full ones).  Widths: one column past a wave's last
lane (64 CPT + 1) and W = ld (64 CPT + 16).

Cases (all "<=" rows but "phase1"; C1 = column 7 prices in first, C2 = column 9 second, C3 = column 11 third where the case plants them):
  dense            random integers: every gate open at every pivot of phase 2
  phase1_dense / phase1   two ">=" rows in front of it, every variable in them (the phase-1 loop's gate-free pass and its epilogue's) / one
                   variable each (zeros in the other row's column: the phase-1 loop's gated pass)
  closed@r         C2's entry of row r becomes exactly +0 under pivot 1 (0.5 - 1 * 0.5): pivot 1 gate-free, pivot 2 gated in r's workgroup, pivot 3
                   gate-free again; r = the workgroup's lane 0, lane 7, a middle lane -- first and last workgroup
  closed_first@r   C1's entry of row r is 0: the FIRST pass is the gated one
  edge_closed / edge_closed_neg / edge_open    C1's entry of a row is 1e-16 / -1e-16 (the test is `>`: closed) / the next double above 1e-16 (open)
  zeros            the pivot row has entries +0 and -0 (their column gates are closed in those lanes only: single columns of a lane, whole lanes, a
                   whole wave's columns) while every row gate is open; cells of -0.0 sit in those columns in rows with positive and with negative
                   multipliers (computed, -0 - (-k * 0) would come out +0), and in a row whose gate is closed under a NEGATIVE pivot-row entry
  unbounded        pivot 1, then C2 has no positive entry: the loop is left with the pivot pending (the epilogue's pass), as at every optimum
The CPU part replays the oracle's trace with the oracle's own pivot() and counts, per pivot and workgroup, the live rows whose entry of the
entering column fails the gate: every instance takes the arms it was built for.

  capped           the exit at the iteration cap -- `end_code = 4` at the TOP of the loop, in front of the pricing, with the last pivot pending: the
                   epilogue's pass brings the rows up to date.  `JSLP_TEST_ITERS_CAP=n` (a host value, read when the engine is created) lowers the cap
                   of 2 000 000 + 200 (rows + columns) pivots to n; the call fails with the cap's error and leaves the tableau as n pivots made
                   it, which is the oracle's replay of the first n entries of its own trace (the oracle has no cap).  Phase 2 (dense, n = 2: the
                   pending pass is gate-free), phase 1 (n = 1) and closed@r (n = 2: the pending pass is the gated one), padded last workgroups."""
import hashlib
import re

import numpy as np
import pytest

from jslpsolver_amd.engine import Tableau

SEED = 515151
PREC = 1e-8
GATE = 1e-16
GEOM = {1: (1024, 2, 8), 2: (512, 4, 8), 3: (512, 4, 16)}  # JSLP_RES_GEOM -> (lanes, columns per lane, rows)
KNOBS = ("JSLP_TEST_ITERS_CAP", "JSLP_FORCE_PATH", "JSLP_RES_CPT", "JSLP_RES_LEAN", "JSLP_RES_GEOM", "JSLP_RES_RPB", "JSLP_RES_WIDE_TALL", "JSLP_XL",
         "JSLP_NO_WGLDS", "JSLP_INJECT_RESIDENT_ABORT_US", "JSLP_FUSED_P1")
LAUNCH = re.compile(r"^\[jslp\] launch (.*)$", re.M)
C1, C2, C3 = 7, 9, 11   # first pricing batch (columns 1 ... 50)
NEGCOL = 13             # "zeros": the pivot row's NEGATIVE entry
ZCOLS = (2, 20, 21, 24, 25, 26, 27, 40)  # "zeros": the pivot row's zero entries (single columns of a lane and whole lanes, 2 and 4 columns per lane)
PIVROW = 2              # the crafted cases' first pivot row (the smallest right-hand side)
NEXT_UP = float(np.nextafter(np.float64(GATE), np.float64(1.0)))


def _ld(W):
    return (W + 15) // 16 * 16


def instance(kind, H, W, rows):
    rng = np.random.default_rng(SEED + 1000 * H + W)
    m, n = H - 1, W - 1
    A = np.zeros((H, W))
    A[1:, 1:] = rng.integers(1, 21, (m, n))
    A[0, 1:] = rng.integers(1, 51, n)
    A[1:, 0] = rng.integers(100, 501, m)
    vibr = np.array([-1] + list(range(n, n + m)), dtype=np.int32)
    vibc = np.array([-1] + list(range(n)), dtype=np.int32)
    name, _, at = kind.partition("@")
    r = int(at) if at else None
    if name in ("dense", "phase1_dense"):  # (sixty-fourths on top: integers alone cancel to an exact 0 now and then)
        A[1:, 1:] += rng.integers(0, 64, (m, n)) / 64.0
    if name == "dense":
        return A, vibr, vibc
    if name in ("phase1", "phase1_dense"):  # two ">=" rows (negative RHS): one variable each / every variable
        A[1:, 0] = rng.integers(60000, 100001, m)
        for rr, c in ((2, 3), (H - 1, 5)):
            if name == "phase1":
                A[rr, 1:] = 0.0
                A[rr, c] = -1.0
            else:
                A[rr, 1:] = -A[rr, 1:]
            A[rr, 0] = -float(rng.integers(5, 21))
        return A, vibr, vibc
    # the crafted cases: C1 prices in first (cost 1000, entries 1: every row's quotient is its RHS, row PIVROW's the smallest).  Pivot 1 leaves
    # cost 900 - 1000 * 0.5 = 400 on C2, ~295 on C3 (small entries) and c - 1000 * (1 ... 20) < 0 elsewhere: C2 enters second, C3 third
    A[0, C1] = 1000.0
    A[1:, C1] = 1.0
    A[PIVROW, 0] = 50.0
    A[0, C2] = 900.0
    A[1:, C2] = 1.0
    A[PIVROW, C2] = 0.5
    A[0, C3] = 300.0
    A[1:, C3] = (np.arange(1, H) + 3) ** 2 / 4096.0  # (squares: no two pivots' combinations cancel to an exact 0 in another row)
    if name == "closed":
        A[r, C2] = 0.5  # 0.5 - 1 * 0.5: exactly +0 once pivot 1 is applied
    elif name == "unbounded":
        A[1:, C2] = -1.0
        A[PIVROW, C2] = -1.0 / 1024  # cost 900 + 1000 / 1024 > 0, every entry stays negative: unbounded at the second pricing
        A[0, C3] = 0.0
    elif name == "closed_first":
        A[r, C1] = 0.0
    elif name == "edge_closed":
        A[r, C1] = GATE
    elif name == "edge_closed_neg":
        A[r, C1] = -GATE
    elif name == "edge_open":
        A[r, C1] = NEXT_UP
    elif name == "zeros":
        neg_rows = [i for i in (1, 4, H - 1) if i != PIVROW and i != r]
        A[neg_rows, C1] = -1.0  # negative multipliers (never candidates of the ratio test)
        A[r, C1] = 0.0          # ... and one closed gate
        for q, c in enumerate(ZCOLS):
            A[1:, c] = np.where(np.arange(1, H) % 2 == 0, -0.0, A[1:, c])
            A[neg_rows[0], c] = -0.0
            A[PIVROW, c] = 0.0 if q % 2 == 0 else -0.0
        lo = 64 * ((W - 1) // 64)  # every live column of the last wave: the pivot row is zero there
        A[PIVROW, lo:] = 0.0
        A[1, lo:] = -0.0
        A[PIVROW, NEGCOL] = -3.0
        A[r, NEGCOL] = -0.0      # closed gate: stays -0.0 (computed, -0 - (0 * -3) = +0)
        A[neg_rows[0], NEGCOL + 1] = -0.0
    else:
        raise ValueError(kind)
    return A, vibr, vibc


def _answer(t, res):
    return (res.as_dict(), t.pivot_trace().tolist(), _hashes(t.download()), repr(t.evaluation))


_ORACLE = {}


def _oracle(lib, kind, H, W, rows):
    """-> (answer, per pivot: {workgroup: live rows whose entry of the entering column fails the gate}, the replay ends in the solve's tableau)"""
    key = (kind, H, W, rows)
    if key not in _ORACLE:
        A, vibr, vibc = instance(kind, H, W, rows)
        t = Tableau(A, vibr, vibc, [], precision=PREC, lib=lib)
        try:
            ans = _answer(t, t.simplex(check_cycles=True))
            final = t.download()[0]
        finally:
            t.close()
        closed = []
        t = Tableau(A, vibr, vibc, [], precision=PREC, lib=lib)
        try:
            for pr, pc in ans[1]:
                col = t.download()[0][:, pc]
                shut = {}
                for i in range(H):
                    if not abs(col[i]) > GATE:
                        shut.setdefault(i // rows, []).append(i)
                closed.append(shut)
                t.pivot(pr, pc)
            replay_ok = t.download()[0].view(np.int64).tobytes() == final.view(np.int64).tobytes()
        finally:
            t.close()
        _ORACLE[key] = (ans, closed, replay_ok, bool(np.isfinite(final).all()))
    return _ORACLE[key]


def _widths(cpt):
    return (64 * cpt + 1, 64 * cpt + 16)


def _cases():
    out = []
    for g in (1, 2):
        _T, cpt, rows = GEOM[g]
        w1, w2 = _widths(cpt)
        for H in (8, 9, 12, 15, 16):
            last = H - 1
            for W in (w1, w2):
                out.append((g, "dense", H, W))
            out.append((g, "phase1", H, w1))
            out.append((g, "phase1_dense", H, w1))
            out.append((g, "unbounded", H, w1))
            first_wg = sorted({1, 4, min(7, last)} - {PIVROW})       # (lane 0 of workgroup 0 is the cost row: its gate is the reduced cost, never closed)
            last_wg = sorted({8, (8 + last) // 2, last}) if H > 8 else []
            for r in first_wg + last_wg:
                out.append((g, "closed@%d" % r, H, w1))
            for r in (first_wg[-1:] + last_wg[-1:]):
                out.append((g, "closed_first@%d" % r, H, w2))
                out.append((g, "zeros@%d" % r, H, w2))
            r = last if H > 8 else 4
            for k in ("edge_closed", "edge_closed_neg", "edge_open"):
                out.append((g, "%s@%d" % (k, r), H, w1))
    cpt = GEOM[3][1]
    out.append((3, "dense", 17, _widths(cpt)[0]))      # <512,4,16>: the parent's code (two workgroups, the last one a single row)
    out.append((3, "closed@16", 17, _widths(cpt)[0]))
    return out


CASES = _cases()
IDS = ["g%d-%s-%dx%d" % c for c in CASES]


@pytest.mark.parametrize("g,kind,H,W", CASES, ids=IDS)
def test_oracle_takes_the_arm_the_instance_was_built_for(oracle_lib, g, kind, H, W):
    rows = GEOM[g][2]
    (res, trace, _arrays, _ev), closed, replay_ok, finite = _oracle(oracle_lib, kind, H, W, rows)
    name, _, at = kind.partition("@")
    r = int(at) if at else None
    assert replay_ok and finite and res["cycle_phase"] == 0, res
    n_closed = [sum(len(v) for v in shut.values()) for shut in closed]  # per pivot: rows whose column entry fails the gate
    if name == "dense":
        assert res["pivots_phase1"] == 0 and res["pivots_phase2"] >= 3 and res["optimal"], res
        assert n_closed == [0] * len(trace), n_closed  # every pass of every workgroup is gate-free
    elif name == "phase1":  # (a ">=" row's single variable: zeros in the other ">=" row's column -- the phase-1 loop's gated arm)
        assert res["pivots_phase1"] >= 2 and res["feasible"], res
        assert any(n > 0 for n in n_closed[:res["pivots_phase1"]]), n_closed
        if H > rows:  # ... while the other workgroup's pass of the same pivot is gate-free
            assert any(len(shut) == 1 for shut in closed[:res["pivots_phase1"]]), closed
    elif name == "phase1_dense":  # the phase-1 loop's gate-free arm, and its epilogue's
        assert res["pivots_phase1"] >= 1 and res["pivots_phase2"] >= 1 and res["feasible"], res
        assert n_closed[:res["pivots_phase1"] + 1] == [0] * (res["pivots_phase1"] + 1), n_closed
    elif name == "unbounded":
        assert res["pivots_phase1"] == 0 and trace == [[PIVROW, C1]] and not res["bounded"] and res["feasible"], (res, trace)
        assert n_closed == [0]
    else:
        assert res["pivots_phase1"] == 0 and res["optimal"] and tuple(trace[0]) == (PIVROW, C1), (res, trace[:3])
        wg = r // rows
        if name == "closed":  # gate-free, gated (exactly row r), gate-free
            assert len(trace) >= 3 and trace[1][1] == C2 and trace[2][1] == C3, trace[:4]
            assert closed[0] == {} and closed[1] == {wg: [r]} and closed[2] == {}, closed[:3]
        elif name in ("closed_first", "edge_closed", "edge_closed_neg"):
            assert closed[0] == {wg: [r]}, closed[:2]
            assert len(trace) >= 2 and wg not in closed[1], (trace[:3], closed[:3])  # ... and gate-free right behind it
        elif name == "edge_open":
            assert closed[0] == {}, closed[:2]
        elif name == "zeros":
            assert closed[0] == {wg: [r]}, closed[:2]
            assert len(trace) >= 2


def test_planted_values_are_what_they_say():
    assert not abs(np.float64(GATE)) > GATE and not abs(np.float64(-GATE)) > GATE and abs(np.float64(NEXT_UP)) > GATE
    assert NEXT_UP > GATE and np.nextafter(np.float64(NEXT_UP), np.float64(0.0)) == GATE
    assert np.float64(0.5) - np.float64(1.0) * np.float64(0.5) == 0.0 and not np.signbit(np.float64(0.5) - np.float64(1.0) * np.float64(0.5))
    # what the column gate protects: computed, a cell of -0.0 would come out +0
    assert not np.signbit(np.float64(-0.0) - np.float64(-1.0) * np.float64(0.0)) and not np.signbit(np.float64(-0.0) - np.float64(0.0) * np.float64(-3.0))
    A = instance("zeros@4", 12, 144, 8)[0]
    assert np.signbit(A[PIVROW, ZCOLS[1]]) and not np.signbit(A[PIVROW, ZCOLS[0]]) and A[PIVROW, ZCOLS[1]] == 0.0
    assert np.signbit(A[4, NEGCOL]) and A[PIVROW, NEGCOL] == -3.0 and np.signbit(A[1, ZCOLS[0]])
    for g, (T, cpt, rows) in GEOM.items():
        for W in _widths(cpt):
            assert W > 64 * cpt and _ld(W) <= T * cpt and W - 1 > 100 and max(C3, NEGCOL + 1, max(ZCOLS)) <= 50  # (partial pricing: batches of 50 columns)
    assert {(c[0], c[2]) for c in CASES if c[0] != 3} == {(g, H) for g in (1, 2) for H in (8, 9, 12, 15, 16)}


@pytest.mark.gpu
@pytest.mark.parametrize("g,kind,H,W", CASES, ids=IDS)
def test_forced_resident_equals_oracle(hip_lib, oracle_lib, monkeypatch, capfd, g, kind, H, W):
    T, cpt, rows = GEOM[g]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_FORCE_PATH", "resident")
    monkeypatch.setenv("JSLP_RES_GEOM", str(g))
    monkeypatch.setenv("JSLP_RES_RPB", str(rows))
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    want = _oracle(oracle_lib, kind, H, W, rows)[0]
    A, vibr, vibc = instance(kind, H, W, rows)
    chk = kind in ("dense", "phase1", "phase1_dense")  # (both builds of each geometry: the plain solves run the cycle-check one, the crafted ones the check-off one)
    capfd.readouterr()
    t = Tableau(A, vibr, vibc, [], precision=PREC, lib=hip_lib)
    try:
        got = _answer(t, t.simplex(check_cycles=chk))
        cnt = t.get_counters()
    finally:
        t.close()
    lines = [x for x in LAUNCH.findall(capfd.readouterr().err) if x.startswith("k_simplex_resident<")]
    G = (H + rows - 1) // rows
    head = "k_simplex_resident<%d,%d,%d> unr 0 lean 1 opt 0 chk %d xl 0 G %d rpb %d" % (T, cpt, rows, int(chk), G, rows)
    assert len(lines) == 1 and lines[0].startswith(head), (lines, head)
    assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), cnt
    assert got[1] == want[1], (got[1][:4], want[1][:4])
    for k in want[0]:
        x, y = got[0][k], want[0][k]
        assert x == y or (isinstance(x, float) and np.isnan(x) and np.isnan(y)), (k, x, y)
    assert got[2] == want[2]
    assert got[3] == want[3]


# ---- the exit at the iteration cap -----------------------------------------------------------------------------------------------
def _cap_cases():
    out = []
    for g in (1, 2):
        w1 = _widths(GEOM[g][1])[0]
        for H in (9, 12, 15, 16):
            out.append((g, "dense", H, w1, 2))
            out.append((g, "phase1", H, w1, 1))
            out.append((g, "closed@%d" % (H - 1), H, w1, 2))
    return out


CAP_CASES = _cap_cases()
CAP_IDS = ["g%d-%s-%dx%d-cap%d" % c for c in CAP_CASES]
_CAPPED = {}


def _oracle_capped(lib, kind, H, W, rows, cap):
    """-> (the first `cap` entries of the oracle's trace, the hashes of what its own pivot() makes of them)"""
    key = (kind, H, W, rows, cap)
    if key not in _CAPPED:
        trace = _oracle(lib, kind, H, W, rows)[0][1]
        A, vibr, vibc = instance(kind, H, W, rows)
        t = Tableau(A, vibr, vibc, [], precision=PREC, lib=lib)
        try:
            for pr, pc in trace[:cap]:
                t.pivot(pr, pc)
            _CAPPED[key] = (trace[:cap], _hashes(t.download()))
        finally:
            t.close()
    return _CAPPED[key]


def _hashes(arrays):
    return [hashlib.sha256(np.ascontiguousarray(x).view(np.int64).tobytes() if x.dtype == np.float64 else np.ascontiguousarray(x).tobytes()).hexdigest()
            for x in arrays]


@pytest.mark.parametrize("g,kind,H,W,cap", CAP_CASES, ids=CAP_IDS)
def test_oracle_trace_is_longer_than_the_cap(oracle_lib, g, kind, H, W, cap):
    rows = GEOM[g][2]
    (res, trace, _arrays, _ev), closed, replay_ok, _finite = _oracle(oracle_lib, kind, H, W, rows)
    assert replay_ok and len(trace) > cap, (len(trace), cap)
    pending = closed[cap - 1]  # the pass the epilogue runs
    if kind == "dense":
        assert res["pivots_phase1"] == 0 and pending == {}
    elif kind == "phase1":
        assert res["pivots_phase1"] > cap  # (the cap ends phase 1's loop)
    else:
        r = int(kind.partition("@")[2])
        assert pending == {r // rows: [r]} and H - (r // rows) * rows <= rows
    assert len(_oracle_capped(oracle_lib, kind, H, W, rows, cap)[0]) == cap


@pytest.mark.gpu
@pytest.mark.parametrize("g,kind,H,W,cap", CAP_CASES, ids=CAP_IDS)
def test_exit_at_the_iteration_cap_equals_the_truncated_replay(hip_lib, oracle_lib, monkeypatch, capfd, g, kind, H, W, cap):
    from jslpsolver_amd._capi import EngineError
    T, cpt, rows = GEOM[g]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_FORCE_PATH", "resident")
    monkeypatch.setenv("JSLP_RES_GEOM", str(g))
    monkeypatch.setenv("JSLP_RES_RPB", str(rows))
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    monkeypatch.setenv("JSLP_TEST_ITERS_CAP", str(cap))
    want_trace, want_hashes = _oracle_capped(oracle_lib, kind, H, W, rows, cap)
    A, vibr, vibc = instance(kind, H, W, rows)
    capfd.readouterr()
    t = Tableau(A, vibr, vibc, [], precision=PREC, lib=hip_lib)
    try:
        with pytest.raises(EngineError, match="iteration"):
            t.simplex(check_cycles=False)
        got_trace, got_hashes, cnt = t.pivot_trace().tolist(), _hashes(t.download()), t.get_counters()
    finally:
        t.close()
    lines = [x for x in LAUNCH.findall(capfd.readouterr().err) if x.startswith("k_simplex_resident<")]
    head = "k_simplex_resident<%d,%d,%d> unr 0 lean 1 opt 0 chk 0 xl 0 G %d rpb %d" % (T, cpt, rows, (H + rows - 1) // rows, rows)
    assert len(lines) == 1 and lines[0].startswith(head), (lines, head)
    assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), cnt
    assert got_trace == want_trace, (got_trace, want_trace)
    assert got_hashes == want_hashes
