"""The lean register-resident pivot loop where its chain is trimmed or was tried to be (jslp_resident_pipe.hip.h: ONE fold per ratio-test
verdict -- a degenerate row carries key 0 -- in the ratio-test wave and in the gather's close; the row normalisation's divisions and the
ratio test's LDS operands, profiles/chain_diet.md) -- small LPs through the FORCED resident path, each against the CPU oracle's solve of
the same LP: same pivot trace, every array of the final tableau equal bit for bit, same result.

Shapes: the smallest where that code can go wrong.  `JSLP_RES_GEOM` picks the instance -- one of each column count per lane (2, 4, 6, 8)
and of each row count per workgroup (8, 12, 16): the fourth DPP step of the folds and step N's divisions are both reached --,
`JSLP_RES_RPB` = ROWS packs the rows: H = ROWS is ONE workgroup with every lane's row live, H = ROWS + 1 two workgroups, the last one
a single row, H = 2 ROWS two full ones.  Widths: one column past a wave's last lane (64 CPT + 1: ld = W + 15, the padding is live
lanes without columns) and W = ld (64 CPT + 16).

Crafted first decisions (planted in a dense all-"<=" integer LP; the entering column is the one column that prices in first):
two degenerate rows in one workgroup and in two; a degenerate row against a smaller quotient elsewhere; equal quotients in the first and
the last lane and across workgroups; no candidate at all (unbounded); a pivot whose quotient sends normalised entries under the 1e-16
gate; the entering column entering again right after it left (a negative pivot element); a pivot row with an entry so large against
its small pivot element that v_div_scale scales the operands (exponents 768 apart: where a normalisation that shares one reciprocal
among a lane's entries has to fall back to plain division).
The CPU part proves on the oracle alone that every instance makes the decision it was planted for; the oracle alone says what is
expected, the library under test never does."""
import hashlib
import os
import re

import numpy as np
import pytest

from jslpsolver_amd.engine import Tableau

SEED = 424242
PREC = 1e-8
GEOM = {1: (1024, 2, 8), 2: (512, 4, 8), 3: (512, 4, 16), 4: (512, 6, 12), 5: (512, 8, 8)}  # JSLP_RES_GEOM -> (lanes, columns per lane, rows)
KNOBS = ("JSLP_FORCE_PATH", "JSLP_RES_CPT", "JSLP_RES_LEAN", "JSLP_RES_GEOM", "JSLP_RES_RPB", "JSLP_RES_WIDE_TALL", "JSLP_XL",
         "JSLP_NO_WGLDS", "JSLP_INJECT_RESIDENT_ABORT_US", "JSLP_FUSED_P1")
LAUNCH = re.compile(r"^\[jslp\] launch (.*)$", re.M)
CE = 7     # the entering column of the crafted cases: first pricing batch, by far the largest cost
BIG = 40   # the column of the large entry ("fallback"): never prices in
KINDS = ("plain", "phase1", "two_deg_one_wg", "two_deg_two_wg", "deg_vs_smaller_quotient", "smaller_quotient_vs_deg", "tie_first_last_lane",
         "tie_across_wgs", "unbounded", "tiny_normalised", "reenter", "fallback")


def _widths(cpt):
    return (64 * cpt + 1, 64 * cpt + 16)


def _heights(rows):
    return (rows, rows + 1, 2 * rows)


def instance(kind, H, W, rows):
    """-> (A, vibr, vibc, what the oracle must show: ("pivot", row or None, col) / ("unbounded",) / ("reenter", row, col) / None)"""
    rng = np.random.default_rng(SEED + 1000 * H + W)
    m, n = H - 1, W - 1
    A = np.zeros((H, W))
    A[1:, 1:] = rng.integers(1, 21, (m, n))
    A[0, 1:] = rng.integers(1, 51, n)
    A[1:, 0] = rng.integers(100, 501, m)
    vibr = np.array([-1] + list(range(n, n + m)), dtype=np.int32)
    vibc = np.array([-1] + list(range(n)), dtype=np.int32)
    want = None
    if kind == "phase1":  # two ">=" rows (negative RHS, one variable each): the phase-1 pipeline's normalisation runs first
        A[1:, 0] = rng.integers(60000, 100001, m)
        for r, c in ((2, 3), (H - 1, 5)):
            A[r, 1:] = 0.0
            A[r, c] = -1.0
            A[r, 0] = -float(rng.integers(5, 21))
    if kind not in ("plain", "phase1"):
        A[0, CE] = 1000.0
        A[1:, CE] = 1.0  # every row's quotient is its RHS: 100 ... 500
    last0 = rows - 1        # the last lane of workgroup 0
    first1 = rows           # the first lane of workgroup 1 (H > ROWS)
    if kind == "two_deg_one_wg":
        for r in (2, min(5, H - 1)):
            A[r, 0] = 0.0
        want = ("pivot", 2, CE)
    elif kind == "two_deg_two_wg":  # workgroup 0's last lane and the last row (workgroup 1's first or last lane)
        A[last0, 0] = A[H - 1, 0] = 0.0
        want = ("pivot", last0, CE)
    elif kind == "deg_vs_smaller_quotient":  # the smallest quotient sits in the first row, the degenerate row in the last: it wins
        A[1, 0] = 1e-3
        A[H - 1, 0] = 0.0
        want = ("pivot", H - 1, CE)
    elif kind == "smaller_quotient_vs_deg":  # ... and the other way round
        A[3, 0] = 0.0
        A[H - 1, 0] = 1e-3
        want = ("pivot", 3, CE)
    elif kind == "tie_first_last_lane":  # quotient 3 in the last workgroup's first and last lane (H = ROWS: lane 0 is the cost row -- rows 1 and ROWS - 1)
        lo = first1 if H == 2 * rows else 1
        for r in (lo, H - 1):
            A[r, 0], A[r, CE] = 6.0, 2.0
        want = ("pivot", lo, CE)
    elif kind == "tie_across_wgs":  # quotient 3 in workgroup 0's last lane, workgroup 1's first lane and the last row
        for r in {last0, first1, H - 1}:
            A[r, 0], A[r, CE] = 6.0, 2.0
        want = ("pivot", last0, CE)
    elif kind == "unbounded":
        A[1:, CE] = -1.0
        A[2, CE] = 0.0
        want = ("unbounded",)
    elif kind == "tiny_normalised":  # pivot element 1e7: the row's entries of 1e-10 become 1e-17 -- under the gate, stored as 0 --, 2e-9 stays (2e-16)
        A[3, CE], A[3, 0] = 1e7, 100.0
        A[3, 20:30] = 1e-10
        A[3, 30:34] = 2e-9
        want = ("pivot", 3, CE)
    elif kind == "reenter":  # a NEGATIVE pivot element (RHS inside (-precision, 0)): the column's new cost is -1000 / -0.5, the largest again
        A[4, :] = 0.0
        A[4, 0], A[4, CE] = -9e-9, -0.5
        want = ("reenter", 4, CE)
    elif kind == "fallback":  # 1e225 / 2e-8: exponents 773 apart -- v_div_scale scales this numerator's divisor differently from 1.0's
        A[2, CE], A[2, 0] = 2e-8, 1e-6  # quotient 50: the smallest
        A[2, BIG] = 1e225
        A[H - 1, CE], A[H - 1, 0] = 3e-8, 1e-5  # a losing candidate of the last workgroup: published normalised too (NPUB builds)
        A[H - 1, BIG] = 1e225
        A[0, BIG] = -1.0
        want = ("pivot", 2, CE)
    return A, vibr, vibc, want


def _answer(t, res):
    d = res.as_dict()
    return (d, t.pivot_trace().tolist(), [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in t.download()], repr(t.evaluation))


_ORACLE = {}


def _oracle(lib, kind, H, W, rows):
    key = (kind, H, W, rows)
    if key not in _ORACLE:
        A, vibr, vibc, _want = instance(kind, H, W, rows)
        t = Tableau(A, vibr, vibc, [], precision=PREC, lib=lib)
        try:
            res = t.simplex(check_cycles=True)
            final = t.download()[0]
            _ORACLE[key] = (_answer(t, res), bool(np.isfinite(final).all()), float(np.abs(final).max()))
        finally:
            t.close()
    return _ORACLE[key]


def _cases():
    out = []
    for g in (1, 2, 3, 4, 5):
        _T, cpt, rows = GEOM[g]
        for kind in KINDS:
            if kind in ("plain", "phase1"):
                heights = _heights(rows)
            elif kind in ("two_deg_two_wg", "tie_across_wgs"):  # (they need a second workgroup)
                heights = (rows + 1, 2 * rows)
            elif kind == "tie_first_last_lane":  # (a one-row workgroup has no last lane of its own)
                heights = (rows, 2 * rows)
            else:  # (two FULL workgroups add nothing to the cases that plant single rows)
                heights = (rows, rows + 1)
            for H in heights:
                for W in (_widths(cpt) if kind == "plain" else _widths(cpt)[:1]):
                    out.append((g, kind, H, W))
    return out


CASES = _cases()
IDS = ["g%d-%s-%dx%d" % c for c in CASES]


@pytest.mark.parametrize("g,kind,H,W", CASES, ids=IDS)
def test_oracle_makes_the_planted_decision(oracle_lib, g, kind, H, W):
    rows = GEOM[g][2]
    want = instance(kind, H, W, rows)[3]
    (res, trace, _arrays, _ev), finite, biggest = _oracle(oracle_lib, kind, H, W, rows)
    assert finite and res["cycle_phase"] == 0, (res, biggest)
    if kind == "phase1":
        assert res["pivots_phase1"] >= 2 and res["feasible"], res
    elif kind == "plain":
        assert res["pivots_phase1"] == 0 and res["pivots_phase2"] >= 3 and res["optimal"], res
    elif want[0] == "unbounded":
        assert trace == [] and not res["bounded"] and res["feasible"], (res, trace[:2])
    else:
        assert res["pivots_phase1"] == 0 and tuple(trace[0]) == (want[1], want[2]), (trace[:3], want)
        if want[0] == "reenter":
            assert trace[1][1] == want[2], trace[:3]
        if kind == "fallback":
            assert biggest > 1e225


def test_planted_values_are_what_they_say():
    """the fallback case's operands are >= 768 binary exponents apart and the pivot element is no smaller than the precision; the tiny
    case's quotients straddle the 1e-16 gate"""
    assert np.frexp(1e225)[1] - np.frexp(2e-8)[1] >= 768 and 2e-8 >= PREC and np.isfinite(np.float64(1e225) / np.float64(2e-8))
    assert abs(np.float64(1e-10) / np.float64(1e7)) < 1e-16 < abs(np.float64(2e-9) / np.float64(1e7))
    assert -PREC < -9e-9 < 0 and np.float64(-9e-9) / np.float64(-0.5) > PREC
    for g, (_T, cpt, rows) in GEOM.items():
        for W in _widths(cpt):
            assert W > 64 * cpt and (W + 15) // 16 * 16 <= _T * cpt and BIG < W and W - 1 > 100  # (partial pricing: batches of 50 columns, CE in the first)
    assert {GEOM[g][1] for g in GEOM} == {2, 4, 6, 8} and {GEOM[g][2] for g in GEOM} == {8, 12, 16}


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
    A, vibr, vibc, _w = instance(kind, H, W, rows)
    chk = kind in ("plain", "phase1")  # (the CHK builds sit at their register limit: the plain solves run them, the crafted ones the check-off builds)
    capfd.readouterr()
    t = Tableau(A, vibr, vibc, [], precision=PREC, lib=hip_lib)
    try:
        got = _answer(t, t.simplex(check_cycles=chk))
        cnt = t.get_counters()
    finally:
        t.close()
    lines = [x for x in LAUNCH.findall(capfd.readouterr().err) if x.startswith("k_simplex_resident<")]
    reached_phase2 = want[0]["pivots_phase2"] >= 0
    if g <= 2 or reached_phase2:
        G = (H + rows - 1) // rows
        head = "k_simplex_resident<%d,%d,%d> unr 0 lean 1 opt 0 chk %d xl 0 G %d rpb %d" % (T, cpt, rows, int(chk), G, rows)
        assert len(lines) == 1 and lines[0].startswith(head), (lines, head)
        assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), cnt
    assert got[1][:2] == want[1][:2], (got[1][:3], want[1][:3])  # the planted decision first
    assert got[1] == want[1]
    for k in want[0]:
        x, y = got[0][k], want[0][k]
        assert x == y or (isinstance(x, float) and np.isnan(x) and np.isnan(y)), (k, x, y)
    assert got[2] == want[2]
    assert got[3] == want[3]
