"""The lean pipelined phase 2's pricing (price_row_pipe, jslp_resident_pipe.hip.h) on tableaus whose FIRST pivot is decided by the
pricing's tie rules, on every register-resident geometry that holds them, HIP against the CPU oracle bit for bit (the whole pivot
trace, the final tableau, the result).

The pricing's key is lexicographic (simplex.ts:136-219): the earliest batch of partial pricing that holds a candidate, then the largest
value in it, then the smallest column.  A reduction over lanes and waves has to keep that order wherever the deciding columns sit,
so the cases put them where lanes, waves and batches meet:
  * equal best values in two waves (and two lanes, and one lane) of the winning batch: the smallest column wins;
  * the winning batch's only candidate next to a much larger value of the next batch, in the same lane, with larger values still in
    later waves: the earlier batch wins;
  * the only candidates in the last, short batch up to the last column (ties there too);
  * an unrestricted column whose reduced cost is negative (|rc| ties a positive one further right): it wins, with its sign;
  * no candidate at all, values at and just below the precision included: optimal at once.
CPU part: the oracle pivots each instance first on the column the case names."""
import hashlib
import os
import re
import sys

import numpy as np
import pytest

from jslpsolver_amd.engine import Tableau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resident_stress import int_instance  # noqa: E402  (the dense all-"<=" integer LP of the stress tool)

SEED = 4242
PREC = 1e-8
H, W = 257, 801  # 2 rows per workgroup on 129 workgroups; partial pricing in batches of 50 columns (simplex.ts:118-127)
BATCH = 50
# geometry (JSLP_RES_GEOM) -> (threads, columns per lane, rows per lane)
GEOM = {1: (1024, 2, 8), 2: (512, 4, 8), 3: (512, 4, 16), 4: (512, 6, 12), 5: (512, 8, 8)}
KNOBS = ("JSLP_FORCE_PATH", "JSLP_RES_CPT", "JSLP_RES_LEAN", "JSLP_RES_GEOM", "JSLP_RES_RPB", "JSLP_RES_WIDE_TALL", "JSLP_XL",
         "JSLP_NO_WGLDS", "JSLP_INJECT_RESIDENT_ABORT_US")
LAUNCH = re.compile(r"^\[jslp\] launch (k_simplex_resident<\d+,\d+,\d+> unr \d+ lean \d+)", re.M)
CASES = ("tie_across_waves", "earlier_batch_wins", "last_batch", "unrestricted_negative", "optimal")
N_UNR = 3


def _batch_of(col):
    return (col - 1) // BATCH


def planted(case, geom):
    """-> (A, unrestricted variables, the first entering column or 0)"""
    T, C, _R = GEOM[geom]
    A, _vibr, _vibc = int_instance(H - 1, W - 1, SEED)
    rng = np.random.default_rng(SEED + geom)
    cost = -rng.integers(1, 20, W).astype(np.float64)  # nothing prices in unless a case says so
    cost[0] = 0.0
    unr = []
    B = 64 * C  # the first column of wave 1
    b = _batch_of(B)  # the batch across the waves' boundary
    lo, hi = 1 + BATCH * b, BATCH * (b + 1)
    later = np.arange(hi + 1, W)
    if case == "tie_across_waves":
        cost[later] = rng.integers(1, 100, len(later))  # larger values in later batches lose
        cost[B - 1] = 12.0
        cost[[B - 3, B + 1, B + 2 * C, B + 2 * C + 1]] = 40.0  # wave 0, wave 1's first lane, then both first columns of its third lane
        cost[B + 2 * C + 2] = 39.999999
        first = B - 3
    elif case == "earlier_batch_wins":
        cost[later] = rng.integers(50, 1000, len(later))
        cost[hi + 1] = 1000.0
        cost[hi] = 1.5  # (hi and hi + 1 share a lane on every geometry here)
        first = hi
    elif case == "last_batch":
        cost[[W - 4, W - 2]] = 9.0
        cost[W - 1] = 8.99
        cost[W - 3] = PREC
        first = W - 4
    elif case == "unrestricted_negative":
        unr = list(range(N_UNR))  # variables 0..2 = columns 1..3
        A[2:H - 1, 1:1 + N_UNR] *= np.where(rng.random((H - 3, N_UNR)) < 0.5, -1.0, 1.0)  # bounded both ways
        cost[1:1 + N_UNR] = [5.0, -9.0, 9.0]
        cost[40] = 8.5
        cost[later] = rng.integers(10, 100, len(later))
        first = 2
    elif case == "optimal":
        cost[[5, B, W - 1]] = PREC
        cost[[7, B + 1]] = 0.5 * PREC
        cost[[9, B + 2]] = 0.0
        first = 0
    else:
        raise ValueError(case)
    A[0, :] = cost
    return A, unr, first


def _answer(t, res):
    return (res.as_dict(), t.pivot_trace().tolist(), [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in t.download()],
            repr(t.evaluation))


def _solve(lib, case, geom, chk):
    A, unr, _first = planted(case, geom)
    _A, vibr, vibc = int_instance(H - 1, W - 1, SEED)
    t = Tableau(A, vibr, vibc, unr, precision=PREC, lib=lib)
    try:
        return _answer(t, t.simplex(check_cycles=chk)), t.get_counters() if hasattr(lib, "backend") else None
    finally:
        t.close()


def _params():
    out = []
    for case in CASES:
        for g in ((1, 2) if case == "unrestricted_negative" else tuple(GEOM)):  # (unrestricted variables: the headline geometries only)
            out.append((case, g))
    return out


_ORACLE = {}


def _oracle(lib, case, geom):
    if (case, geom) not in _ORACLE:
        _ORACLE[(case, geom)] = _solve(lib, case, geom, True)[0]
    return _ORACLE[(case, geom)]


@pytest.mark.parametrize("case,geom", _params(), ids=["%s-g%d" % p for p in _params()])
def test_oracle_enters_the_planted_column_first(oracle_lib, case, geom):
    res, trace = _oracle(oracle_lib, case, geom)[:2]
    first = planted(case, geom)[2]
    assert res["feasible"] and res["bounded"]
    if first == 0:
        assert trace == [] and res["pivots_phase2"] == 0
    else:
        assert len(trace) > 1 and trace[0][1] == first, trace[:2]


@pytest.mark.gpu
@pytest.mark.parametrize("chk", (False, True), ids=("chk0", "chk1"))
@pytest.mark.parametrize("case,geom", _params(), ids=["%s-g%d" % p for p in _params()])
def test_resident_pricing_equals_oracle(hip_lib, oracle_lib, monkeypatch, capfd, case, geom, chk):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_FORCE_PATH", "resident")
    if case == "unrestricted_negative":  # (JSLP_RES_GEOM forces lean builds without unrestricted variables: the policy picks g1 / g2)
        if geom == 2:
            monkeypatch.setenv("JSLP_RES_CPT", "4")
    else:
        monkeypatch.setenv("JSLP_RES_GEOM", str(geom))
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    want = _oracle(oracle_lib, case, geom)  # (cycle check on: with no cycle found its trace is the check-off run's too)
    capfd.readouterr()
    got, cnt = _solve(hip_lib, case, geom, chk)
    lines = LAUNCH.findall(capfd.readouterr().err)
    T, C, R = GEOM[geom]
    assert lines == ["k_simplex_resident<%d,%d,%d> unr %d lean 1" % (T, C, R, int(case == "unrestricted_negative"))], lines
    assert got[1] == want[1]  # the pivot trace: the same entering column on every pivot
    assert got == want
    assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), cnt
