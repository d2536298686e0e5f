"""The four selection rules of the simplex (simplex.ts) at their edges, on every launch shape that restates them, HIP against the CPU
oracle bit for bit:
  * pricing (simplex.ts:136-219): the earliest batch with a candidate, the largest value in it, the first column on ties;
  * the phase-1 leaving row (:39-54): the most negative RHS below -precision, the first row on ties;
  * the phase-1 entering column (:56-76): the largest -cost / coefficient over coefficients below -precision (every coefficient of an
    unrestricted column), by a strict `maxQuotient < quotient` from -Infinity: the first column on ties, never NaN or -Infinity;
  * the phase-2 ratio test (:271-303): the first degenerate row (coefficient > 0, |rhs| < precision), else the smallest quotient above
    precision by a strict `minQuotient > quotient` from +Infinity: the first row on ties, never +Infinity -- +Infinity alone is unbounded.

Each case plants the FIRST decision of one rule in the dense all-"<=" integer LP of tools/resident_stress.py (257 x 801, precision 1e-8:
2 rows per workgroup on 129 workgroups of the chip-wide kernels, partial pricing in batches of 50 columns) with the deciding rows and
columns where lanes, waves, workgroups and batches meet, and values at the thresholds, signed zeros, +-Infinity and NaN -- the last
ones also as they arise from finite input (1e301 / 2e-8; -cost / 0 on an unrestricted column, which the reference then pivots on).
The solve then runs to its end and everything is compared: the result struct, the pivot trace, the evaluation and every array of
download(), with NaN canonicalised (the GPU and x86 make different NaN bits; the reference cannot tell them apart) and -0.0 exact.
CPU part: the oracle makes the decision each case names."""
import hashlib
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
from jslpsolver_amd.engine import Tableau, simplex_many
from test_oracle_golden import replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resident_stress import int_instance  # noqa: E402

SEED = 9090
PREC = 1e-8
H, W = 257, 801
CE = 300  # the entering column of the ratio-test cases
LR = 100  # the leaving row of the phase-1 entering-column cases
BYSTANDER = 790  # the unrestricted column of the "+unr" variants
INF = float("inf")
NAN_POS = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
NAN_NEG = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
BELOW = np.nextafter(PREC, 0.0)  # one ulp below the precision
ABOVE = np.nextafter(PREC, INF)  # one ulp above it
KNOBS = ("JSLP_FORCE_PATH", "JSLP_RES_CPT", "JSLP_RES_LEAN", "JSLP_RES_GEOM", "JSLP_RES_RPB", "JSLP_RES_WIDE_TALL", "JSLP_XL",
         "JSLP_NO_WGLDS", "JSLP_INJECT_RESIDENT_ABORT_US", "JSLP_FUSED_P1")
LAUNCH = re.compile(r"^\[jslp\] launch (.*)$", re.M)
GEOM = {1: (1024, 2, 8), 2: (512, 4, 8), 3: (512, 4, 16), 4: (512, 6, 12), 5: (512, 8, 8)}


# ---- the planted instances -------------------------------------------------------------------------------------------------------
def _base():
    A, vibr, vibc = int_instance(H - 1, W - 1, SEED)
    rng = np.random.default_rng(SEED)
    A[0, 1:] = -rng.integers(1, 20, W - 1).astype(np.float64)  # nothing prices in unless a case says so
    return A, vibr, vibc


def _ratio(A):
    A[0, CE] = 10.0  # the only column that prices in
    A[1:, CE] = 1.0  # every other row's quotient is its RHS: 100 .. 500


def _ratio_sparse(A):
    A[0, CE] = 10.0
    A[1:, CE] = 0.0  # only the planted rows are looked at


def _phase1_rows(A, rows_rhs):
    """rows made ">=" rows on columns 11 (quotient -4: the winner) and 12 (quotient -6); columns 11 / 12 are cheap everywhere"""
    A[1:, [11, 12]] = 1.0
    A[0, 11], A[0, 12] = -4.0, -6.0
    for r, v in rows_rhs.items():
        A[r, 1:] = 0.0
        A[r, [11, 12]] = -1.0
        A[r, 0] = v


def _phase1_entering(A, coef_cost):
    """row LR (RHS -2, the only one below -precision) has exactly the given candidates; every candidate is cheap in the other rows"""
    cols = list(coef_cost)
    A[1:, cols] = 1.0
    A[LR, 1:] = 0.0
    A[LR, 0] = -2.0
    for c, (coef, cost) in coef_cost.items():
        A[LR, c] = coef
        A[0, c] = cost


def _case(name):
    """-> (A, vibr, vibc, unrestricted variables, expected first decision); the decision is (row, col) of the first pivot (row None:
    the case is about the column), ("unbounded", variable) or ("infeasible",)"""
    if name.endswith("+unr"):  # the same decision on the builds with unrestricted variables: one more that takes no part in it
        A, vibr, vibc, unr, want = _case(name[:-len("+unr")])
        A[0, BYSTANDER] = 0.0  # never priced in; in phase 1 its quotient is -0 / 0 = NaN (no planted leaving row holds it)
        return A, vibr, vibc, unr + [BYSTANDER - 1], want
    A, vibr, vibc = _base()
    unr = []
    if name == "ratio_tie":  # quotient 3 in workgroups 31 / 32 / 64 / 128, across lanes 63 | 64 and waves
        _ratio(A)
        for r in (63, 64, 65, 127, 128, 129, 256):
            A[r, 0], A[r, CE] = 6.0, 2.0
        want = (63, CE)
    elif name == "ratio_first_degenerate":  # a small positive quotient first, then two degenerate rows in different workgroups
        _ratio(A)
        A[21, 0] = 1e-3
        A[64, 0] = 0.5 * PREC
        A[201, 0] = -0.5 * PREC
        want = (64, CE)
    elif name == "ratio_negative_col_small_rhs":  # col < 0 with |rhs| < precision is not degenerate, and its quotient is not > 0
        _ratio(A)
        A[30, 0], A[30, CE] = 0.0, -1.0
        A[31, 0], A[31, CE] = 0.5 * PREC, -1.0
        A[150, 0], A[150, CE] = 4.0, 2.0
        want = (150, CE)
    elif name == "ratio_col_at_precision":  # |col| == precision is looked at, one ulp below is not
        _ratio(A)
        A[40, 0], A[40, CE] = 0.0, BELOW
        A[41, 0], A[41, CE] = 0.0, -BELOW
        A[70, 0], A[70, CE] = 0.0, PREC
        want = (70, CE)
    elif name == "ratio_quotient_at_precision":  # rhs == +-precision; quotient == precision (skipped), one ulp above (kept)
        _ratio(A)
        A[50, 0] = PREC
        A[51, 0] = -PREC
        A[52, 0], A[52, CE] = PREC, -1.0
        A[129, 0] = ABOVE
        A[200, 0] = 3 * PREC
        want = (129, CE)
    elif name == "ratio_negative_zero":  # rhs -0.0: degenerate under col > 0, a quotient of +0 under col < 0
        _ratio(A)
        A[3, 0], A[3, CE] = -0.0, 0.0
        A[64, 0], A[64, CE] = -0.0, -1.0
        A[65, 0] = -0.0
        want = (65, CE)
    elif name == "ratio_overflow_only":  # 1e301 / 2e-8 = +Infinity, twice, and nothing else: unbounded
        _ratio_sparse(A)
        A[3, 0], A[3, CE] = 1e301, 2e-8
        A[129, 0], A[129, CE] = 1e301, 2e-8
        want = ("unbounded", int(vibc[CE]))
    elif name == "ratio_overflow_beside_finite":  # +Infinity in workgroup 1, a finite (huge) quotient in workgroup 100
        _ratio_sparse(A)
        A[3, 0], A[3, CE] = 1e301, 2e-8
        A[200, 0], A[200, CE] = 1e300, 1.0
        want = (200, CE)
    elif name in ("ratio_unrestricted_negative", "ratio_unrestricted_degenerate"):
        # an unrestricted column enters with a negative reduced cost: quotient -rhs / col, degenerate test still col > 0 unflipped
        _ratio(A)
        unr = [CE - 1]
        A[0, CE] = -9.0
        A[20, 0], A[20, CE] = 0.0, -1.0  # (flipped, this row would be degenerate)
        A[100, 0], A[100, CE] = 6.0, -2.0
        A[150, 0], A[150, CE] = 3.0, -1.0  # ties row 100
        want = (100, CE)
        if name == "ratio_unrestricted_degenerate":
            A[200, 0] = 0.0
            want = (200, CE)
    elif name == "p1_leave_tie":  # equal most negative RHS in workgroups 31 and 64
        _phase1_rows(A, {2: -2.0, 63: -3.0, 129: -3.0})
        want = (63, 11)
    elif name == "p1_leave_at_precision":  # -precision is no candidate, one ulp below it is
        _phase1_rows(A, {10: -PREC, 64: -PREC, 130: -ABOVE})
        want = (130, 11)
    elif name == "p1_leave_negative_infinity":  # -Infinity wins, the first of two
        _phase1_rows(A, {3: -3.0, 64: -INF, 129: -INF})
        want = (64, 11)
    elif name == "p1_leave_nan":  # NaN (either sign) never leaves
        _phase1_rows(A, {129: -3.0})
        A[3, 0] = NAN_POS
        A[64, 0] = NAN_NEG
        want = (129, 11)
    elif name == "p1_enter_tie":  # quotient -3 across lanes and waves of every geometry; the first column wins
        cc = {c: (-1.0, -3.0) for c in (127, 128, 129, 255, 256, 511, 512, 767, 768)}
        cc.update({c: (-1.0, -5.0) for c in (5, 126, 300, 700)})
        _phase1_entering(A, cc)
        want = (LR, 127)
    elif name == "p1_enter_signed_zero":  # quotients -0.0 (column 127) and +0.0 (128, 129): equal, the first wins
        _phase1_entering(A, {5: (-1.0, -5.0), 127: (-1.0, -0.0), 128: (-1.0, 0.0), 129: (-1.0, 0.0), 300: (-1.0, -5.0)})
        want = (LR, 127)
    elif name == "p1_enter_coef_at_precision":  # coefficient -precision is no candidate (its quotient 5e8 would win)
        _phase1_entering(A, {5: (-1.0, -5.0), 50: (-PREC, 5.0), 300: (-ABOVE, 1.0), 700: (-1.0, -5.0)})
        want = (LR, 300)
    elif name == "p1_enter_nan_ahead":  # NaN quotients (both signs) and -Infinity ahead of the winner in its own lane
        _phase1_entering(A, {5: (-1.0, -5.0), 128: (-1.0, NAN_POS), 129: (-1.0, -2.0), 130: (-1.0, NAN_NEG), 131: (-1.0, -INF),
                             256: (-1.0, NAN_NEG), 257: (-1.0, -2.5), 512: (-1.0, -INF), 513: (-1.0, -3.0)})
        want = (LR, 129)
    elif name == "p1_enter_nonfinite_only":  # the only quotients are -Infinity and NaN: infeasible
        _phase1_entering(A, {128: (-1.0, -INF), 129: (-1.0, NAN_POS), 130: (-1.0, NAN_NEG), 512: (-1.0, -INF)})
        want = ("infeasible",)
    elif name == "p1_enter_positive_infinity":  # +Infinity quotients (cost +Infinity): the first of two wins
        _phase1_entering(A, {5: (-1.0, -5.0), 127: (-1.0, INF), 128: (-1.0, INF), 300: (-1.0, -5.0)})
        want = (LR, 127)
    elif name == "p1_enter_unrestricted_zero":  # an unrestricted column with a zero coefficient: -cost / 0 = +Infinity wins
        _phase1_entering(A, {5: (-1.0, -5.0), 40: (0.0, -3.0), 300: (-1.0, -5.0)})
        unr = [39]
        want = (LR, 40)
    elif name == "price_positive_infinity":  # +Infinity reduced costs across the wave boundary of the 2-column geometry
        A[0, [127, 128]] = INF
        A[0, CE] = 10.0
        want = (None, 127)
    elif name == "price_nan":  # NaN (either sign) never prices in; batch 0 holds nothing else
        A[0, 5], A[0, 6] = NAN_POS, NAN_NEG
        A[0, 60], A[0, 61] = 3.0, NAN_POS
        want = (None, 60)
    elif name == "price_unrestricted_negative_infinity":  # an unrestricted column at -Infinity prices in at +Infinity
        unr = [39]
        A[0, 40] = -INF
        A[0, 41] = 5.0
        A[20, 40], A[21, 40] = -1.0, -2.0
        want = (None, 40)
    else:
        raise ValueError(name)
    return A, vibr, vibc, unr, want


BASE_CASES = ("ratio_tie", "ratio_first_degenerate", "ratio_negative_col_small_rhs", "ratio_col_at_precision", "ratio_quotient_at_precision",
         "ratio_negative_zero", "ratio_overflow_only", "ratio_overflow_beside_finite", "ratio_unrestricted_negative",
         "ratio_unrestricted_degenerate", "p1_leave_tie", "p1_leave_at_precision", "p1_leave_negative_infinity", "p1_leave_nan",
         "p1_enter_tie", "p1_enter_signed_zero", "p1_enter_coef_at_precision", "p1_enter_nan_ahead", "p1_enter_nonfinite_only",
         "p1_enter_positive_infinity", "p1_enter_unrestricted_zero", "price_positive_infinity", "price_nan",
         "price_unrestricted_negative_infinity")
CASES = BASE_CASES + tuple(c + "+unr" for c in BASE_CASES if not _case(c)[3])
UNR_CASES = {c for c in CASES if _case(c)[3]}


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def _canon(x):
    """bytes of an array or a float with every NaN made the same NaN (-0.0 kept)"""
    a = np.asarray(x)
    if a.dtype.kind == "f":
        a = G.canon_nan(a)
    return np.ascontiguousarray(a).tobytes()


def _answer(t, res):
    d = res.as_dict()
    d = {k: (_canon(v) if isinstance(v, float) else v) for k, v in d.items()}
    return dict(res=d, trace=t.pivot_trace().tolist(), arrays=[hashlib.sha256(_canon(x)).hexdigest() for x in t.download()],
                evaluation=repr(t.evaluation), eval_bytes=_canon(t.evaluation))


def _tableau(lib, name):
    A, vibr, vibc, unr, _ = _case(name)
    return Tableau(A, vibr, vibc, unr, precision=PREC, lib=lib)


_ORACLE = {}


def _oracle(lib, name, chk=True):
    if (name, chk) not in _ORACLE:
        t = _tableau(lib, name)
        try:
            _ORACLE[(name, chk)] = _answer(t, t.simplex(check_cycles=chk))
        finally:
            t.close()
    return _ORACLE[(name, chk)]


@pytest.mark.parametrize("name", CASES)
def test_oracle_makes_the_planted_decision(oracle_lib, name):
    want = _case(name)[4]
    got = _oracle(oracle_lib, name)
    res, trace = got["res"], got["trace"]
    if want[0] == "unbounded":
        assert trace == [] and not res["bounded"] and res["feasible"], (res, trace[:2])
        assert res["unbounded_var_index"] == want[1]
    elif want[0] == "infeasible":
        assert trace == [] and not res["feasible"] and res["pivots_phase1"] == 0, (res, trace[:2])
    else:
        assert trace, res
        row, col = want
        assert trace[0][1] == col and (row is None or trace[0][0] == row), trace[:2]
        assert (res["pivots_phase1"] > 0) == name.startswith("p1_"), res


def test_planted_values_are_what_they_say():
    """the threshold values are exactly one ulp from the precision, the overflow is an overflow, NaN signs are both there"""
    assert BELOW < PREC < ABOVE and np.nextafter(BELOW, 1.0) == PREC and np.nextafter(PREC, 1.0) == ABOVE
    assert ABOVE / 1.0 > PREC and PREC / 1.0 == PREC
    with np.errstate(over="ignore"):
        assert np.float64(1e301) / np.float64(2e-8) == INF
    assert np.signbit(NAN_NEG) and not np.signbit(NAN_POS) and np.isnan(NAN_NEG) and np.isnan(NAN_POS)
    with np.errstate(divide="ignore"):
        assert -np.float64(-3.0) / np.float64(0.0) == INF


# ---- GPU: every launch shape with its own selection code ------------------------------------------------------------------------
# launch shape -> its environment (cases without unrestricted variables; _check_launch says what each must launch)
PLAIN = {
    "wg": {"JSLP_FORCE_PATH": "wg"},
    "wggen": {"JSLP_FORCE_PATH": "wg", "JSLP_NO_WGLDS": "1"},
    "sp": {"JSLP_FORCE_PATH": "sp"},
    "fused": {"JSLP_FORCE_PATH": "fused"},
    "g1": {"JSLP_FORCE_PATH": "resident", "JSLP_RES_GEOM": "1"},
    "g2": {"JSLP_FORCE_PATH": "resident", "JSLP_RES_GEOM": "2"},
    "g3": {"JSLP_FORCE_PATH": "resident", "JSLP_RES_GEOM": "3"},
    "g4": {"JSLP_FORCE_PATH": "resident", "JSLP_RES_GEOM": "4"},
    "g5": {"JSLP_FORCE_PATH": "resident", "JSLP_RES_GEOM": "5"},
    "resident4": {"JSLP_FORCE_PATH": "resident", "JSLP_RES_CPT": "4"},
    "general": {"JSLP_FORCE_PATH": "resident", "JSLP_RES_LEAN": "0"},
    "xl": {"JSLP_FORCE_PATH": "xl"},
    "auto": {},
}
UNR_MODES = ("auto", "wg", "wggen", "sp", "fused", "resident", "resident4", "general")


def _params():
    out = []
    for name in CASES:
        if name in UNR_CASES:
            modes = UNR_MODES
        else:
            modes = tuple(PLAIN)
        for m in modes:
            out.append((name, m, True))
            if m == "g1":
                out.append((name, m, False))  # (the headline instance without the cycle check)
    return out


def _env(mode):
    if mode == "resident":
        return {"JSLP_FORCE_PATH": "resident"}
    return PLAIN[mode]


def _check_launch(name, mode, lines, path, reached_phase2):
    """the case ran on the launch shape it targets"""
    unr = int(name in UNR_CASES)
    res_lines = [x for x in lines if x.startswith("k_simplex_resident<")]
    if mode in ("wg", "wggen"):
        assert path == "workgroup" and not lines, (path, lines)
    elif mode == "sp":
        assert path == "select+update" and lines == ["select+update"], lines
    elif mode == "fused":  # (phase 1 through k_fused_p1 -- one launch that finds no row when there is no phase 1 --, then phase 2)
        want = ["k_fused_p1<1,%d>" % unr] + (["k_pivot_fused<1,%d,0>" % unr] if reached_phase2 else [])
        assert path == "fused" and lines == want, (path, lines)
    elif mode in ("g1", "g2", "g3", "g4", "g5"):
        g = int(mode[1])
        T, C, R = GEOM[g]
        head = "k_simplex_resident<%d,%d,%d> unr 0 lean 1 " % (T, C, R)
        if g >= 3:  # the tall / wide geometries take phase 2 only: phase 1 goes through k_fused_p1 first
            assert lines[:1] == ["k_fused_p1<1,0>"], lines
            lines = lines[1:]
        if g >= 3 and not reached_phase2:
            assert lines == [], lines
        else:
            assert len(lines) == 1 and lines[0].startswith(head), lines
    elif mode == "xl":
        assert path == "resident-xl" and len(res_lines) == 1 and " xl 1 " in res_lines[0] and len(lines) == 1, lines
    elif mode == "general":
        assert len(lines) == 1 and re.match(r"k_simplex_resident<\d+,\d+,\d+> unr %d lean 0 " % unr, lines[0]), lines
    elif mode in ("resident", "resident4", "auto"):
        cpt = "4" if mode == "resident4" else r"\d+"
        assert len(lines) == 1 and re.match(r"k_simplex_resident<\d+,%s,\d+> unr %d lean 1 " % (cpt, unr), lines[0]), lines
    return len(res_lines)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,chk", _params(), ids=["%s-%s%s" % (n, m, "" if c else "-chk0") for n, m, c in _params()])
def test_selection_equals_oracle(hip_lib, hip_hooks_lib, oracle_lib, monkeypatch, capfd, name, mode, chk):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in _env(mode).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    want = _oracle(oracle_lib, name, chk)
    lib = hip_hooks_lib if mode == "xl" else hip_lib
    capfd.readouterr()
    t = _tableau(lib, name)
    try:
        got = _answer(t, t.simplex(check_cycles=chk))
        path = t.last_path()
        cnt = t.get_counters()
    finally:
        t.close()
    lines = LAUNCH.findall(capfd.readouterr().err)
    reached_phase2 = want["res"]["pivots_phase2"] >= 0  # (-1: phase 1 ended the solve)
    n_res = _check_launch(name, mode, lines, path, reached_phase2)
    assert got["trace"][:1] == want["trace"][:1]  # the planted decision first
    assert got["trace"] == want["trace"]
    assert got == want
    if n_res:
        assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), cnt


@pytest.mark.gpu
def test_selection_cases_in_one_many_batch(hip_lib, oracle_lib, monkeypatch, capfd):
    """every case as one LP of one jslpm_simplex_many call (one workgroup per LP)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_FORCE_PATH", "wg")
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    want = [_oracle(oracle_lib, n) for n in CASES]
    ts = [_tableau(hip_lib, n) for n in CASES]
    try:
        capfd.readouterr()
        results = simplex_many(ts, check_cycles=True)
        lines = LAUNCH.findall(capfd.readouterr().err)
        assert len(lines) == 1 and re.match(r"k_simplex_lds_many<\d+,opt 0> n %d " % len(CASES), lines[0]), lines
        for n, t, r, w in zip(CASES, ts, results, want):
            assert t.last_path() == "workgroup-many", n
            assert _answer(t, r) == w, n
    finally:
        for t in ts:
            t.close()


def _node_answer(res, rhs, rows):
    return (bool(res.feasible), bool(res.bounded), res.pivots_phase1, res.pivots_phase2, res.height, repr(res.evaluation),
            _canon(res.evaluation), hashlib.sha256(_canon(rhs)).hexdigest(), np.asarray(rows).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_selection_through_the_node_kernel(hip_lib, oracle_lib, monkeypatch, name):
    """save() on the unsolved planted tableau, then applyCuts([]): the single-child node kernel (k_node_lds) solves it"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    out = []
    for lib in (oracle_lib, hip_lib):
        t = _tableau(lib, name)
        try:
            t.save()
            res, rhs, rows = t.applyCuts([], check_cycles=True)
            out.append(_node_answer(res, rhs[:res.height], rows[:res.height]))
            if lib is hip_lib:
                assert t.last_path() == "workgroup"
        finally:
            t.close()
    assert out[1] == out[0]


@pytest.mark.gpu
def test_selection_through_the_node_queue():
    """every case as the nodes of batches larger than their slots (k_node_queue), the phase-1 leaving-row ties with a cut row that ties
    too; in a subprocess: JSLP_GROUP_MAX is read once per process"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env["JSLP_GROUP_MAX"] = "4"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "selection_node_worker.py")], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]


# ---- models on which the reference itself leaves the finite range (tests/golden/gen_golden_nonfinite.js) --------------------------
NONFINITE = os.path.join(G.GOLDEN, "nonfinite.json.gz")
NONFINITE_NAMES = ("overflow_ratio", "unrestricted_zero", "unrestricted_zero_neg", "overflow_pivot", "unrestricted_zero_mip",
                   "overflow_pivot_mip", "branch_overflow_mip", "branch_nonfinite_mip")
_GOLD = {}


def _nonfinite(name):
    if not _GOLD:
        _GOLD.update(G.load(NONFINITE))
    return _GOLD[name]


def test_nonfinite_goldens_are_what_they_say():
    """the reference did leave the finite range: +Infinity alone in a ratio test (unbounded), a pivot on zero (NaN), an overflow"""
    assert sorted(G.load(NONFINITE)) == sorted(NONFINITE_NAMES)
    assert not _nonfinite("overflow_ratio")["final"]["bounded"] and _nonfinite("overflow_ratio")["nPivots"] == 0
    for name in ("unrestricted_zero_neg", "unrestricted_zero_mip"):
        assert _nonfinite(name)["canonical"]["nonFinite"] > 0 and not _nonfinite(name)["final"]["feasible"]
    for name in ("overflow_pivot", "overflow_pivot_mip"):
        assert _nonfinite(name)["canonical"]["nonFinite"] > 0 and _nonfinite(name)["nPivots"] == 1
    assert _nonfinite("unrestricted_zero_mip")["tableau"]["integerVarIndexes"] and _nonfinite("overflow_pivot_mip")["tableau"]["integerVarIndexes"]
    for name in ("branch_overflow_mip", "branch_nonfinite_mip"):  # a finite root, then children with cuts that leave the finite range
        g = _nonfinite(name)
        calls, nonfinite = g["simplexCalls"], g["canonical"]["callNonFinite"]
        assert len(calls) > 2 and calls[0]["feasible"] and nonfinite[0] == 0 and any(nonfinite[1:]), (name, nonfinite)
        assert all(c["cuts"] for c in calls[1:]) and g["savedAfterCall"] == 0, name


@pytest.mark.parametrize("name", NONFINITE_NAMES)
def test_oracle_reproduces_reference_nonfinite(oracle_lib, name):
    replay(oracle_lib, _nonfinite(name))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["auto", "wg", "wggen", "sp", "fused", "resident", "resident4", "xl"])  # (test_gpu_parity.PATHS)
@pytest.mark.parametrize("name", NONFINITE_NAMES)
def test_nonfinite_goldens_on_every_path(hip_lib, hip_hooks_lib, name, mode):
    from test_gpu_parity import set_path
    set_path(mode)
    try:
        replay(hip_hooks_lib if mode == "xl" else hip_lib, _nonfinite(name))
    finally:
        set_path("auto")


@pytest.mark.gpu
def test_nonfinite_goldens_in_one_many_batch(hip_lib, monkeypatch, capfd):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    names = [n for n in NONFINITE_NAMES if not _nonfinite(n)["tableau"]["integerVarIndexes"]]
    ts = []
    for n in names:
        tab = _nonfinite(n)["tableau"]
        m, vibr, vibc = G.dense_tableau(tab)
        ts.append(Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], lib=hip_lib))
    try:
        capfd.readouterr()
        results = simplex_many(ts, check_cycles=[_nonfinite(n)["tableau"]["checkForCycles"] for n in names])
        lines = LAUNCH.findall(capfd.readouterr().err)
        assert len(lines) == 1 and re.match(r"k_simplex_lds_many<\d+,opt 0> n %d " % len(names), lines[0]), lines
        for n, t, r in zip(names, ts, results):
            g = _nonfinite(n)
            call = g["simplexCalls"][0]
            assert t.last_path() == "workgroup-many", n
            assert (bool(r.feasible), bool(r.bounded), r.pivots_phase1, r.pivots_phase2) == (call["feasible"], call["bounded"], call["p1"], call["p2"]), n
            ev = G.num(call["evaluation"])
            assert t.evaluation == ev or (np.isnan(ev) and np.isnan(t.evaluation)), n
            rhs, rows = t.read_rhs()
            assert G.sha_rhs(G.canon_nan(rhs), rows) == g["canonical"]["callRhsSha"][0], n
            assert t.pivot_trace().reshape(-1).tolist() == g["pivots"], n
            assert G.sha_matrix(G.canon_nan(t.download()[0])) == g["canonical"]["finalMatrixSha"], n
    finally:
        for t in ts:
            t.close()
