"""Helpers of tests/test_measure_modes.py: the instances, the independent count of a pivot trace, and what the contract of
include/jslp_engine.h (jslp_work_counters, jslp_engine_set_timing) makes of it on every launch shape.  No test functions, no HIP library:
everything here runs on numpy and on whatever engine library (the CPU oracle, in practice) the caller hands in.

The count is independent of the counters under test: the trace is replayed with Tableau.pivot(), the tableau is downloaded after every
pivot, and the rows and columns are counted from the downloaded cells -- the pivot column BEFORE the pivot, the pivot row AFTER it."""
import os
import re
import sys
import tempfile

import numpy as np

from jslpsolver_amd.engine import Tableau
from test_selection_edges import BASE_CASES, LAUNCH, UNR_CASES, _answer, _canon, _check_launch, _env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resident_stress import int_instance  # noqa: E402

PREC = 1e-8
GATE = 1e-16  # simplex.ts:370-375
S_SEED = 4242
WORK_FIELDS = ("relaxations", "simplex_calls", "pivots", "gated_cells", "gated_rows", "restored_rows", "cut_rows", "height_sum")
HEALTH_FIELDS = ("resident_launches", "resident_aborts", "resident_handovers", "resident_refusals")


# ---- instances ----------------------------------------------------------------------------------------------------------------------
def _s_matrix():
    """int_instance(256, 800, 4242, two_phase) with a third of its "<=" rows thinned to a quarter of their cells and 400 of the cells
    that are zero then set to 1e-17 / -3e-17: values a `!= 0` test sees and the reference's 1e-16 gate does not"""
    A, vibr, vibc = int_instance(256, 800, S_SEED, two_phase=True)
    rng = np.random.default_rng(S_SEED + 1)
    le = np.flatnonzero(A[1:, 0] >= 0) + 1
    thin = le[np.argsort(A[le, 0], kind="stable")[:len(le) // 3]]  # (the smallest limits: the rows likeliest to leave while their tiny cells are still there)
    A[np.ix_(thin, np.arange(1, A.shape[1]))] *= rng.random((len(thin), A.shape[1] - 1)) < 0.25
    rr, cc = np.nonzero(A[le, 1:] == 0.0)
    pick = rng.choice(len(rr), 400, replace=False)
    A[le[rr[pick]], 1 + cc[pick]] = np.where(rng.random(400) < 0.5, 1e-17, -3e-17)
    return A, vibr, vibc


def instance(name):
    """-> dict(A, vibr, vibc, unr, oo, check): S, S+unr, S+opt, the two 4 x 4 undecidable-pivot instances, the simplex_many LPs"""
    if name in ("S", "S+unr", "S+opt"):
        A, vibr, vibc = _s_matrix()
        unr, oo = [], None
        if name == "S+unr":
            unr = [5, 300, 790]
        if name == "S+opt":
            oo = np.random.default_rng(S_SEED + 2).integers(-5, 6, (2, A.shape[1])).astype(np.float64)
        # (S with the cycle check on, its variants without: the oracle's check is most of its time, and the CHK = false builds get their turn)
        return dict(name=name, A=A, vibr=vibr, vibc=vibc, unr=unr, oo=oo, check=name == "S")
    if name.startswith("slow_p"):  # tests/test_wide_goldens.py: test_fused_phase_1 / _2_hands_the_undecidable_pivot_over
        phase, other = name[len("slow_p")], float(name.split(":")[1])
        sign = -1.0 if phase == "1" else 1.0
        A = np.array([[0.0, 0.0, 0.0, 0.0], [sign * 1.0, sign * 1e5, 1e-15, 2.0], [5.0, other, 1.0, 1.0], [4.0, 0.0, 2.0, 1.0]])
        oo = np.array([[0.0, 7.0, 0.0, 0.0]]) if phase == "2" else None
        return dict(name=name, A=A, vibr=np.array([-1, 3, 4, 5], dtype=np.int32), vibc=np.array([-1, 0, 1, 2], dtype=np.int32), unr=[], oo=oo, check=True)
    if name.startswith("many"):  # S-like small LPs: "many:40x30", "many:14x11:nocheck", "many:60x90"
        parts = name.split(":")
        rows, cols = (int(x) for x in parts[1].split("x"))
        A, vibr, vibc = int_instance(rows - 1, cols - 1, S_SEED + rows, two_phase=True)
        rng = np.random.default_rng(S_SEED + cols)
        le = np.flatnonzero(A[1:, 0] >= 0) + 1
        thin = le[::3]
        A[np.ix_(thin, np.arange(1, cols))] *= rng.random((len(thin), cols - 1)) < 0.25
        rr, cc = np.nonzero(A[le, 1:] == 0.0)
        pick = rng.choice(len(rr), min(20, len(rr)), replace=False)
        A[le[rr[pick]], 1 + cc[pick]] = 1e-17
        return dict(name=name, A=A, vibr=vibr, vibc=vibc, unr=[], oo=None, check=len(parts) < 3)
    raise ValueError(name)


SLOW = ("slow_p1:0.0", "slow_p1:3.0", "slow_p2:0.0", "slow_p2:3.0")
MANY = ("many:40x30", "many:14x11:nocheck", "many:60x90")


def tableau(lib, inst, **kw):
    return Tableau(inst["A"], inst["vibr"], inst["vibc"], inst["unr"], precision=PREC, lib=lib, optional_objectives=inst["oo"], **kw)


# ---- the independent count ----------------------------------------------------------------------------------------------------------
def replay_count(lib, inst, trace):
    """Replays `trace` ((row, col) pairs) on a fresh tableau of `inst` with Tableau.pivot() and counts, per pivot, from the downloaded cells:
      gated_rows   rows r != r* (the cost row included) with |A[r, c*]| > 1e-16 before the pivot
      live_cols    columns of the pivot row after the pivot with |v| > 1e-16, plus c*
      nz_rows / nz_cols   the same two under a `!= 0` test (the columns from the pivot row before the pivot: the pivot zeroes the tiny ones)
      dense_rows / dense_cols   H - 1 and W
      tiny_col / tiny_row   the pivot column / the pivot row held a cell with 0 < |v| <= 1e-16 before the pivot
      undecidable  the NORMALISED pivot row holds such a cell (simplex.ts:381-383 zeroes it only if another row is gated) and the cost row's
                   entry in the pivot column does not settle that: the pivot a fused pipeline hands to k_select + k_update (ST_P1_SLOW)
    -> a structured array, one record per pivot, and the final matrix"""
    t = tableau(lib, inst)
    try:
        m = t.download()[0]
        H, W = m.shape
        out = np.zeros(len(trace), dtype=[(k, np.int64) for k in ("gated_rows", "live_cols", "nz_rows", "nz_cols", "dense_rows", "dense_cols", "tiny_col",
                                                                   "tiny_row", "undecidable")])
        for i, (r, c) in enumerate(np.asarray(trace).reshape(-1, 2).tolist()):
            col, row = m[:, c].copy(), m[r, :].copy()
            t.pivot(r, c)
            m = t.download()[0]
            others = np.arange(H) != r
            rec = out[i]
            rec["gated_rows"] = int(np.count_nonzero((np.abs(col) > GATE) & others))
            after = np.abs(m[r, :]) > GATE
            after[c] = True
            rec["live_cols"] = int(np.count_nonzero(after))
            rec["nz_rows"] = int(np.count_nonzero((col != 0.0) & others))
            before = row != 0.0
            before[c] = True
            rec["nz_cols"] = int(np.count_nonzero(before))
            rec["dense_rows"], rec["dense_cols"] = H - 1, W
            tiny = lambda v: bool(np.any((v != 0.0) & (np.abs(v) <= GATE)))  # noqa: E731
            rec["tiny_col"], rec["tiny_row"] = tiny(col[others]), tiny(np.delete(row, c))
            with np.errstate(all="ignore"):
                norm = np.where(np.abs(row) > GATE, row / row[c], 0.0)
            rec["undecidable"] = tiny(np.delete(norm, c)) and not abs(col[0]) > GATE
        return out, m
    finally:
        t.close()


def totals(count, rule, lo=0, hi=None):
    """(rows, cells) of pivots [lo, hi) under `rule`: "gated", "nz" or "dense" """
    rows, cols = {"gated": ("gated_rows", "live_cols"), "nz": ("nz_rows", "nz_cols"), "dense": ("dense_rows", "dense_cols")}[rule]
    part = count[lo:hi]
    return int(part[rows].sum()), int((part[rows] * part[cols]).sum())


# ---- the contract -------------------------------------------------------------------------------------------------------------------
# rule per phase of a simplex() call on each launch shape (include/jslp_engine.h, jslp_work_counters): the one-workgroup kernels and
# k_select + k_update count through the gate; k_fused_p1, k_pivot_fused and k_simplex_resident report every row and cell.
def phase_rules(mode):
    """-> (phase-1 rule, phase-2 rule, which pivots update_kernel_launches counts: "none", "phase2" or "all", resident launches)"""
    if mode in ("wg", "wggen", "many"):
        return "gated", "gated", "none", 0
    if mode == "sp":
        return "gated", "gated", "all", 0
    if mode == "fused":
        return "dense", "dense", "phase2", 0
    if mode == "fused-p1off":  # JSLP_FUSED_P1=0: phase 1 through k_select + k_update, untimed
        return "gated", "dense", "phase2", 0
    if mode in ("g3", "g4", "g5"):  # the tall / wide geometries: phase 1 through k_fused_p1, phase 2 in the cooperative launch
        return "dense", "dense", "phase2", 1
    if mode in ("g1", "g2", "resident", "resident4", "general", "xl", "auto"):
        return "dense", "dense", "all", 1
    raise ValueError(mode)


def expected_counters(count, p1, H, mode):
    """the eight work fields and the health fields of ONE counted simplex() call whose trace gave `count`, the first p1 pivots in phase 1.
    A fused pipeline (mode "fused", "fused-p1off", and phase 1 of "g3".."g5") hands its undecidable pivots to k_select + k_update: gated."""
    r1, r2, _, launches = phase_rules(mode)
    fused1 = mode in ("fused", "g3", "g4", "g5")
    fused2 = mode in ("fused", "fused-p1off")
    rows = cells = 0
    for i in range(len(count)):
        rule = r1 if i < p1 else r2
        if count["undecidable"][i] and (fused1 if i < p1 else fused2):
            rule = "gated"
        r, c = totals(count, rule, i, i + 1)
        rows, cells = rows + r, cells + c
    want = dict(relaxations=0, simplex_calls=1, pivots=len(count), gated_cells=cells, gated_rows=rows, restored_rows=0, cut_rows=0, height_sum=H)
    want.update(resident_launches=launches, resident_aborts=0, resident_handovers=0, resident_refusals=0)
    return want


def expected_launches(count, p1, mode):
    """update_kernel_launches of one timed simplex() call (include/jslp_engine.h, jslp_engine_set_timing)"""
    which = phase_rules(mode)[2]
    if which == "none":
        return 0
    if which == "all":
        return len(count)
    n = len(count) - p1
    if mode in ("fused", "fused-p1off"):  # ... performed by k_pivot_fused: not the ones it handed over
        n -= int(count["undecidable"][p1:].sum())
    return n


# ---- one measured solve and what it must show ------------------------------------------------------------------------------------------
class StderrLines:
    """the process's stderr (file descriptor 2: where the engine prints its JSLP_DEBUG_LAUNCH lines) into a temporary file while the block runs"""

    def __enter__(self):
        sys.stderr.flush()
        self._tmp = tempfile.TemporaryFile()
        self._saved = os.dup(2)
        os.dup2(self._tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        sys.stderr.flush()
        os.dup2(self._saved, 2)
        os.close(self._saved)
        self._tmp.seek(0)
        self.text = self._tmp.read().decode(errors="replace")
        self._tmp.close()
        sys.stderr.write(self.text)  # (nothing is swallowed)

    def launches(self):
        return LAUNCH.findall(self.text)


def full_answer(t, res):
    """test_selection_edges._answer (result struct, trace, evaluation, every array of download(), NaN canonicalised) and the objective rows"""
    a = _answer(t, res)
    a["objectives"] = _canon(t.optional_objectives()) if t.n_optional else b""
    return a


def solve_measured(lib, inst, counting, timing):
    """simplex() of `inst` on a fresh engine of `lib` under the two modes, with JSLP_DEBUG_LAUNCH set by the caller -> what was observed"""
    t = tableau(lib, inst)
    try:
        if counting:
            t.set_counting(True)
        if timing:
            t.set_timing(True)
        with StderrLines() as err:
            res = t.simplex(check_cycles=inst["check"])
        out = dict(ans=full_answer(t, res), path=t.last_path(), counters=t.get_counters(), timing=t.get_timing(), lines=err.launches())
        t.set_counting(True)
        out["after_second_set_counting"] = t.get_counters()
        t.set_timing(False)
        out["after_set_timing_off"] = t.get_timing()
        return out
    finally:
        t.close()


def check_measured(what, got, want_answer, exp, exp_launches, counting, timing):
    """one solve of solve_measured against the oracle's answer and the contract's counters (expected_counters) and launches"""
    assert got["ans"]["trace"] == want_answer["trace"], what
    assert got["ans"] == want_answer, what
    c = got["counters"]
    assert {k: c[k] for k in HEALTH_FIELDS} == {k: exp[k] for k in HEALTH_FIELDS}, (what, c)
    if counting:
        assert {k: c[k] for k in WORK_FIELDS} == {k: exp[k] for k in WORK_FIELDS}, (what, c, exp)
    else:
        assert all(c[k] == 0 for k in WORK_FIELDS), (what, c)
    assert all(v == 0 for k, v in got["after_second_set_counting"].items() if k in WORK_FIELDS + HEALTH_FIELDS), (what, got["after_second_set_counting"])
    upd_ms, launches, total_ms = got["timing"]
    if timing:
        assert launches == exp_launches, (what, got["timing"], exp_launches)
        assert total_ms > 0, (what, got["timing"])
        assert upd_ms > 0 or launches == 0, (what, got["timing"])
        assert upd_ms <= total_ms, (what, got["timing"])  # the inner event pairs lie inside the outer pair, on one stream
    else:
        assert (upd_ms, launches, total_ms) == (0.0, 0, 0.0), (what, got["timing"])
    assert got["after_set_timing_off"] == (0.0, 0, 0.0), (what, got["after_set_timing_off"])


def mode_env(mode):
    """the environment of a launch shape: test_selection_edges' modes, and "fused-p1off" (JSLP_FUSED_P1 is latched: a process of its own)"""
    if mode == "fused-p1off":
        return {"JSLP_FORCE_PATH": "fused", "JSLP_FUSED_P1": "0"}
    return _env(mode)


def check_lines(name, mode, lines, path, reached_phase2):
    """the solve ran on the launch shape the case names (its JSLP_DEBUG_LAUNCH lines and last_path); -> accepted cooperative launches"""
    unr, opt = int(name == "S+unr"), int(name == "S+opt" or name.startswith("slow_p2"))
    fused2 = "k_pivot_fused<1,%d,%d>" % (unr, opt)
    if name in SLOW and mode == "fused":  # (the pipeline starts over behind a handed-over pivot that did not end the solve)
        assert path == "fused" and lines[:1] == ["k_fused_p1<1,0>"] and set(lines[1:]) <= {fused2}, (path, lines)
        assert name.startswith("slow_p1") or len(lines) >= 2, lines
        return 0
    if mode == "fused-p1off":
        assert path == "fused" and lines == ["select+update", fused2], (path, lines)
        return 0
    if opt and mode == "fused":
        assert path == "fused" and lines == ["k_fused_p1<1,0>", fused2], (path, lines)
        return 0
    if opt and mode in ("auto", "resident"):
        assert path == "resident" and len(lines) == 1 and re.match(r"k_simplex_resident<\d+,\d+,\d+> unr 0 lean 1 opt 1 ", lines[0]), (path, lines)
        return 1
    # (test_selection_edges._check_launch tells the builds by its own case names: one of its cases with / without unrestricted variables)
    return _check_launch(sorted(UNR_CASES)[0] if unr else BASE_CASES[0], mode, lines, path, reached_phase2)


def run_case(lib, name, mode, w):
    """the four solves of one case (counting off / on x timing off / on, fresh engines) checked against `w`: dict(inst, ans, count, p1, p2, H)"""
    exp = expected_counters(w["count"], w["p1"], w["H"], mode)
    exp_launches = expected_launches(w["count"], w["p1"], mode)
    for counting in (False, True):
        for timing in (False, True):
            got = solve_measured(lib, w["inst"], counting, timing)
            what = "%s %s counting %d timing %d" % (name, mode, counting, timing)
            print(what, got["path"], got["lines"], got["counters"], got["timing"], flush=True)
            assert check_lines(name, mode, got["lines"], got["path"], w["p2"] >= 0) == exp["resident_launches"], what
            check_measured(what, got, w["ans"], exp, exp_launches, counting, timing)
