"""Helpers of tests/test_pack_edges.py and tests/test_pack_edges_gpu.py (not a test module): small LPs whose FIRST decision sits where the
pack kernels' own loops turn (jslpsolver_amd/csrc/jslp_packed.hip.h: k_simplex_packed's loop and its second copy pk_simplex, which
k_tree_packed runs per node).  Both restate select_step / prepare_pivot / update_rows_wg over LDS with thread loops `r = 1 + tid; r +=
THREADS`, reductions of their own (shuffles alone at 64 threads, block_reduce at 256), a row gate with lazy zeroing behind a
__syncthreads_or, a two-level cycle history (PK_HIST = 128 pairs in LDS, then the global copy) and capacities of their own.

Shapes (SHAPES).  The one-wave build takes at most 2048 cells at the row capacity, the four-wave build the rest:
  TALL64 131 x 15, WIDE64 13 x 131     deciding rows / columns 1, 63, 64, 65, 66, 128, 129, 130: index 64 is lane 63's first turn, 65 lane
                                       0's second, 129 lane 0's third; WIDE64 has 130 > 100 columns: partial pricing in batches of 50, whose
                                       boundaries 50|51 and 100|101 lie inside a thread turn
  TALL256 262 x 12, WIDE256 9 x 262    1, 64, 65, 128, 129, 192, 193, 255, 256, 257, 258, 261: the wave boundaries and thread 0's second turn
With the 2 cut rows of a tree's single integer variable the one-wave shapes stay within 2048 cells (133 x 15, 15 x 131).

Cases.  selection_cases(): every case of test_selection_edges.BASE_CASES with its "+unr" variant, written over a shape and its position
table -- the ratio test and the phase-1 leaving row on the tall shapes, pricing and the phase-1 entering column on the wide ones -- and the
cases the pack's loops make possible: ties whose first row sits in the LAST lane while later ones sit in lower lanes' later turns, ties
inside one thread, the earliest-batch rule inside one thread, pricing at the threshold, an unrestricted tie, and (soft_cases) the
optional-objective pricing at +-precision.  gate_cases(): the `|k| > 1e-16` gate of test_resident_update_fast_path.instance at the edges of
the update's row grid (RP = THREADS >> cshift rows at a time), and the lazy zeroing with and without an open gate.  history_cases(): cycles
detected at history lengths around PK_HIST = 128, reached with Klee-Minty blocks (2^n - 1 pivots in an (n + 1) x (n + 1) tableau).
capacity_lp(k): Klee-Minty n = 12 with k fillers, 4095 + k phase-2 pivots around JSLPP_HIST_CAP = 4096."""
import collections
import functools
import hashlib
import os
import struct
import sys

import numpy as np

import cycle_edges as E
import golden_util as G
from jslpsolver_amd import Model
from jslpsolver_amd.engine import Tableau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resident_stress import int_instance  # noqa: E402

SEED = 7171
PREC = 1e-8
GATE = 1e-16
INF = float("inf")
NAN_POS = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
NAN_NEG = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
BELOW = float(np.nextafter(PREC, 0.0))  # one ulp below the precision
ABOVE = float(np.nextafter(PREC, INF))  # one ulp above it
NEXT_UP = float(np.nextafter(np.float64(GATE), np.float64(1.0)))
PK_HIST = 128        # jslp_packed.hip.h: the first pairs of the history live in LDS
HIST_CAP = 4096      # JSLPP_HIST_CAP (include/jslpp_packed.h)
LDS_LIMIT = 65536
ROUTING_CELLS = 2048  # PACK_CELLS_WAVE (jslp_hip.hip): at most this many cells at the row capacity -> the one-wave build
TREE_ROWS = 2        # the rows a tree root gets beyond its height: the 2 cuts of its single integer variable (cut_rows, and row_extra)

# name, height, width, threads, tall, the deciding positions along the long side
Shape = collections.namedtuple("Shape", "name H W threads tall pos")
POS64 = (1, 63, 64, 65, 66, 128, 129, 130)
POS256 = (1, 64, 65, 128, 129, 192, 193, 255, 256, 257, 258, 261)
SHAPES = {s.name: s for s in (Shape("TALL64", 131, 15, 64, True, POS64), Shape("WIDE64", 13, 131, 64, False, POS64),
                              Shape("TALL256", 262, 12, 256, True, POS256), Shape("WIDE256", 9, 262, 256, False, POS256))}
CE = 5         # tall shapes: the entering column of the ratio-test cases
P1A, P1B = 3, 4  # tall shapes: the columns of the ">=" rows (quotient -4: the winner, and -6)
LR = 5         # wide shapes: the leaving row of the phase-1 entering-column cases
FILL = (5, 70)  # wide shapes: columns of ordinary candidates that lose (lanes in the middle of a wave, first and second turn at 64 threads)


def edge(shape):
    """(the LAST thread's first turn, thread 0's second turn, thread 1's second turn) along the long side: 64, 65, 66 / 256, 257, 258"""
    t = shape.threads
    return t, t + 1, t + 2


def tie_sets(shape):
    """position sets of a tie, each with the index that must win (the first): every deciding position; the last thread's first turn against
    lower threads' later turns (a reduction that prefers the lower lane on equal values picks a later index); two turns of one thread (a
    fold that prefers the later turn picks the later index)"""
    e0, e1, e2 = edge(shape)
    return {"all": shape.pos, "last_lane_first": tuple(p for p in shape.pos if p >= e0), "one_thread": (e2 - shape.threads, e2)}


class Case:
    """one LP: lp = (matrix, varIndexByRow, varIndexByCol, unrestricted variables); want = the first decision -- (row, column) of the first
    pivot (row None: the case is about the column), ("unbounded", variable), ("infeasible",), ("optimal",) (no pivot at all) or None (the
    case names no first decision)"""

    def __init__(self, name, shape, lp, want, optional=None, check=True, precision=PREC):
        self.name, self.shape, self.lp, self.want, self.check, self.precision = name, shape, lp, want, check, precision
        self.optional = None if optional is None else np.ascontiguousarray(optional, dtype=np.float64)
        self.finite = bool(np.isfinite(lp[0]).all())

    @property
    def threads(self):
        h, w = self.lp[0].shape
        return 64 if h * w <= ROUTING_CELLS else 256

    @property
    def tree_threads(self):
        h, w = self.lp[0].shape
        return 64 if (h + TREE_ROWS) * w <= ROUTING_CELLS else 256

    def with_zero_row(self):
        """the optional objectives of the case in an OPT build: its own, or ONE all-zero row, which prices nothing and must change nothing"""
        return self.optional if self.optional is not None else np.zeros((1, self.lp[0].shape[1]))


# ---- selection --------------------------------------------------------------------------------------------------------------------
def _base(shape):
    A, vibr, vibc = int_instance(shape.H - 1, shape.W - 1, SEED)
    rng = np.random.default_rng(SEED)
    A[0, 1:] = -rng.integers(1, 20, shape.W - 1).astype(np.float64)  # nothing prices in unless a case says so
    return A, vibr, vibc


def _ratio(A):
    A[0, CE] = 10.0  # the only column that prices in
    A[1:, CE] = 1.0  # every other row's quotient is its RHS: 100 .. 500


def _ratio_sparse(A):
    A[0, CE] = 10.0
    A[1:, CE] = 0.0  # only the planted rows are looked at


def _phase1_rows(A, rows_rhs):
    """rows made ">=" rows on columns P1A (quotient -4: the winner) and P1B (quotient -6); both columns are cheap everywhere"""
    A[1:, [P1A, P1B]] = 1.0
    A[0, P1A], A[0, P1B] = -4.0, -6.0
    for r, v in rows_rhs.items():
        A[r, 1:] = 0.0
        A[r, [P1A, P1B]] = -1.0
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


TALL_CASES = ("ratio_first_degenerate", "ratio_negative_col_small_rhs", "ratio_col_at_precision", "ratio_quotient_at_precision",
              "ratio_negative_zero", "ratio_overflow_only", "ratio_overflow_beside_finite", "ratio_unrestricted_negative",
              "ratio_unrestricted_degenerate", "p1_leave_at_precision", "p1_leave_only_at_precision", "p1_leave_negative_infinity", "p1_leave_nan")
WIDE_CASES = ("p1_enter_signed_zero", "p1_enter_coef_at_precision", "p1_enter_nan_ahead", "p1_enter_nonfinite_only",
              "p1_enter_positive_infinity", "p1_enter_unrestricted_zero", "price_positive_infinity", "price_nan",
              "price_unrestricted_negative_infinity",
              # what the pack's loops make possible
              "price_batch_in_thread", "price_batch_in_thread_tied", "price_later_batch_in_thread", "price_at_threshold",
              "price_unrestricted_tie", "price_unrestricted_tie_second")
TIED = {"ratio_tie": True, "p1_leave_tie": True, "p1_enter_tie": False, "price_tie": False}  # rule -> on the tall shapes


def _plant(shape, name):
    """-> (A, vibr, vibc, unrestricted variables, the first decision)"""
    A, vibr, vibc = _base(shape)
    P, T = shape.pos, shape.threads
    e0, e1, e2 = edge(shape)
    unr = []
    rule, _, which = name.partition("@")
    if rule in TIED:
        S = tie_sets(shape)[which]
        if rule == "ratio_tie":  # quotient 3 against 100 .. 500
            _ratio(A)
            for r in S:
                A[r, 0], A[r, CE] = 6.0, 2.0
            want = (S[0], CE)
        elif rule == "p1_leave_tie":  # equal most negative RHS, and a row in front of them that is less negative
            rows = {r: -3.0 for r in S}
            rows[2 if 2 not in S else 3] = -2.0
            _phase1_rows(A, rows)
            want = (S[0], P1A)
        elif rule == "p1_enter_tie":  # quotient -3; the others -5
            cc = {c: (-1.0, -3.0) for c in S}
            cc.update({c: (-1.0, -5.0) for c in FILL if c not in S})
            _phase1_entering(A, cc)
            want = (LR, S[0])
        else:  # price_tie: equal reduced costs in ONE pricing batch, the one of the last thread's first turn
            if which == "all":
                S = tuple(c for c in P if (c - 1) // 50 == (e0 - 1) // 50)
            elif which == "last_lane_first":
                S = (e0, e1, e2)
            A[0, list(S)] = 7.0
            if which == "one_thread":  # two turns of one thread lie in two batches: the tie is then the batch rule's; a third in the later batch
                A[0, S[1] + 1] = 7.0
            want = (None, S[0])
    elif name == "ratio_first_degenerate":  # a small positive quotient first, then two degenerate rows, the second in a lower lane's later turn
        _ratio(A)
        A[P[0], 0] = 1e-3
        A[e0, 0] = 0.5 * PREC
        A[e1, 0] = -0.5 * PREC
        want = (e0, CE)
    elif name == "ratio_negative_col_small_rhs":  # col < 0 with |rhs| < precision is not degenerate, and its quotient is not > 0
        _ratio(A)
        A[P[1], 0], A[P[1], CE] = 0.0, -1.0
        A[e0, 0], A[e0, CE] = 0.5 * PREC, -1.0
        A[e1, 0], A[e1, CE] = 4.0, 2.0
        want = (e1, CE)
    elif name == "ratio_col_at_precision":  # |col| == precision is looked at, one ulp below is not
        _ratio(A)
        A[P[1], 0], A[P[1], CE] = 0.0, BELOW
        A[e0, 0], A[e0, CE] = 0.0, -BELOW
        A[e1, 0], A[e1, CE] = 0.0, PREC
        want = (e1, CE)
    elif name == "ratio_quotient_at_precision":  # rhs == +-precision; quotient == precision (skipped), one ulp above (kept)
        _ratio(A)
        A[P[1], 0] = PREC
        A[e0, 0] = -PREC
        A[e0 - 1, 0], A[e0 - 1, CE] = PREC, -1.0
        A[e1, 0] = ABOVE
        A[e2, 0] = 3 * PREC
        want = (e1, CE)
    elif name == "ratio_negative_zero":  # rhs -0.0: degenerate under col > 0, a quotient of +0 under col < 0
        _ratio(A)
        A[P[0], 0], A[P[0], CE] = -0.0, 0.0
        A[e0, 0], A[e0, CE] = -0.0, -1.0
        A[e1, 0] = -0.0
        want = (e1, CE)
    elif name == "ratio_overflow_only":  # 1e301 / 2e-8 = +Infinity, twice, and nothing else: unbounded
        _ratio_sparse(A)
        A[e0, 0], A[e0, CE] = 1e301, 2e-8
        A[e1, 0], A[e1, CE] = 1e301, 2e-8
        want = ("unbounded", int(vibc[CE]))
    elif name == "ratio_overflow_beside_finite":  # +Infinity in the last lane's first turn, a finite (huge) quotient in lane 0's second
        _ratio_sparse(A)
        A[e0, 0], A[e0, CE] = 1e301, 2e-8
        A[e1, 0], A[e1, CE] = 1e300, 1.0
        want = (e1, CE)
    elif name in ("ratio_unrestricted_negative", "ratio_unrestricted_degenerate"):
        # an unrestricted column enters with a negative reduced cost: quotient -rhs / col, degenerate test still col > 0 unflipped
        _ratio(A)
        unr = [int(vibc[CE])]
        A[0, CE] = -9.0
        A[P[1], 0], A[P[1], CE] = 0.0, -1.0  # (flipped, this row would be degenerate)
        A[e0, 0], A[e0, CE] = 6.0, -2.0
        A[e1, 0], A[e1, CE] = 3.0, -1.0  # ties row e0
        want = (e0, CE)
        if name == "ratio_unrestricted_degenerate":
            A[e2, 0] = 0.0
            want = (e2, CE)
    elif name == "p1_leave_at_precision":  # -precision is no candidate, one ulp below it is
        _phase1_rows(A, {P[1]: -PREC, e0: -PREC, e1: -ABOVE})
        want = (e1, P1A)
    elif name == "p1_leave_only_at_precision":  # ... and with nothing below it there is no phase 1 at all: optimal without a pivot
        _phase1_rows(A, {P[1]: -PREC, e0: -PREC, e1: -PREC})
        want = ("optimal",)
    elif name == "p1_leave_negative_infinity":  # -Infinity wins, the first of two
        _phase1_rows(A, {P[0]: -3.0, e0: -INF, e1: -INF})
        want = (e0, P1A)
    elif name == "p1_leave_nan":  # NaN (either sign) never leaves: in front of the winner in its own thread, and in the last lane
        _phase1_rows(A, {e1: -3.0})
        A[e1 - T, 0] = NAN_POS
        A[e0, 0] = NAN_NEG
        want = (e1, P1A)
    elif name == "p1_enter_signed_zero":  # quotients -0.0 (column e0) and +0.0 (e1, e2): equal, the first wins
        _phase1_entering(A, {FILL[0]: (-1.0, -5.0), e0: (-1.0, -0.0), e1: (-1.0, 0.0), e2: (-1.0, 0.0), FILL[1]: (-1.0, -5.0)})
        want = (LR, e0)
    elif name == "p1_enter_coef_at_precision":  # coefficient -precision is no candidate (its quotient 5e8 would win)
        _phase1_entering(A, {FILL[0]: (-1.0, -5.0), e0: (-PREC, 5.0), e1: (-ABOVE, 1.0), FILL[1]: (-1.0, -5.0)})
        want = (LR, e1)
    elif name == "p1_enter_nan_ahead":  # NaN quotients (both signs) and -Infinity ahead of the winner in its own thread
        _phase1_entering(A, {FILL[0]: (-1.0, -5.0), e1 - T: (-1.0, NAN_POS), e1: (-1.0, -2.0), e2 - T: (-1.0, -INF), e2: (-1.0, -2.5),
                             e0: (-1.0, NAN_NEG), e0 - 1: (-1.0, -3.0), P[-1]: (-1.0, NAN_NEG)})
        want = (LR, e1)
    elif name == "p1_enter_nonfinite_only":  # the only quotients are -Infinity and NaN: infeasible
        _phase1_entering(A, {e0: (-1.0, -INF), e1: (-1.0, NAN_POS), e2: (-1.0, NAN_NEG), P[1]: (-1.0, -INF)})
        want = ("infeasible",)
    elif name == "p1_enter_positive_infinity":  # +Infinity quotients (cost +Infinity): the first of two wins
        _phase1_entering(A, {FILL[0]: (-1.0, -5.0), e0: (-1.0, INF), e1: (-1.0, INF), FILL[1]: (-1.0, -5.0)})
        want = (LR, e0)
    elif name == "p1_enter_unrestricted_zero":  # an unrestricted column with a zero coefficient: -cost / 0 = +Infinity wins
        _phase1_entering(A, {FILL[0]: (-1.0, -5.0), e1: (0.0, -3.0), FILL[1]: (-1.0, -5.0)})
        unr = [int(vibc[e1])]
        want = (LR, e1)
    elif name == "price_positive_infinity":  # +Infinity reduced costs in the last lane's first turn and lane 0's second; a finite one in their batch
        A[0, [e0, e1]] = INF
        A[0, e2 + 2] = 10.0
        want = (None, e0)
    elif name == "price_nan":  # NaN (either sign) never prices in; batch 0 holds nothing else
        A[0, 5], A[0, 6] = NAN_POS, NAN_NEG
        A[0, e0], A[0, e1] = 3.0, NAN_POS
        want = (None, e0)
    elif name == "price_unrestricted_negative_infinity":  # an unrestricted column at -Infinity prices in at +Infinity
        unr = [int(vibc[e1])]
        A[0, e1] = -INF
        A[0, e2] = 5.0
        A[2, e1], A[3, e1] = -1.0, -2.0
        want = (None, e1)
    elif name in ("price_batch_in_thread", "price_batch_in_thread_tied"):
        # thread 4 holds column 5 (batch 0, first turn) and column 5 + T (a later batch, second turn, larger); thread 1's second turn holds a
        # still larger one of that later batch: the earliest batch wins
        big, bigger = (3.0, 3.0) if name.endswith("_tied") else (5.0, 7.0)
        A[0, 5], A[0, 5 + T], A[0, 2 + T] = 3.0, big, bigger
        want = (None, 5)
    elif name == "price_later_batch_in_thread":  # nothing in batch 0: thread 54 holds column 55 (batch 1) and a larger one of a later batch
        A[0, 55], A[0, 55 + T] = 3.0, 9.0
        want = (None, 55)
    elif name == "price_at_threshold":  # a reduced cost equal to the precision does not price in, one ulp above it does
        A[0, e0], A[0, e1] = PREC, ABOVE
        want = (None, e1)
    elif name in ("price_unrestricted_tie", "price_unrestricted_tie_second"):  # an unrestricted column at -v ties a restricted one at +v
        first = name == "price_unrestricted_tie"
        u, r = (e0, e1) if first else (e1, e0)
        unr = [int(vibc[u])]
        A[0, u], A[0, r] = -7.0, 7.0
        A[2, u], A[3, u] = -1.0, -2.0
        want = (None, e0)
    else:
        raise ValueError(name)
    return A, vibr, vibc, unr, want


def _names(shape):
    tied = ["%s@%s" % (rule, which) for rule, on_tall in TIED.items() if on_tall == shape.tall for which in ("all", "last_lane_first", "one_thread")]
    names = tied + list(TALL_CASES if shape.tall else WIDE_CASES)
    if shape.W - 1 < 55 + shape.threads:  # (at 256 threads no thread has two turns beyond batch 0)
        names = [n for n in names if n != "price_later_batch_in_thread"]
    return names


@functools.lru_cache(maxsize=None)
def selection_cases():
    """every case on the two shapes of its side; a case without unrestricted variables also as "+unr": one more variable, unrestricted, that
    takes no part in the decision (in phase 1 its quotient is -0 / 0 = NaN: no planted leaving row holds it)"""
    out = []
    for shape in SHAPES.values():
        bystander = shape.W - 1 if shape.tall else 100  # (a column no case plants anything in)
        for name in _names(shape):
            A, vibr, vibc, unr, want = _plant(shape, name)
            out.append(Case("%s-%s" % (name, shape.name), shape, (A, vibr, vibc, unr), want))
            if not unr:
                A = A.copy()
                A[0, bystander] = 0.0
                out.append(Case("%s+unr-%s" % (name, shape.name), shape, (A, vibr, vibc, [int(vibc[bystander])]), want))
    return out


@functools.lru_cache(maxsize=None)
def soft_cases():
    """the optional-objective pricing (simplex.ts:221-263) on the wide shapes.  The cost row prices nothing; the deferred set is the columns
    within +-precision (open interval) on the cost row and on every earlier objective"""
    out = []
    for shape in (SHAPES["WIDE64"], SHAPES["WIDE256"]):
        e0, e1, e2 = edge(shape)
        far = shape.pos[1]
        W = shape.W

        def make(name, cost, rows, want, unr=(), neg_rows=()):
            A, vibr, vibc = _base(shape)
            for c, v in cost.items():
                A[0, c] = v
            for c in neg_rows:
                A[2, c], A[3, c] = -1.0, -2.0
            oo = np.zeros((len(rows), W))
            for o, row in enumerate(rows):
                for c, v in row.items():
                    oo[o, c] = v
            out.append(Case("%s-%s" % (name, shape.name), shape, (A, vibr, vibc, [int(vibc[c]) for c in unr]), want, optional=oo))

        # cost-row cells at +-BELOW are deferred, at exactly +-precision they are not (their larger optional values must not win)
        make("opt_cost_at_precision", {e0: PREC, e1: -PREC, e2: BELOW, far: -BELOW}, [{e0: 9.0, e1: 9.0, e2: 5.0, far: 3.0}], (None, e2))
        # the same boundary on objective 0, which decides whether objective 1 is consulted for the column
        make("opt_objective0_at_precision", {e0: 0.0, e1: 0.0, e2: 0.0, far: 0.0},
             [{e0: PREC, e1: -PREC, e2: BELOW, far: -BELOW}, {e0: 9.0, e1: 9.0, e2: 5.0, far: 3.0}], (None, e2))
        # a value one ulp above the precision on objective 0 wins there: objective 1 is not consulted at all
        make("opt_objective0_above_precision", {e0: 0.0, e1: 0.0, e2: 0.0}, [{e1: ABOVE}, {e0: 9.0, e2: 5.0}], (None, e1))
        # a tie in an optional row between the last thread's first turn and lower threads' second turns, and inside one thread
        make("opt_tie_turns", {e0: 0.0, e1: 0.0, e2: 0.0}, [{e0: 4.0, e1: 4.0, e2: 4.0}], (None, e0))
        make("opt_tie_one_thread", {e2 - shape.threads: 0.0, e2: 0.0, e1: 0.0}, [{e2 - shape.threads: 4.0, e2: 4.0, e1: 4.0}],
             (None, e2 - shape.threads))
        # an unrestricted column named by an optional row on a NEGATIVE coefficient: isReducedCostNegative comes from that row, the ratio test flips
        make("opt_unrestricted_negative", {e1: 0.0, e2: 0.0}, [{e1: -6.0, e2: 4.0}], (None, e1), unr=(e1,), neg_rows=(e1,))
        # ... and on the cost row a POSITIVE cell below the precision: the flag must not come from the cost row
        make("opt_unrestricted_negative_cost_positive", {e1: BELOW, e2: 0.0}, [{e1: -6.0, e2: 4.0}], (None, e1), unr=(e1,), neg_rows=(e1,))
    return out


# ---- the row gate and the lazy zeroing ------------------------------------------------------------------------------------------
C1, C2, C3 = 7, 9, 11   # price in first, second, third (first pricing batch)
NEGCOL = 13             # "zeros": the pivot row's NEGATIVE entry
PIVROW = 2              # the crafted cases' first pivot row (the smallest right-hand side)
# (threads, height, width): a width <= 32 (several rows per step), CW == THREADS, and a width past the thread count (the column loop turns twice)
GATE_SHAPES = ((64, 20, 24), (64, 20, 64), (64, 20, 70), (256, 90, 24), (256, 9, 256), (256, 9, 262))
GATE_KINDS = ("closed", "closed_first", "edge_closed", "edge_closed_neg", "edge_open", "zeros")


def update_grid(threads, W):
    """(CW, RP) of the row update: CW columns (a power of two covering the width, at most the workgroup) x RP rows at a time"""
    cshift = 0
    while (1 << cshift) < W and (1 << cshift) < threads:
        cshift += 1
    return 1 << cshift, threads >> cshift


def _zcols(W):
    """"zeros": the pivot row's zero entries -- single columns and runs, clear of C1 .. NEGCOL + 1"""
    return (2, 15, 16, 17, 18, 19, 20, 21) if W < 64 else (2, 20, 21, 24, 25, 26, 27, 40)


def gate_instance(kind, H, W, r):
    """test_resident_update_fast_path.instance's crafted cases with the planted row r (see its module text): column C1 prices in first with
    row PIVROW leaving, C2 second, C3 third"""
    rng = np.random.default_rng(515151 + 1000 * H + W)
    m, n = H - 1, W - 1
    A = np.zeros((H, W))
    A[1:, 1:] = rng.integers(1, 21, (m, n))
    A[0, 1:] = rng.integers(1, 51, n)
    A[1:, 0] = rng.integers(100, 501, m)
    vibr = np.array([-1] + list(range(n, n + m)), dtype=np.int32)
    vibc = np.array([-1] + list(range(n)), dtype=np.int32)
    A[0, C1] = 1000.0
    A[1:, C1] = 1.0
    A[PIVROW, 0] = 50.0
    A[0, C2] = 900.0
    A[1:, C2] = 1.0
    A[PIVROW, C2] = 0.5
    A[0, C3] = 300.0
    A[1:, C3] = (np.arange(1, H) + 3) ** 2 / 4096.0  # (squares: no two pivots' combinations cancel to an exact 0 in another row)
    if kind == "closed":
        A[r, C2] = 0.5  # 0.5 - 1 * 0.5: exactly +0 once pivot 1 is applied
    elif kind == "closed_first":
        A[r, C1] = 0.0
    elif kind == "edge_closed":
        A[r, C1] = GATE
    elif kind == "edge_closed_neg":
        A[r, C1] = -GATE
    elif kind == "edge_open":
        A[r, C1] = NEXT_UP
    elif kind == "zeros":
        neg_rows = [i for i in (1, 4, H - 1) if i != PIVROW and i != r]
        A[neg_rows, C1] = -1.0  # negative multipliers (never candidates of the ratio test)
        A[r, C1] = 0.0          # ... and one closed gate
        for q, c in enumerate(_zcols(W)):
            A[1:, c] = np.where(np.arange(1, H) % 2 == 0, -0.0, A[1:, c])
            A[neg_rows[0], c] = -0.0
            A[PIVROW, c] = 0.0 if q % 2 == 0 else -0.0
        lo = 64 * ((W - 1) // 64)  # every column of the last turn / wave: the pivot row is zero there
        if lo >= 64:
            A[PIVROW, lo:] = 0.0
            A[1, lo:] = -0.0
        A[PIVROW, NEGCOL] = -3.0
        A[r, NEGCOL] = -0.0      # closed gate: stays -0.0 (computed, -0 - (0 * -3) = +0)
        A[neg_rows[0], NEGCOL + 1] = -0.0
    else:
        raise ValueError(kind)
    return A, vibr, vibc


def gate_rows(threads, H, W):
    """the planted rows: the first step of the row grid, both sides of its first boundary, the last row"""
    RP = update_grid(threads, W)[1]
    return sorted({1, RP - 1, RP, RP + 1, H - 1} - {0, PIVROW} - set(range(H, H + RP + 2)))


@functools.lru_cache(maxsize=None)
def gate_cases():
    out = []
    for threads, H, W in GATE_SHAPES:
        shape = Shape("G%dx%d" % (H, W), H, W, threads, False, ())
        for kind in GATE_KINDS:
            for r in gate_rows(threads, H, W):
                A, vibr, vibc = gate_instance(kind, H, W, r)
                c = Case("%s@%d-%dx%d" % (kind, r, H, W), shape, (A, vibr, vibc, []), (PIVROW, C1))
                c.kind, c.row = kind, r
                out.append(c)
    return out


LZ_VAL, LZ_QUOT = 1e-10, -1e7   # a pivot-row entry above the gate whose quotient -1e-17 is nonzero and below it
LZ_RHS_QUOT = -1e17             # ... and a pivot under which the row's RIGHT-HAND SIDE -2 is such an entry (quotient 2e-17)


@functools.lru_cache(maxsize=None)
def lazy_zero_cases():
    """phase 1 picks row pr (the only negative RHS) and column pc (its only candidate, coefficient LZ_QUOT, cost 0); the pivot row holds
    LZ_VAL in column cx, whose quotient LZ_VAL / LZ_QUOT is nonzero and at most 1e-16 in magnitude (simplex.ts:381-383 zeroes it from inside
    the row loop: only when some other row's gate is open).  "none": column pc is zero everywhere else, the cost row included -- no row
    runs the loop, the quotient stays; "any": one other row has an entry; "cost": the cost row alone has one.  Nothing prices in afterwards:
    the cell is in the final tableau.  "rhs_*": the same with the coefficient LZ_RHS_QUOT, under which the row's right-hand side is the
    entry: the cell is in the RHS column, which a tree pack reads back too (it has no download())."""
    out = []
    for shape in SHAPES.values():
        e0, e1, e2 = edge(shape)
        if shape.tall:
            spots = [(pr, 3, shape.W - 1, other) for pr, other in ((e0, e1), (e1, e0), (1, shape.H - 1), (shape.H - 1, 1))]
        else:
            spots = [(LR, 3, cx, other) for cx, other in ((e0, 1), (e1, shape.H - 1), (shape.W - 1, 2))]
        for pr, pc, cx, other in spots:
            for kind in ("none", "any", "cost", "rhs_none", "rhs_any", "rhs_cost"):
                rhs = kind.startswith("rhs_")
                A, vibr, vibc = _base(shape)
                A[:, pc] = 0.0
                A[pr, 1:] = 0.0
                A[pr, 0], A[pr, pc], A[pr, cx] = -2.0, LZ_RHS_QUOT if rhs else LZ_QUOT, LZ_VAL
                if kind.endswith("any"):
                    A[other, pc] = 1.0
                elif kind.endswith("cost"):
                    A[0, pc] = -3.0
                c = Case("lazy_zero_%s@%d,%d-%s" % (kind, pr, cx, shape.name), shape, (A, vibr, vibc, []), (pr, pc))
                c.kind, c.cell, c.quotient = kind, (pr, 0 if rhs else cx), (-2.0 / LZ_RHS_QUOT if rhs else LZ_VAL / LZ_QUOT)
                out.append(c)
    return out


# ---- the cycle history around PK_HIST ----------------------------------------------------------------------------------------------
def klee_minty(n, tag, objective, cost_sign, scale):
    """maximise sum 2^(n-j) x_j subject to x_i + sum_{j<i} 2^(i-j+1) x_j <= 5^i: 2^n - 1 phase-2 pivots under Dantzig's rule"""
    cons = {"km%s_c%d" % (tag, i): {"max": float(5 ** i)} for i in range(1, n + 1)}
    variables = {}
    for j in range(1, n + 1):
        v = {objective: cost_sign * scale * float(2 ** (n - j))}
        for i in range(j, n + 1):
            v["km%s_c%d" % (tag, i)] = 1.0 if i == j else float(2 ** (i - j + 1))
        variables["km%s_x%d" % (tag, j)] = v
    return cons, variables


def blocks_then(small, blocks, scale=1e6):
    """block-diagonal Klee-Minty blocks (costs scaled so that they are spent before the small model is looked at, negated for a
    minimisation) in front of a small cycling golden's model"""
    sign = 1.0 if small["opType"] == "max" else -1.0
    big = {"optimize": small["optimize"], "opType": small["opType"], "constraints": {}, "variables": {}}
    for b, n in enumerate(blocks):
        cons, variables = klee_minty(n, str(b), small["optimize"], sign, scale)
        big["constraints"].update(cons)
        big["variables"].update(variables)
    big["constraints"].update(small["constraints"])
    big["variables"].update({name: dict(v) for name, v in small["variables"].items()})
    if "unrestricted" in small:
        big["unrestricted"] = dict(small["unrestricted"])
    big["options"] = {"presolve": False}
    return big


def km_lp(n, k=0, pad=0):
    """Klee-Minty alone with k fillers in front: 2^n - 1 + k phase-2 pivots in an (n + 1 + k)^2 tableau; pad: that many zero-cost variables
    and constraints of their own behind it (test_cycle_goldens._embed), which never take part"""
    cons, variables = klee_minty(n, "", "obj", 1.0, 1.0)
    base = {"optimize": "obj", "opType": "max", "constraints": cons, "variables": variables, "options": {"presolve": False}}
    base = E.with_fillers(base, k) if k else base
    model = Model(E._embed(base, pad, pad) if pad else base)
    return model.build_tableau() + (list(model.unrestricted),)


# (small golden, Klee-Minty blocks, fillers k, padding (variables, constraints) of test_cycle_goldens._embed or None) -> the class named
# under cycle_edges.classify(n, start, length, PK_HIST).  SMALL_BLOCKS spend 119 pivots, BIG_BLOCKS 78: with more fillers the tableau is
# beyond 2048 cells and the four-wave build runs it.
SMALL_BLOCKS, ACROSS_BLOCKS, BIG_BLOCKS = (6, 5, 4, 3, 2), (6, 5), (6, 4)
Hist = collections.namedtuple("Hist", "small blocks k want")
HISTORY = (
    [Hist("unr_3", SMALL_BLOCKS, k, w) for k, w in ((2, "below"), (3, "below"), (4, "n == B"), (5, "n == B + 1"), (6, "between the copies"),
                                                    (7, "first copy across"), (8, "beyond"), (9, "beyond"))] +
    [Hist("unr_3", BIG_BLOCKS, k + 41, w) for k, w in ((3, "below"), (4, "n == B"), (5, "n == B + 1"), (6, "between the copies"),
                                                       (7, "first copy across"), (8, "beyond"))])
ACROSS = ("deg_178868", "deg_233528")  # goldens of cycle length 6 and 7 (minimisations): the copies of the square can straddle the boundary


def hist_lp(small, blocks, k):
    model = Model(E.with_fillers(blocks_then(E.small_model(small), blocks), k))
    return model.build_tableau() + (list(model.unrestricted),)


def run_history(lib, lp, precision=PREC):
    """-> (history length at the hit, start, length, phase-1 pivots, phase-2 pivots) of the oracle's solve with the check on"""
    t = Tableau(*lp, precision=precision, lib=lib)
    try:
        res = t.simplex(check_cycles=True)
        trace = t.pivot_trace().tolist()
    finally:
        t.close()
    if not res.cycle_phase:
        return None, None, None, res.pivots_phase1, res.pivots_phase2
    p1, p2, _, _ = E.replay(trace, lp[1], lp[2], res.pivots_phase1)
    pairs = E.with_stop(p2 if res.cycle_phase == 2 else p1, res.cycle_start, res.cycle_length)
    n, hit = E.first_hit(pairs)
    assert hit == [res.cycle_start, res.cycle_length] and n == len(pairs)
    return n, res.cycle_start, res.cycle_length, res.pivots_phase1, res.pivots_phase2


_ACROSS = {}


def across_specs(lib):
    """for each golden of ACROSS and both block sets: the filler counts that put the hit where the second copy, and where the first copy,
    straddles pair PK_HIST -- computed from the hit without fillers (each filler shifts it by one pivot), asserted by the CPU part"""
    if not _ACROSS:
        for small in ACROSS:
            for blocks in (ACROSS_BLOCKS, BIG_BLOCKS):  # (11 and 27 or more fillers: below and above 2048 cells)
                n0, s0, L, _, _ = run_history(lib, hist_lp(small, blocks, 0))
                assert n0 is not None and n0 < PK_HIST, (small, blocks, n0)
                # second copy across: n - L < B < n, with the first copy below: n = B + L // 2; first copy across: start < B < start + L
                for want, n in (("second copy across", PK_HIST + L // 2), ("first copy across", PK_HIST + L + L // 2)):
                    _ACROSS[(small, blocks, want)] = Hist(small, blocks, n - n0, want)
    return list(_ACROSS.values())


def history_specs(lib):
    return HISTORY + across_specs(lib)


_HIST_CASES = {}


def history_cases(lib):
    if not _HIST_CASES:
        for h in history_specs(lib):
            lp = hist_lp(h.small, h.blocks, h.k)
            H, W = lp[0].shape
            c = Case("hist_%s_b%d_k%d" % (h.small, len(h.blocks), h.k), Shape("hist", H, W, 64 if H * W <= ROUTING_CELLS else 256, False, ()), lp, None)
            c.spec = h
            _HIST_CASES[c.name] = c
    return list(_HIST_CASES.values())


# ---- capacities -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def capacity_lp(k, pad=0):
    """Klee-Minty n = 12 with k fillers: 4095 + k phase-2 pivots, (13 + k)^2 cells; CAP_PAD: (13 + k + 34)^2 > 2048 cells, the four-wave build"""
    return km_lp(12, k, pad)


CAP_PAD = 34


def pivot_cap_cases():
    """the LPs of the max_pivots runs, one wave and four: a gate case (the pivot pending at the cap is the gated one) and a phase-1 LP
    (several ">=" rows: the cap ends phase 1)"""
    gates = [c for c in gate_cases() if c.kind == "closed" and c.shape.W == 24 and c.row == c.shape.H - 1]
    assert len(gates) == 2
    p1 = []
    for g in gates:  # test_resident_update_fast_path's "phase1": two ">=" rows (negative RHS) with one variable each
        H, W = g.lp[0].shape
        rng = np.random.default_rng(616161 + 1000 * H + W)
        A = np.zeros((H, W))
        A[1:, 1:] = rng.integers(1, 21, (H - 1, W - 1))
        A[0, 1:] = rng.integers(1, 51, W - 1)
        A[1:, 0] = rng.integers(60000, 100001, H - 1)
        for rr, c in ((2, 3), (H - 1, 5)):
            A[rr, 1:] = 0.0
            A[rr, c] = -1.0
            A[rr, 0] = -float(rng.integers(5, 21))
        p1.append(Case("phase1-%dx%d" % (H, W), g.shape, (A, g.lp[1], g.lp[2], []), None))
    return gates + p1


# ---- comparison: everything as bytes, NaN canonical, -0.0 exact -------------------------------------------------------------------------
def canon(x):
    a = np.asarray(x)
    if a.dtype.kind == "f":
        a = G.canon_nan(a)
    return np.ascontiguousarray(a).tobytes()


def canon_result(res):
    """the result struct as a dict with its floats canonical"""
    d = res.as_dict() if hasattr(res, "as_dict") else {k: res[k].item() for k in res.dtype.names}
    return {k: (canon(v) if isinstance(v, float) else v) for k, v in d.items()}


def engine_state(lib, lp, precision=PREC, check=True, optional=None, row_capacity=None):
    """the LP through jslp_engine_simplex on a FRESH engine of `lib`: what a pack must leave for it"""
    t = Tableau(*lp, precision=precision, lib=lib, optional_objectives=optional, row_capacity=row_capacity)
    try:
        res = t.simplex(check_cycles=check)
        rhs, rows = t.read_rhs()
        return dict(res=canon_result(res), evaluation=canon(np.float64(t.evaluation)), rhs=canon(rhs), rows=canon(rows),
                    trace=np.ascontiguousarray(t.pivot_trace(), dtype=np.int32).tobytes(),
                    arrays=[hashlib.sha256(canon(x)).hexdigest() for x in t.download()],
                    optional=canon(t.optional_objectives()) if optional is not None else b"")
    finally:
        t.close()


def pack_lp_state(pack, i, has_optional):
    rhs, rows = pack.read_rhs(i)
    return dict(res=canon_result(pack.result(i)), evaluation=canon(np.float64(pack.evaluation[i])), rhs=canon(rhs), rows=canon(rows),
                trace=np.ascontiguousarray(pack.pivot_trace(i), dtype=np.int32).tobytes(),
                arrays=[hashlib.sha256(canon(x)).hexdigest() for x in pack.download(i)],
                optional=canon(pack.optional_objectives(i)) if has_optional else b"")


def differing(a, b):
    return [k for k in a if a[k] != b[k]]


# ---- tree roots ---------------------------------------------------------------------------------------------------------------------
def nonbasic_variable(lib, case):
    """a variable that is non-basic in the oracle's final root tableau (restricted if there is one): its value is 0, the root is integral"""
    t = Tableau(*case.lp, precision=case.precision, lib=lib, optional_objectives=case.optional)
    try:
        t.simplex(check_cycles=case.check)
        vibc = t.download()[2]
    finally:
        t.close()
    unr = set(int(u) for u in case.lp[3])
    cands = [int(v) for v in vibc[1:] if int(v) not in unr] or [int(v) for v in vibc[1:]]
    return cands[0]


class TreeItem:
    """a case as the root of a tree with ONE integer variable: what tree_inc_util.make_pack reads of an item, for every kind of LP"""

    def __init__(self, case, integer, kind):
        self.case, self.lp, self.precision, self.check = case, case.lp, case.precision, case.check
        self.integers = [integer]
        self.cut_rows = self.row_extra = TREE_ROWS
        self.mir = kind == "mir"
        self.optional = case.with_zero_row() if kind == "opt" else None
        self.n_optional = 0 if self.optional is None else self.optional.shape[0]


TREE_KINDS = ("plain", "opt", "mir", "enh", "inc")
# the non-finite cases kept out of the tree packs: on them the host tree on the oracle does not end at the root --
# NaN or an infinity in the root's result sends it on to branch, or into an error -- so there is no one-iteration yardstick
LP_ONLY = ()


def tree_policy(kind):
    import tree_inc_util as I
    return {"enh": ("depth-first", "most-fractional"), "inc": I.Inc("best-first", "most-fractional", 2)}.get(kind)


def lp_cases(lib):
    """every case: the ones of the OPT builds only (their optional rows are the case) last"""
    return selection_cases() + gate_cases() + lazy_zero_cases() + history_cases(lib) + soft_cases()


_INTEGER = {}


def tree_items(lib, kind, cases=None):
    """the cases that become tree roots of this kind: every finite case and every non-finite one not listed in LP_ONLY; the cases with
    optional rows of their own in the OPT build only (without their rows they are other LPs)"""
    out = []
    for c in lp_cases(lib) if cases is None else cases:
        if c.name in LP_ONLY or (c.optional is not None and kind != "opt"):
            continue
        if c.name not in _INTEGER:
            _INTEGER[c.name] = nonbasic_variable(lib, c)
        out.append(TreeItem(c, _INTEGER[c.name], kind))
    return out


def tree_pack(lib, items, kind, trace_cap=512, **kw):
    import tree_inc_util as I
    return I.make_pack(lib, items, [tree_policy(kind)] * len(items), trace_cap=trace_cap, heap_cap=8, **kw)


def tree_state(pack, i):
    """everything the tree of LP i leaves, as bytes with NaN canonical: the result struct, the tree / MIR / enhanced / incremental records,
    the evaluation, the RHS column, the row map, the pivot trace, the optional rows (no download(): after a tree the arena holds the saved
    root, and jslpp_pack_download says so)"""
    rhs, rows = pack.read_rhs(i)
    return dict(res=canon_result(pack.results[i]), tree=pack.tree[i].tobytes(), mir=pack.mir[i].tobytes(), enhanced=pack.enhanced[i].tobytes(),
                incremental=pack.incremental[i].tobytes(), evaluation=canon(np.float64(pack.evaluation[i])), rhs=canon(rhs), rows=canon(rows),
                trace=np.ascontiguousarray(pack.pivot_trace(i), dtype=np.int32).tobytes(),
                optional=canon(pack.optional_objectives(i)))


def truncated_replay(lib, lp, n, precision=PREC, check=False):
    """-> (the first n entries of the oracle's pivot trace, the arrays of download() after the oracle's own pivot() applied to them on a
    fresh engine, the length of the whole trace): what a solve stopped by a capacity after n pivots must leave"""
    t = Tableau(*lp, precision=precision, lib=lib)
    try:
        t.simplex(check_cycles=check)
        trace = t.pivot_trace().tolist()
    finally:
        t.close()
    t = Tableau(*lp, precision=precision, lib=lib)
    try:
        for pr, pc in trace[:n]:
            t.pivot(pr, pc)
        arrays = [canon(x) for x in t.download()]
    finally:
        t.close()
    return np.asarray(trace[:n], dtype=np.int32).reshape(-1, 2), arrays, len(trace)
