"""The MIR row builders and the volume rule at their edges: a restatement, the instances, the defects.

* `restate()`: applyMIRCuts + addLowerBoundMIRCut (src/tableau/cutting-strategies.ts:74-135, 199-212) and computeFractionalVolume(true)
  (src/tableau/mip-utils.ts:67-92), sequential, in Python floats (IEEE doubles, no fused multiply-add), line by line.  One keyword switch
  per defect (`DEFECTS`): every switch that arithmetic lets one see must change what `restate` returns on a named instance
  (tests/test_mir_edges.py), the others are listed in `UNOBSERVABLE` with the reason.
* `INSTANCES`: pre-solved tableaus built from seeds at import time -- the cost row offers no entering column (every entry <= 0) and no
  right-hand side can leave (non-negative, or NaN / +Infinity, or negative in a row without a negative coefficient), so a root's
  applyCuts([]) makes zero pivots and the MIR code sees exactly what was planted.  vibr = [-1, W-1 .. W+H-3], vibc = [-1, 0 .. W-2].
  tests/golden/mir_edges.json.gz (gen_golden_mir_edges.js) holds the reference's own answer for every one of them, keyed by name and
  pinned by the sha256 of the input.

`python tests/mir_edges.py --dump` writes the instances as JSON (doubles as hex) to stdout: what the golden generator reads.
"""
import hashlib
import json
import math
import struct
import sys

import numpy as np

NAN = float("nan")
INF = float("inf")
MAX_CUTS = 10  # applyMIRCuts' maxCuts (cutting-strategies.ts:204)


# ---- JavaScript's Math functions on doubles -------------------------------------------------------------------------------------------
def js_floor(x):
    return float(math.floor(x)) if math.isfinite(x) else x  # Math.floor(NaN) = NaN, Math.floor(+-Infinity) = +-Infinity


def neg_zero(x):
    return x == 0 and math.copysign(1.0, x) < 0


def js_max(a, b):
    """Math.max(a, b): NaN if either is NaN; +0 is larger than -0"""
    if a != a or b != b:
        return NAN
    if a == 0 and b == 0:
        return b if neg_zero(a) else a
    return a if a > b else b


def js_min(a, b):
    """Math.min(a, b): NaN if either is NaN; -0 is smaller than +0"""
    if a != a or b != b:
        return NAN
    if a == 0 and b == 0:
        return a if neg_zero(a) else b
    return a if a < b else b


def c_fmax(a, b):
    """C's fmax: a NaN operand is dropped"""
    if a != a:
        return b
    if b != b:
        return a
    return js_max(a, b)


def c_fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return js_min(a, b)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def same_double(a, b):
    """NaN equals NaN, every other double by its bits (-0 is not +0)"""
    return (a != a and b != b) or bits(a) == bits(b)


def same_doubles(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


# ---- the defects ----------------------------------------------------------------------------------------------------------------------
# scan (what an ordered compaction over chunks of `threads` rows, waves of 64, can get wrong)
SCAN_DEFECTS = ("wave_rank", "chunk_rank", "cap_per_chunk", "first_chunk_only", "threshold_le_ge")
# cell arithmetic
CELL_DEFECTS = ("c_minmax", "min0_plus_zero", "rhs_as_minus_f", "reciprocal")
# volume
VOLUME_DEFECTS = ("pairwise", "per_chunk", "no_abs", "skip_nan")
DEFECTS = SCAN_DEFECTS + CELL_DEFECTS + VOLUME_DEFECTS
# Switches no input can show in an appended row, with the reason (tests/test_mir_edges.py sweeps the special values to back each claim):
UNOBSERVABLE = {
    "min0_plus_zero": "Math.min(0, q) is -0 only for q = -0, q = a / (1 - f) with 0 < 1 - f <= 1 is -0 only for a = -0 (a quotient by a divisor "
                      "<= 1 never underflows), and the cell is min0 - a: (-0) - (-0) and (+0) - (-0) are both +0",
    "rhs_as_minus_f": "floor(rhs) - rhs and -(rhs - floor(rhs)) are each other's negation rounded the same way; they differ only in the sign of a "
                      "zero, and a row with f = 0 is no candidate (f < precision); a NaN is a NaN either way",
}


def select_rows(cand, H, threads=None, wave_rank=False, chunk_rank=False, cap_per_chunk=False, first_chunk_only=False):
    """the rows applyMIRCuts cuts on, in order (:206-211): the first MAX_CUTS candidates.  With a scan defect: what a compaction over
    chunks of `threads` rows (row r is thread r - 1 - chunk * threads, waves of 64 lanes) writes into its selection slots; a slot nobody
    wrote is None"""
    if not (wave_rank or chunk_rank or cap_per_chunk or first_chunk_only):
        sel = []
        for r in range(1, H):  # :206
            if len(sel) >= MAX_CUTS:
                break
            if cand[r]:  # :208
                sel.append(r)  # :209
        return sel
    chunks = [[r for r in range(r0, min(r0 + threads, H)) if cand[r]] for r0 in range(1, H, threads)]
    if first_chunk_only:  # the scan ends after its first chunk
        return chunks[0][:MAX_CUTS]
    if cap_per_chunk:  # every chunk takes up to MAX_CUTS of its own
        return [r for rows in chunks for r in rows[:MAX_CUTS]]
    slots = {}
    base = 0
    for chunk, rows in enumerate(chunks):
        if base >= MAX_CUTS:
            break
        for before, r in enumerate(rows):
            pos = base + before
            if wave_rank and ((r - 1) % threads) >> 6 > 0:
                pos += 1  # the waves in front counted one too many
            if chunk_rank and chunk > 0 and base > 0:
                pos -= 1  # the chunks in front counted one too few
            if pos < MAX_CUTS:
                slots[pos] = r
        base += len(rows)
    return [slots.get(k) for k in range(min(base, MAX_CUTS))]


def restate(matrix, vibr, vibc, ints, precision, threads=256, **defect):
    """applyMIRCuts() and computeFractionalVolume(true) of the tableau (matrix H x W, the two maps, the set of integer variable indexes).
    Returns {"sel": source rows, "rows": the appended rows (n x W), "slacks": their variable indexes, "volume": of the tableau as given}"""
    unknown = set(defect) - set(DEFECTS)
    assert not unknown, unknown
    d = {k: bool(defect.get(k)) for k in DEFECTS}
    H, W = matrix.shape
    m = [[float(x) for x in row] for row in matrix]
    ints = set(int(i) for i in ints)

    def is_integer(v):  # variablesPerIndex[v] !== undefined && .isInteger (:82-85, :117-119)
        return int(v) >= 0 and int(v) in ints

    def fraction(r):
        rhs = m[r][0]  # :87
        return rhs - js_floor(rhs)  # :88

    def candidate(r):
        if not is_integer(vibr[r]):  # :82-85
            return False
        f = fraction(r)
        if d["threshold_le_ge"]:
            return not (f <= precision or f >= 1 - precision)
        return not (f < precision or f > 1 - precision)  # :89

    cand = [False] + [candidate(r) for r in range(1, H)]
    sel = select_rows(cand, H, threads, d["wave_rank"], d["chunk_rank"], d["cap_per_chunk"], d["first_chunk_only"])
    rows, slacks = [], []
    last_element_index = W + H - 2  # tableau.ts:312-316
    for r in sel:
        slacks.append(last_element_index)  # :108-111, getNewElementIndex (tableau.ts:393-401)
        last_element_index += 1
        if r is None:
            rows.append([NAN] * W)  # a slot nobody wrote: whatever row it names, it is not the reference's
            continue
        src = m[r]
        rhs = src[0]
        f = fraction(r)
        new = [0.0] * W
        new[0] = js_floor(rhs)  # :114
        for c in range(1, W):  # :116
            a = src[c]  # :118
            if is_integer(vibc[c]):  # :119
                fl = js_floor(a)
                x = a - fl - f
                mx = c_fmax(0.0, x) if d["c_minmax"] else js_max(0.0, x)
                new[c] = fl + (mx * (1 / (1 - f)) if d["reciprocal"] else mx / (1 - f))  # :120-124
            else:
                q = a * (1 / (1 - f)) if d["reciprocal"] else a / (1 - f)
                mn = c_fmin(0.0, q) if d["c_minmax"] else js_min(0.0, q)
                if d["min0_plus_zero"] and neg_zero(mn):
                    mn = 0.0
                new[c] = mn  # :126
        for c in range(W):  # :130-132
            new[c] = new[c] - src[c]
        if d["rhs_as_minus_f"]:
            new[0] = -f
        rows.append(new)
    return {"sel": sel, "rows": np.array(rows, dtype=np.float64).reshape(len(rows), W), "slacks": slacks,
            "volume": restate_volume([row[0] for row in m], vibr, ints, precision, threads, **{k: d[k] for k in VOLUME_DEFECTS})}


def restate_volume(rhs, vibr, ints, precision, threads=256, pairwise=False, per_chunk=False, no_abs=False, skip_nan=False):
    """computeFractionalVolume(ignoreIntegerValues = true), mip-utils.ts:67-92: the product is taken left to right in row order"""
    ints = set(int(i) for i in ints)
    volume = -1.0  # :68
    factors = []  # (row, distance) of the contributing rows, for the reordered products
    for r in range(1, len(vibr)):  # :73
        if not (int(vibr[r]) >= 0 and int(vibr[r]) in ints):  # :74-75
            continue
        value = float(rhs[r])  # :76
        distance = value if no_abs else abs(value)  # :77
        nearest = js_min(distance - js_floor(distance), js_floor(distance + 1))  # :79
        if skip_nan and nearest != nearest:
            continue
        if nearest < precision:  # :79 (false for NaN)
            continue  # :81-83 with ignoreIntegerValues === true
        factors.append((r, distance))
        volume = distance if volume == -1.0 else volume * distance  # :84-88
    if pairwise and factors:
        level = [x for _, x in factors]
        while len(level) > 1:
            level = [level[i] * level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
        return level[0]
    if per_chunk and factors:
        total = None
        for c in sorted(set((r - 1) // threads for r, _ in factors)):
            part = None
            for r, x in factors:
                if (r - 1) // threads == c:
                    part = x if part is None else part * x
            total = part if total is None else total * part
        return total
    return 0.0 if volume == -1.0 else volume  # :91


# ---- the instances --------------------------------------------------------------------------------------------------------------------
class Lcg:
    """a generator of the test's own: the instances must not move with a library's"""

    def __init__(self, seed):
        self.s = (seed * 2862933555777941757 + 3037000493) & 0xFFFFFFFFFFFFFFFF

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.s >> 33) % n


def maps(H, W):
    return (np.array([-1] + list(range(W - 1, W + H - 2)), dtype=np.int32), np.array([-1] + list(range(W - 1)), dtype=np.int32))


def row_var(W, r):
    return W - 2 + r  # vibr[r]


def col_var(c):
    return c - 1  # vibc[c]


def base_matrix(seed, H, W, steps=4, span=3):
    """cost row: negative multiples of 1/2 (no entering column); rows: multiples of 1 / steps in [-span, span]; integer right-hand sides"""
    g = Lcg(seed)
    m = np.zeros((H, W))
    for c in range(1, W):
        m[0, c] = -(1 + g.below(8)) / 2.0
    for r in range(1, H):
        m[r, 0] = float(20 + g.below(40))
        for c in range(1, W):
            m[r, c] = (g.below(2 * span * steps + 1) - span * steps) / float(steps)
    return m


def instance(name, family, m, ints, precision=1e-8, **notes):
    H, W = m.shape
    vibr, vibc = maps(H, W)
    out = {"name": name, "family": family, "H": H, "W": W, "precision": precision, "ints": sorted(int(i) for i in ints), "matrix": m, "vibr": vibr,
           "vibc": vibc}
    out.update(notes)
    return out


def sha_input(inst):
    """what pins an instance: the matrix bytes, the two maps, the integer indexes and the precision"""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(inst["matrix"], dtype="<f8").tobytes())
    h.update(np.ascontiguousarray(inst["vibr"], dtype="<i4").tobytes())
    h.update(np.ascontiguousarray(inst["vibc"], dtype="<i4").tobytes())
    h.update(np.array(inst["ints"], dtype="<i4").tobytes())
    h.update(struct.pack("<d", inst["precision"]))
    return h.hexdigest()


# -- scan family: W = 9 (ld = 16); chunk turns at rows 257 / 513 / 769 / 1025 (256 threads), 513 / 1025 (512), 1025 (1024); wave turns 64 | 65
SCAN_W = 9
SCAN_INT_COLS = (1, 2, 3, 4)  # the columns under an integer variable; 5 .. 8 are continuous


def scan_fraction(r):
    """every candidate its own fraction: k / 1024, distinct for rows 1 .. 1023"""
    return ((r * 37) % 1023 + 1) / 1024.0


def scan_instance(name, H, candidates, seed):
    """candidates: the rows that cut.  Every other row is one of three decoys, in turn: an integer variable at an integer value, a
    continuous variable at a fractional value, an integer variable within the precision of an integer (1e-9 above)"""
    W = SCAN_W
    m = base_matrix(seed, H, W)
    ints = set(col_var(c) for c in SCAN_INT_COLS)
    cand = set(candidates)
    for r in range(1, H):
        if r in cand:
            ints.add(row_var(W, r))
            m[r, 0] += scan_fraction(r)
        elif r % 3 == 0:
            ints.add(row_var(W, r))
        elif r % 3 == 1:
            m[r, 0] += scan_fraction(r)  # (its variable is continuous)
        else:
            ints.add(row_var(W, r))
            m[r, 0] += 1e-9
    return instance(name, "scan", m, ints, candidates=sorted(cand))


def scan_instances():
    H = 1040
    return [
        scan_instance("scan_turns", H, [3, 64, 65, 256, 257, 512, 513, 1024, 1025, 1039], 101),  # exactly ten, the last row among them
        scan_instance("scan_tenth_opens_a_chunk", H, [5, 63, 64, 128, 129, 300, 511, 700, 1024, 1025, 1026], 102),  # the eleventh is dropped
        scan_instance("scan_early_exit", H, list(range(1, 11)) + list(range(300, H)), 103),
        scan_instance("scan_past_the_cap", H, list(range(250, 260)) + list(range(300, H)), 104),  # base + before far past the cap in chunk 0/1
        scan_instance("scan_all", H, list(range(1, H)), 105),
        scan_instance("scan_none", H, [], 106),
        scan_instance("scan_one_row", 2, [1], 107),
        scan_instance("scan_66", 66, [1, 2, 33, 64, 65], 108),
    ]


# -- value family: 24 x 20 (ld = 32), at precision 1e-8 and at 0.25 (thresholds exactly representable); odd columns are integer
VALUE_H, VALUE_W = 24, 20


def ulp_down(x):
    return math.nextafter(x, -INF)


def ulp_up(x):
    return math.nextafter(x, INF)


def value_cells(f):
    """the cells planted under an integer and under a continuous column of a source row whose fraction is f (f finite; else 0.5 stands in)"""
    if not math.isfinite(f):
        f = 0.5
    equal = 2.0 + f if (2.0 + f) - 2.0 - f == 0.0 else f  # a - floor(a) - f == 0.0 exactly
    assert equal - js_floor(equal) - f == 0.0
    return [("zero", 0.0), ("neg_zero", -0.0), ("three", 3.0), ("neg_three", -3.0), ("frac_below", 2.0 + f / 2), ("frac_equal", equal),
            ("frac_above", 2.0 + (f + 1.0) / 2), ("neg_frac", -1.375), ("two_53", 2.0 ** 53), ("e300", 1e300), ("subnormal", 5e-324), ("inf", INF),
            ("neg_inf", -INF), ("nan", NAN)]


def value_rhs(p):
    """(label, right-hand side, cuts?) row by row from row 1"""
    return [("f_eq_precision", p, True), ("f_ulp_below_precision", ulp_down(p), False), ("f_eq_one_minus_precision", 1.0 - p, True),
            ("f_ulp_above_one_minus_precision", ulp_up(1.0 - p), False), ("negative", -2.75, True), ("two_52_plus_half", 2.0 ** 52 + 0.5, False),
            ("two_51_plus_half", 2.0 ** 51 + 0.5, True), ("neg_zero", -0.0, False), ("nan", NAN, True), ("inf", INF, True), ("neg_inf", -INF, True),
            ("plain_a", 7.3125, True), ("plain_b", 5.5, True)]
    # (2^52 + 0.5 is not a double: the sum rounds to 2^52, an integer, and the row does not cut; 2^51 + 0.5 is the largest magnitude class
    #  that still has a fraction)


def value_instance(p, tag):
    H, W = VALUE_H, VALUE_W
    m = base_matrix(201, H, W, steps=8)
    ints = set(col_var(c) for c in range(1, W) if c % 2 == 1)
    planted = {}  # (row, col) -> label
    rows = value_rhs(p)
    k = 0
    for i, (label, rhs, cuts) in enumerate(rows):
        r = i + 1
        ints.add(row_var(W, r))
        m[r, 0] = rhs
        if not cuts:
            continue
        f = rhs - js_floor(rhs)
        cells = value_cells(f)
        for c in range(1, W):
            j = (c - 1) // 2
            label_c, x = cells[(j + 3 * k) % len(cells)]
            m[r, c] = x
            planted[(r, c)] = label_c
        k += 1
    for r in range(len(rows) + 1, H):  # the rest: integer variables at integer values and continuous ones at fractions
        if r % 2 == 0:
            ints.add(row_var(W, r))
        else:
            m[r, 0] += 0.5
    return instance("value_" + tag, "value", m, ints, precision=p, rhs_rows=[(i + 1, label, cuts) for i, (label, _, cuts) in enumerate(rows)],
                    planted=planted)


# -- width family: 12 rows; W = 16 (no padding column), 17, 258, 1026; a column is continuous when its index is a multiple of 3
WIDTHS = (16, 17, 258, 1026)
WIDTH_COLS = (1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
WIDTH_CANDIDATES = (2, 3, 5, 7, 8, 11)


def width_instance(W):
    H = 12
    m = base_matrix(300 + W, H, W, steps=8)
    ints = set(col_var(c) for c in range(1, W) if c % 3 != 0)
    cols = sorted(set(c for c in WIDTH_COLS if c < W) | {W - 1})
    for k, r in enumerate(WIDTH_CANDIDATES):
        ints.add(row_var(W, r))
        m[r, 0] += (2 * k + 3) / 16.0
        for j, c in enumerate(cols):  # distinct non-trivial cells on both sides of the 256- / 512- / 1024-thread column turns
            m[r, c] = (-1) ** (j + k) * (1.0 + (2 * (7 * j + 3 * k) + 1) / 64.0)  # (an odd count of 64ths: never an integer)
    for r in range(1, H):
        if r not in WIDTH_CANDIDATES and r % 2 == 0:
            ints.add(row_var(W, r))
    return instance("width_%d" % W, "width", m, ints, candidates=list(WIDTH_CANDIDATES), turn_cols=cols)


# -- volume family: H = 1040, W = 9
def volume_instance(name, values, seed, blocked=()):
    """values: {row: right-hand side} of rows under an integer variable; every other row holds a continuous variable at a fraction.
    blocked: rows with a negative right-hand side -- their coefficients are made non-negative, so phase 1 finds no entering column, makes
    no pivot and calls the tableau infeasible; the most negative right-hand side of the tableau must be one of them"""
    H, W = 1040, SCAN_W
    m = base_matrix(seed, H, W)
    ints = set(col_var(c) for c in SCAN_INT_COLS)
    for r in range(1, H):
        if r in values:
            ints.add(row_var(W, r))
            m[r, 0] = values[r]
        else:
            m[r, 0] += 0.5
    for r in blocked:
        m[r, 1:] = np.abs(m[r, 1:])
    return instance(name, "volume", m, ints, values=dict(values), blocked=list(blocked))


def product_rows():
    """about 300 contributing rows spread over the turns at rows 257 / 513 / 1025"""
    rows = list(range(200, 320)) + list(range(480, 560)) + list(range(980, 1039))
    return {r: (1 + (k % 13)) / 7.0 for k, r in enumerate(rows)}  # 1/7 .. 13/7: below and above 1; 7/7 is an integer and contributes nothing


def volume_instances():
    prod = product_rows()
    out = [volume_instance("volume_product", prod, 401)]
    mixed = {r: (-v if k % 3 == 0 else v) for k, (r, v) in enumerate(sorted(prod.items())[:40])}
    mixed[7] = -2.75
    out.append(volume_instance("volume_negative_rows", mixed, 402, blocked=[r for r, v in mixed.items() if v < 0]))
    near = {10: 4.0 + 5e-9, 11: 6.0 - 5e-9, 300: 1.5, 600: 3.0 - 5e-9, 601: 2.0 + 5e-9, 1030: 2.25}
    out.append(volume_instance("volume_near_integer", near, 403))
    out.append(volume_instance("volume_nan_row", {5: 1.5, 258: NAN, 700: 2.5}, 404))
    out.append(volume_instance("volume_inf_row", {5: 1.5, 514: INF, 700: 2.5}, 405))
    out.append(volume_instance("volume_overflow", {r: 2.0 ** 51 + 0.5 for r in range(500, 525)}, 406))
    out.append(volume_instance("volume_none", {r: float(r % 7) for r in range(1, 1040, 3)}, 407))
    return out


# -- loop family: NaN right-hand sides in integer rows of a pre-solved tableau: the volume is NaN on every round and the rule never stops
def loop_instance():
    H, W = 12, SCAN_W
    m = base_matrix(501, H, W)
    ints = set(col_var(c) for c in SCAN_INT_COLS)
    for r in range(1, H):
        ints.add(row_var(W, r))
    m[3, 0] = NAN
    m[7, 0] = NAN
    m[9, 0] = INF
    return instance("loop_nan", "loop", m, ints, rows_per_round=3)


def build_instances():
    out = scan_instances()
    out += [value_instance(1e-8, "1e-8"), value_instance(0.25, "quarter")]
    out += [width_instance(W) for W in WIDTHS]
    out += volume_instances()
    out.append(loop_instance())
    return out


INSTANCES = build_instances()
BY_NAME = {i["name"]: i for i in INSTANCES}
assert len(BY_NAME) == len(INSTANCES)


def restate_instance(inst, **defect):
    return restate(inst["matrix"], inst["vibr"], inst["vibc"], inst["ints"], inst["precision"], **defect)


def make_tableau(lib, inst, extra_rows=10, Tableau=None):
    """the instance on an engine of `lib`; row_capacity = H + extra_rows"""
    if Tableau is None:
        from jslpsolver_amd import Tableau
    return Tableau(inst["matrix"], inst["vibr"], inst["vibc"], precision=inst["precision"], row_capacity=inst["H"] + extra_rows, lib=lib,
                   integer_variables=inst["ints"])


def nodes_of(inst):
    """five differing nodes of the instance's root: none, a bound on a non-basic integer variable that holds (no pivot in front of the loop),
    one that does not (phase 1 pivots), both, and a bound on the basic integer variable of the first candidate row"""
    hold = {"type": "max", "varIndex": col_var(1), "value": 3.0}
    move = {"type": "min", "varIndex": col_var(2), "value": 1.0}
    last = {"type": "max", "varIndex": col_var(4), "value": 2.0}
    for r in inst.get("candidates", []):
        rhs = float(inst["matrix"][r, 0])
        if math.isfinite(rhs):
            last = {"type": "max", "varIndex": row_var(inst["W"], r), "value": js_floor(rhs)}
            break
    return [[], [hold], [move], [hold, move], [last]]


# the one-call form's max_rounds per instance: None = the default service's unbounded loop.  Where the volume is NaN the rule never stops the
# loop, so these get a round limit (what an unbounded loop does with them is the loop family's question)
ROUNDS = {"value_1e-8": 2, "value_quarter": 2, "volume_nan_row": 2, "loop_nan": 5}
ONE_CALL_EXTRA_ROWS = 80  # row capacity of the one-call runs beyond H: the longest sequence adds 2 cut rows + 47 MIR rows


def rounds_of(inst):
    return ROUNDS.get(inst["name"])


def root_tableau(lib, inst, extra_rows):
    """the instance as a saved root: applyCuts([]) (zero pivots on a pre-solved tableau) and save()"""
    t = make_tableau(lib, inst, extra_rows)
    res, _, _ = t.applyCuts([], check_cycles=True)
    t.save()
    return t, res


def wglds_bytes(ld, cap_rows):
    """jslp_wglds.hip.h's wglds_bytes: the dynamic LDS of the LDS node kernels (launched with at most 64 KiB)"""
    hc = (cap_rows + 1) & ~1
    return 8 * (2 * ld + 2 * hc) + 4 * hc + 4 * hc + 4 * ld + hc


def leading_dimension(W):
    return (W + 15) & ~15


def hex_doubles(a):
    return np.ascontiguousarray(a, dtype="<f8").tobytes().hex()


def from_hex(text):
    return np.frombuffer(bytes.fromhex(text), dtype="<f8").copy()


def dump(fh):
    doc = [{"name": i["name"], "family": i["family"], "H": i["H"], "W": i["W"], "precision": hex_doubles([i["precision"]]), "ints": i["ints"],
            "matrix": hex_doubles(i["matrix"]), "vibr": [int(v) for v in i["vibr"]], "vibc": [int(v) for v in i["vibc"]], "sha": sha_input(i)}
           for i in INSTANCES]
    json.dump(doc, fh)


if __name__ == "__main__":
    if sys.argv[1:] == ["--dump"]:
        dump(sys.stdout)
    else:
        sys.exit("usage: python tests/mir_edges.py --dump")
