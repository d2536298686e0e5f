"""The MIR row builders and the volume rule at their edges, on the CPU: the restatement of tests/mir_edges.py against
the reference's own word (tests/golden/mir_edges.json.gz), the oracle library and the Python volume helpers against the restatement, what
every instance is there for, every defect switch against a named instance, and what the GPU test (tests/test_mir_edges_gpu.py) leans on:
that the oracle's sequence ends on every instance sent through the one-call form, and that a wrong appended row shows behind the simplex.

Every comparison is exact (NaN equals NaN, every other double by its bits).  The one bound is the 2000 pivots of the one-call list.
"""
import gzip
import json
import math
import os

import numpy as np
import pytest

import golden_util as G
import mir_edges as E
from jslpsolver_amd import Tableau, _capi
from jslpsolver_amd.engine import fractional_volume_rows
from test_mir_one_call import by_hand, u64, volume

with gzip.open(os.path.join(G.GOLDEN, "mir_edges.json.gz"), "rt") as _fh:
    GOLDEN = json.load(_fh)
NAMES = [i["name"] for i in E.INSTANCES]
# Through the one-call form (and through mirRound's simplex): every instance but the two of the value family, whose rows hold negative and
# -Infinity right-hand sides among NaN / Infinity cells -- the root's simplex pivots on them (2 pivots) and the state behind it is no longer
# the planted one.  They end on the oracle all the same (test_the_one_call_sequence_ends_on_the_oracle), so they stay in the list; the other
# non-finite instances (volume_nan_row, volume_inf_row, loop_nan) are pre-solved and stay too.  None had to be removed.
ONE_CALL = list(NAMES)
PRESOLVED = [n for n in NAMES if not n.startswith("value_")]
THREADS = (256, 512, 1024)
_restated = {}


def restated(name):
    if name not in _restated:
        _restated[name] = E.restate_instance(E.BY_NAME[name])
    return _restated[name]


def where(r, threads):
    """(chunk, wave, lane) of row r in a scan whose chunks are `threads` rows wide (row r is thread r - 1 of its chunk)"""
    return ((r - 1) // threads, ((r - 1) % threads) >> 6, (r - 1) & 63)


def nan_bits(x):
    """the bits of a double, every NaN as the one canonical NaN (the bits of a NaN depend on the hardware that made it)"""
    x = float(x)
    return E.bits(E.NAN) if x != x else E.bits(x)


def same_node(got, e, prev):
    """test_mir_one_call.same_node -- got = (result, outcome, rhs, vibr) of a one-call node, e = by_hand's dict, prev = the evaluation a node
    none of whose simplexes set it keeps -- with every double compared by its bits except that a NaN equals a NaN: these instances make NaNs
    (Infinity - Infinity, 0 * Infinity), and the sign of a made NaN is the hardware's"""
    res, oc, rhs, vibr = got
    d, x = res.as_dict(), e["res"].as_dict()
    d.pop("evaluation"), x.pop("evaluation")
    for k in d:
        if isinstance(d[k], float):
            d[k], x[k] = nan_bits(d[k]), nan_bits(x[k])
    assert d == x, {k: (d[k], x[k]) for k in d if d[k] != x[k]}
    assert nan_bits(res.evaluation) == nan_bits(e["evaluation"] if e["sets"] else prev)
    assert (int(oc["rounds"]), int(oc["rows_added"]), int(oc["optimal_count"]), int(oc["pivots"])) == e["record"]
    assert nan_bits(oc["volume_before"]) == nan_bits(e["volumes"][0]) and nan_bits(oc["volume_after"]) == nan_bits(e["volumes"][1])
    h = res.height
    assert E.same_doubles(rhs[:h], e["rhs"]) and np.array_equal(vibr[:h], e["vibr"])


# ---- the golden ------------------------------------------------------------------------------------------------------------------------
def test_the_golden_holds_these_instances():
    assert sorted(GOLDEN) == sorted(NAMES)
    for inst in E.INSTANCES:
        assert GOLDEN[inst["name"]]["sha"] == E.sha_input(inst), inst["name"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    inst, g, got = E.BY_NAME[name], GOLDEN[name], restated(name)
    H, W = inst["H"], inst["W"]
    assert len(got["sel"]) == g["n"] <= E.MAX_CUTS
    assert E.same_doubles(got["rows"].reshape(-1), E.from_hex(g["rows"]))  # NaN as "is NaN", every other cell by its bits, -0 included
    assert got["slacks"] == g["vibr"] == list(range(W + H - 2, W + H - 2 + g["n"])) and g["last"] == W + H - 2 + g["n"]
    assert g["rbv"] == list(range(H, H + g["n"])) and g["cbv"] == [-1] * g["n"]
    assert E.same_double(got["volume"], float(E.from_hex(g["volume"])[0]))


# ---- the oracle library and the volume helpers against the restatement --------------------------------------------------------------------
def check_apply_mir_cuts_direct(lib, name):
    """applyMIRCuts() straight after construction: the appended rows cell by cell, the untouched rows, the maps, the count"""
    inst, want = E.BY_NAME[name], restated(name)
    H, W, n = inst["H"], inst["W"], len(want["sel"])
    t = E.make_tableau(lib, inst, extra_rows=n)  # (row_capacity == H + n exactly)
    assert t.applyMIRCuts() == n
    m, vibr, vibc, rbv, cbv = t.download()
    assert m.shape == (H + n, W)
    assert E.same_doubles(m[:H], inst["matrix"])
    for k in range(n):
        assert E.same_doubles(m[H + k], want["rows"][k]), (name, k, want["sel"][k])
    assert vibr[:H].tolist() == inst["vibr"].tolist() and vibr[H:].tolist() == want["slacks"] and vibc.tolist() == inst["vibc"].tolist()
    assert [int(rbv[s]) for s in want["slacks"]] == list(range(H, H + n)) and all(int(cbv[s]) == -1 for s in want["slacks"])
    rhs, rows = t.read_rhs()
    assert E.same_doubles(rhs, m[:, 0]) and rows.tolist() == vibr.tolist()
    t.close()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_apply_mir_cuts(oracle_lib, name):
    check_apply_mir_cuts_direct(oracle_lib, name)


def grown(name, **defect):
    """the instance with the restatement's appended rows: (matrix, vibr)"""
    inst = E.BY_NAME[name]
    r = E.restate_instance(inst, **defect) if defect else restated(name)
    return np.vstack([inst["matrix"], r["rows"]]), np.concatenate([inst["vibr"], np.array(r["slacks"], dtype=np.int32)])


def final_state(t):
    m, vibr, vibc, _, _ = t.download()
    return E.hex_doubles(G.canon_nan(m)), vibr.tolist(), vibc.tolist()


def simplex_of_grown(lib, name, **defect):
    """upload the grown tableau as a new Tableau (upload sets the element counter to W + H - 2 of the GROWN height: the slack indexes line
    up) and run simplex(): round 1 without the library's MIR code"""
    inst = E.BY_NAME[name]
    m, vibr = grown(name, **defect)
    t = Tableau(m, vibr, inst["vibc"], precision=inst["precision"], row_capacity=m.shape[0], lib=lib, integer_variables=inst["ints"])
    res = t.simplex(check_cycles=True)
    out = (final_state(t), res.pivots_phase1, res.pivots_phase2, bool(res.feasible), bool(res.optimal), bool(res.bounded))
    t.close()
    return out


def check_mir_round(lib, oracle_lib, name):
    """mirRound() straight after construction: the count is the restatement's, and what stands behind its simplex is what the simplex of the
    restatement's grown tableau leaves (computed on the oracle library, without any MIR code but the restatement)"""
    inst, want = E.BY_NAME[name], restated(name)
    t = E.make_tableau(lib, inst, extra_rows=len(want["sel"]))
    n, res, rhs, vibr = t.mirRound(check_cycles=True)
    got = (final_state(t), res.pivots_phase1, res.pivots_phase2, bool(res.feasible), bool(res.optimal), bool(res.bounded))
    m = t.download()[0]
    assert n == len(want["sel"]) and E.same_doubles(rhs, m[:, 0]) and vibr.tolist() == t.download()[1].tolist()
    t.close()
    assert got == simplex_of_grown(oracle_lib, name)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_mir_round(oracle_lib, name):
    check_mir_round(oracle_lib, oracle_lib, name)


@pytest.mark.parametrize("name", NAMES)
def test_volume_helpers(name):
    inst, want = E.BY_NAME[name], restated(name)
    ints = set(inst["ints"])
    rhs = inst["matrix"][:, 0]
    assert E.same_double(fractional_volume_rows(ints, rhs, inst["vibr"], inst["precision"]), want["volume"])
    assert E.same_double(volume(ints, rhs, inst["vibr"], inst["precision"]), want["volume"])


# ---- every instance does what it is there for --------------------------------------------------------------------------------------------
def test_scan_instances():
    turns = E.BY_NAME["scan_turns"]
    sel = restated("scan_turns")["sel"]
    assert sel == turns["candidates"] == [3, 64, 65, 256, 257, 512, 513, 1024, 1025, 1039] and sel[-1] == turns["H"] - 1
    assert [where(r, 256)[0] for r in sel] == [0, 0, 0, 0, 1, 1, 2, 3, 4, 4]
    assert [where(r, 512)[0] for r in sel] == [0, 0, 0, 0, 0, 0, 1, 1, 2, 2]
    assert [where(r, 1024)[0] for r in sel] == [0] * 8 + [1, 1]
    assert where(64, 256)[1:] == (0, 63) and where(65, 256)[1:] == (1, 0)  # the two sides of a wave turn
    for threads in THREADS:  # the last thread of a chunk and the first of the next, in every build
        assert where(threads, threads) == (0, threads // 64 - 1, 63) and where(threads + 1, threads) == (1, 0, 0)
        assert threads in sel and threads + 1 in sel
    tenth = E.BY_NAME["scan_tenth_opens_a_chunk"]
    sel = restated("scan_tenth_opens_a_chunk")["sel"]
    assert len(tenth["candidates"]) == 11 and sel == tenth["candidates"][:10] and tenth["candidates"][10] == 1026
    assert all(r <= 1024 for r in sel[:9]) and sel[9] == 1025
    for threads in THREADS:  # the tenth cut is thread 0 of a later chunk in every build, the eleventh candidate sits right behind it
        assert where(1025, threads)[0] > 0 and where(1025, threads)[1:] == (0, 0) and where(1026, threads)[0] == where(1025, threads)[0]
    early = E.BY_NAME["scan_early_exit"]
    assert restated("scan_early_exit")["sel"] == list(range(1, 11)) and len(early["candidates"]) == 750
    assert all(where(r, 256)[0] == 0 for r in range(1, 11))  # ten in the first chunk of every build: the scan need not take a second turn
    past = E.BY_NAME["scan_past_the_cap"]
    assert restated("scan_past_the_cap")["sel"] == list(range(250, 260))
    for threads, in_chunk in ((256, 1), (512, 0), (1024, 0)):  # the chunk that holds the tenth cut holds hundreds of candidates behind it
        c = where(259, threads)[0]
        assert c == in_chunk and sum(1 for r in past["candidates"] if where(r, threads)[0] == c) > 200
    assert where(256, 256)[0] == 0 and where(257, 256)[0] == 1  # ... and with 256 threads the ten straddle a chunk turn
    assert restated("scan_all")["sel"] == list(range(1, 11)) and len(E.BY_NAME["scan_all"]["candidates"]) == 1039
    none = restated("scan_none")
    assert none["sel"] == [] and none["rows"].shape == (0, E.SCAN_W) and E.same_double(none["volume"], 0.0)
    assert restated("scan_one_row")["sel"] == [1] and E.BY_NAME["scan_one_row"]["H"] == 2
    assert restated("scan_66")["sel"] == [1, 2, 33, 64, 65] and E.BY_NAME["scan_66"]["H"] == 66
    # which instances drop candidates
    drops = sorted(i["name"] for i in E.INSTANCES if i["family"] == "scan" and len(i["candidates"]) > E.MAX_CUTS)
    assert drops == ["scan_all", "scan_early_exit", "scan_past_the_cap", "scan_tenth_opens_a_chunk"]
    # every candidate row of the exact instances has a fraction of its own: a wrong pick or a wrong order changes the rows, not only the count
    for name in ("scan_turns", "scan_tenth_opens_a_chunk", "scan_66"):
        inst = E.BY_NAME[name]
        fr = [inst["matrix"][r, 0] - math.floor(inst["matrix"][r, 0]) for r in inst["candidates"]]
        assert len(set(fr)) == len(fr)
    # the decoys are there: integer variables at (nearly) integer values and continuous variables at fractions, in every chunk
    inst = E.BY_NAME["scan_turns"]
    ints = set(inst["ints"])
    for c in range(5):
        rows = [r for r in range(1, inst["H"]) if where(r, 256)[0] == c and r not in inst["candidates"]]
        assert any(int(inst["vibr"][r]) not in ints and inst["matrix"][r, 0] % 1 > 0.001 for r in rows)
        assert any(int(inst["vibr"][r]) in ints and 0 < inst["matrix"][r, 0] % 1 < 1e-8 for r in rows)


def arms(inst):
    """which arm of js_max0 / js_min0 every planted cell of a cut row with a finite fraction takes: {(kind, label): arm}"""
    ints = set(inst["ints"])
    out = {}
    for (r, c), label in inst["planted"].items():
        rhs = float(inst["matrix"][r, 0])
        f = rhs - E.js_floor(rhs)
        if f != f:
            continue
        a = float(inst["matrix"][r, c])
        if int(inst["vibc"][c]) in ints:
            x = a - E.js_floor(a) - f
            arm = "nan" if x != x else ("positive" if x > 0 else ("zero" if x == 0 else "negative"))
            out.setdefault(("int", label), set()).add(arm)
        else:
            q = a / (1 - f)
            arm = "nan" if q != q else ("negative" if q < 0 else ("neg_zero" if E.neg_zero(q) else ("zero" if q == 0 else "positive")))
            out.setdefault(("cont", label), set()).add(arm)
    return out


@pytest.mark.parametrize("name", ["value_1e-8", "value_quarter"])
def test_value_instances(name):
    inst, got = E.BY_NAME[name], restated(name)
    p = inst["precision"]
    assert got["sel"] == [r for r, _, cuts in inst["rhs_rows"] if cuts] and len(got["sel"]) == 9
    rhs = {label: float(inst["matrix"][r, 0]) for r, label, _ in inst["rhs_rows"]}
    assert rhs["f_eq_precision"] - math.floor(rhs["f_eq_precision"]) == p  # a cut: f < precision is false
    assert math.nextafter(rhs["f_ulp_below_precision"], 1.0) == p
    f = rhs["f_eq_one_minus_precision"] - math.floor(rhs["f_eq_one_minus_precision"])
    assert f == 1 - p and 1 - f <= p * (1 + 1e-7)  # a cut: f > 1 - precision is false; 1 - f as small as the threshold allows
    assert math.nextafter(rhs["f_ulp_above_one_minus_precision"], 0.0) == 1 - p
    assert rhs["two_52_plus_half"] == 2.0 ** 52 and rhs["two_51_plus_half"] - 2.0 ** 51 == 0.5  # (2^52 + 0.5 is not a double: an integer, no cut)
    assert E.neg_zero(rhs["neg_zero"]) and rhs["negative"] == -2.75 and rhs["nan"] != rhs["nan"] and rhs["inf"] == E.INF and rhs["neg_inf"] == -E.INF
    if p == 0.25:
        assert rhs["negative"] - math.floor(rhs["negative"]) == p  # f == precision once more, from a negative right-hand side
    # NaN and infinite right-hand sides cut, and every cell of their rows is NaN
    for r, label, _ in inst["rhs_rows"]:
        if label in ("nan", "inf", "neg_inf"):
            assert np.isnan(got["rows"][got["sel"].index(r)]).all()
    # every planted value under an integer and under a continuous column, in rows with a finite fraction; every arm is taken
    a = arms(inst)
    labels = [label for label, _ in E.value_cells(0.5)]
    assert sorted(a) == sorted((kind, label) for kind in ("int", "cont") for label in labels)
    assert a[("int", "frac_below")] == {"negative"} and a[("int", "frac_equal")] == {"zero"} and a[("int", "frac_above")] == {"positive"}
    assert a[("int", "nan")] == a[("int", "inf")] == a[("int", "neg_inf")] == {"nan"} and "negative" in a[("int", "zero")] | a[("int", "neg_zero")]
    assert a[("cont", "nan")] == {"nan"} and a[("cont", "neg_zero")] == {"neg_zero"} and a[("cont", "zero")] == {"zero"}
    assert a[("cont", "neg_three")] == a[("cont", "neg_frac")] == a[("cont", "neg_inf")] == {"negative"}
    assert a[("cont", "three")] == a[("cont", "inf")] == a[("cont", "subnormal")] == a[("cont", "e300")] == {"positive"}
    # the cells of the rows with a NaN fraction under a continuous column: Math.min(0, NaN) is NaN, C's fmin gives 0
    ints = set(inst["ints"])
    assert any(int(inst["vibc"][c]) not in ints for (r, c) in inst["planted"] if r in (9, 10, 11))
    assert inst["H"] * inst["W"] == 24 * 20 and E.leading_dimension(inst["W"]) == 32
    assert sum(1 for c in range(1, inst["W"]) if int(inst["vibc"][c]) in ints) == 10  # half the columns are integer


@pytest.mark.parametrize("W", E.WIDTHS)
def test_width_instances(W):
    inst, got = E.BY_NAME["width_%d" % W], restated("width_%d" % W)
    ints = set(inst["ints"])
    assert got["sel"] == list(E.WIDTH_CANDIDATES) and inst["H"] == 12
    cols = inst["turn_cols"]
    assert cols == sorted(set(c for c in E.WIDTH_COLS if c < W) | {W - 1})
    if W == 16:
        assert E.leading_dimension(W) == W  # no padding column
    else:
        assert E.leading_dimension(W) > W
    if W == 1026:
        assert cols == [1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
        for turn in (256, 512, 1024):  # both sides of every column turn, and both kinds of column around them
            kinds = set(int(inst["vibc"][c]) in ints for c in (turn - 1, turn, turn + 1))
            assert kinds == {True, False}
        # the LDS state still fits the 64 KiB the LDS kernels are launched with, at the capacity the one-call runs use
        assert E.wglds_bytes(E.leading_dimension(W), inst["H"] + E.ONE_CALL_EXTRA_ROWS) <= 64 * 1024
    for r in E.WIDTH_CANDIDATES:  # distinct non-trivial cells, and appended cells that differ from column to column
        cells = [float(inst["matrix"][r, c]) for c in cols]
        assert len(set(cells)) == len(cells) and all(x != 0 and x != math.floor(x) for x in cells)
    for k in range(len(got["sel"])):
        assert np.isfinite(got["rows"][k]).all() and (W < 258 or len(set(got["rows"][k, cols].tolist())) > len(cols) // 2)


def test_volume_instances():
    prod = E.BY_NAME["volume_product"]
    rows = sorted(prod["values"])
    contributing = [r for r in rows if prod["values"][r] != math.floor(prod["values"][r])]
    assert len(rows) == 259 and len(contributing) == 239  # (every thirteenth value is 7/7)
    for turn in (256, 512, 1024):  # contributing rows on both sides of the chunk turns at rows 257 / 513 / 1025
        assert any(turn - 14 < r <= turn for r in contributing) and any(turn < r <= turn + 14 for r in contributing), turn
    v = restated("volume_product")["volume"]
    assert math.isfinite(v) and v > 0
    # the ordered product differs in its bits from the pairwise product and from every per-chunk product: asserted here, on the CPU
    args = (prod["matrix"][:, 0], prod["vibr"], prod["ints"], prod["precision"])
    assert not E.same_double(E.restate_volume(*args, pairwise=True), v)
    for threads in THREADS:
        assert not E.same_double(E.restate_volume(*args, threads=threads, per_chunk=True), v), threads
    neg = E.BY_NAME["volume_negative_rows"]
    assert sum(1 for x in neg["values"].values() if x < 0) >= 10 and neg["values"][7] == -2.75
    assert min(neg["matrix"][1:, 0]) == -2.75 and (neg["matrix"][neg["blocked"], 1:] >= 0).all()  # phase 1 picks a blocked row: no pivot
    assert restated("volume_negative_rows")["volume"] > 0
    near = E.BY_NAME["volume_near_integer"]
    # within the precision ABOVE an integer: no factor; within the precision BELOW one: a factor (Math.floor(distance + 1) is no distance)
    want = (6.0 - 5e-9) * 1.5 * (3.0 - 5e-9) * 2.25
    assert E.same_double(restated("volume_near_integer")["volume"], want) and near["values"][10] == 4.0 + 5e-9
    assert math.isnan(restated("volume_nan_row")["volume"]) and restated("volume_inf_row")["volume"] == E.INF
    over = E.BY_NAME["volume_overflow"]
    assert restated("volume_overflow")["volume"] == E.INF and all(math.isfinite(x) for x in over["values"].values())
    assert E.same_double(restated("volume_none")["volume"], 0.0) and len(E.BY_NAME["volume_none"]["values"]) > 300


# ---- the defect switches -------------------------------------------------------------------------------------------------------------------
WITNESS = {  # switch -> instances whose observable it must change (the scan defects: at every chunk width)
    "wave_rank": ["scan_turns", "scan_66"],
    "chunk_rank": ["scan_turns"],
    "cap_per_chunk": ["scan_tenth_opens_a_chunk", "scan_all"],
    "first_chunk_only": ["scan_turns", "scan_tenth_opens_a_chunk"],
    "threshold_le_ge": ["value_1e-8", "value_quarter"],
    "c_minmax": ["value_1e-8", "value_quarter"],
    "reciprocal": ["scan_turns", "width_16", "width_1026", "value_1e-8"],
    "pairwise": ["volume_product"],
    "per_chunk": ["volume_product"],
    "no_abs": ["volume_negative_rows"],
    "skip_nan": ["volume_nan_row", "value_1e-8", "loop_nan"],
}


def observable(r):
    return ([-1 if s is None else s for s in r["sel"]], E.hex_doubles(G.canon_nan(r["rows"])), r["slacks"], E.hex_doubles(G.canon_nan([r["volume"]])))


@pytest.mark.parametrize("switch", [d for d in E.DEFECTS if d not in E.UNOBSERVABLE])
def test_defect_switch_changes_a_named_instance(switch):
    for name in WITNESS[switch]:
        for threads in (THREADS if switch in E.SCAN_DEFECTS or switch == "per_chunk" else (256,)):
            good = E.restate_instance(E.BY_NAME[name], threads=threads)
            bad = E.restate_instance(E.BY_NAME[name], threads=threads, **{switch: True})
            assert observable(good) == observable(restated(name))  # the chunk width is no input of a correct scan
            assert observable(bad) != observable(good), (switch, name, threads)


def test_every_switch_is_accounted_for():
    assert set(WITNESS) | set(E.UNOBSERVABLE) == set(E.DEFECTS) and not set(WITNESS) & set(E.UNOBSERVABLE)


def test_unobservable_switches_change_no_instance_and_no_special_value():
    """the two switches arithmetic hides (mir_edges.UNOBSERVABLE says why): no instance shows them, and neither does a sweep of every special
    cell value under every fraction the value family uses"""
    for switch in E.UNOBSERVABLE:
        for inst in E.INSTANCES:
            assert observable(E.restate_instance(inst, **{switch: True})) == observable(restated(inst["name"])), (switch, inst["name"])
    cells = [x for _, x in E.value_cells(0.3125)] + [-5e-324, -1e-300, 1e-300, -2.0 ** 53, -1e300, 0.3125, -0.3125]
    for f in (1e-8, 0.25, 0.3125, 0.5, 0.75, 1 - 1e-8, E.NAN):
        for a in cells:
            q = a / (1 - f)
            mn = E.js_min(0.0, q)
            assert E.same_double(mn - a, (0.0 if E.neg_zero(mn) else mn) - a)
    for rhs in (1e-8, 0.25, -2.75, 7.3125, 2.0 ** 51 + 0.5, 1 - 1e-8, E.NAN, E.INF, -E.INF, 5e-324, -5e-324):
        f = rhs - E.js_floor(rhs)
        if not (f < 1e-8 or f > 1 - 1e-8):
            assert E.same_double(E.js_floor(rhs) - rhs, -f)


def test_js_max0_nan_arm_cannot_show():
    """the NaN arm of Math.max(0, x) in an integer column is kept as the reference has it, but no appended cell can tell it from C's fmax:
    x = a - floor(a) - f is NaN only for a NaN or infinite a, or a NaN f, and then floor(a) + ... - a is NaN whatever max gave.  (Math.min's
    NaN arm does show: the continuous cells of a row with a NaN fraction -- the c_minmax witness.)"""
    for f in (0.25, 0.5, E.NAN):
        for a in (E.NAN, E.INF, -E.INF, 1.5):
            fl = E.js_floor(a)
            x = a - fl - f
            if x != x:
                assert math.isnan(fl + E.js_max(0.0, x) / (1 - f) - a) and math.isnan(fl + E.c_fmax(0.0, x) / (1 - f) - a)


# ---- what the GPU test leans on ------------------------------------------------------------------------------------------------------------
_expect = {}


def expectation(oracle_lib, name):
    """the oracle's sequence (test_mir_one_call.by_hand) of every node of the instance: (root result, root evaluation, [per node: by_hand's dict
    + the live tableau and the node's part of the pivot trace])"""
    if name not in _expect:
        inst = E.BY_NAME[name]
        rounds = E.rounds_of(inst)
        t, root = E.root_tableau(oracle_lib, inst, E.ONE_CALL_EXTRA_ROWS)
        root_eval = t.evaluation
        out = []
        for cuts in E.nodes_of(inst):
            trace0 = len(t.pivot_trace())
            e = by_hand(t, set(inst["ints"]), cuts, -1 if rounds is None else rounds, False)
            e["state"] = final_state(t)
            e["trace"] = t.pivot_trace()[trace0:].copy()
            out.append(e)
        t.close()
        _expect[name] = (root, root_eval, out)
    return _expect[name]


@pytest.mark.parametrize("name", ONE_CALL)
def test_the_one_call_sequence_ends_on_the_oracle(oracle_lib, name):
    root, _, ex = expectation(oracle_lib, name)
    assert sum(e["record"][3] for e in ex) + root.pivots_phase1 + max(root.pivots_phase2, 0) < 2000
    if name in PRESOLVED:  # zero pivots at the root: the first node's loop sees exactly what was planted
        assert root.pivots_phase1 == 0 and root.pivots_phase2 in (0, -1)
        first = ex[0]
        assert first["record"][0] >= 1 and first["per_round"][0][1] == len(restated(name)["sel"])
        assert E.same_double(first["volumes"][0] if first["record"][0] == 1 else restated(name)["volume"], restated(name)["volume"])
    assert all(e["record"][0] >= 1 for e in ex)


@pytest.mark.parametrize("name", ["scan_none", "volume_none"])
def test_no_candidate_stops_after_one_round(oracle_lib, name):
    e = expectation(oracle_lib, name)[2][0]
    assert e["record"][:2] == (1, 0) and u64(e["volumes"][0])[()] == 0 and u64(e["volumes"][1])[()] == 0  # 0 >= 0.9 * 0


@pytest.mark.parametrize("name", PRESOLVED)
def test_round_one_without_the_oracles_mir_code(oracle_lib, name):
    """by_hand(max_rounds = 1) of the root's node [] leaves what simplex() leaves of the restatement's grown tableau; with one defect switched
    on the final tableau changes: the post-simplex observable of the GPU test sees a wrong appended row"""
    inst = E.BY_NAME[name]
    t, _ = E.root_tableau(oracle_lib, inst, E.ONE_CALL_EXTRA_ROWS)
    e = by_hand(t, set(inst["ints"]), [], 1, False)
    state = final_state(t)
    m = t.download()[0]
    t.close()
    want = simplex_of_grown(oracle_lib, name)
    assert state == want[0] and E.same_doubles(e["rhs"], m[:, 0]) and e["vibr"].tolist() == state[1]
    assert (e["res"].pivots_phase1, e["res"].pivots_phase2, bool(e["res"].feasible), bool(e["res"].optimal)) == want[1:5]


@pytest.mark.parametrize("name,switch", [("scan_turns", "first_chunk_only"), ("scan_turns", "reciprocal"), ("scan_tenth_opens_a_chunk", "cap_per_chunk"),
                                         ("width_1026", "reciprocal"), ("value_quarter", "threshold_le_ge")])
def test_a_wrong_row_shows_behind_the_simplex(oracle_lib, name, switch):
    bad = E.restate_instance(E.BY_NAME[name], **{switch: True})
    assert None not in bad["sel"]
    inst = E.BY_NAME[name]
    m = np.vstack([inst["matrix"], bad["rows"]])
    vibr = np.concatenate([inst["vibr"], np.array(bad["slacks"], dtype=np.int32)])
    t = Tableau(m, vibr, inst["vibc"], precision=inst["precision"], row_capacity=m.shape[0], lib=oracle_lib, integer_variables=inst["ints"])
    t.simplex(check_cycles=True)
    assert final_state(t) != simplex_of_grown(oracle_lib, name)[0]
    t.close()


# ---- capacity and the round limit (shared with the GPU test) ---------------------------------------------------------------------------------
def plain_node(oracle_lib, inst, cuts, extra_rows):
    t, _ = E.root_tableau(oracle_lib, inst, extra_rows)
    want = t.applyCuts(cuts)
    out = (want[0].as_dict(), want[1].copy(), want[2].copy())
    t.close()
    return out


def usable_again(t, want, cuts):
    """after a refusal: restore() and a plain applyCuts equal the oracle's"""
    t.restore()
    got = t.applyCuts(cuts)
    assert got[0].as_dict() == want[0] and np.array_equal(u64(got[1]), u64(want[1])) and np.array_equal(got[2], want[2])


def check_capacity(lib, oracle_lib, batch):
    """row_capacity == H + n exactly: the call fits and is right; H + n - 1: JSLP_ERR_CAPACITY, and the engine is usable again; for the
    one-call form also a capacity that holds round 1's rows and not round 2's"""
    capacity = r"\(%d\)" % _capi.JSLP_ERR_CAPACITY
    for name in ("scan_66", "scan_tenth_opens_a_chunk"):
        inst, want = E.BY_NAME[name], restated(name)
        n = len(want["sel"])
        check_apply_mir_cuts_direct(lib, name)  # (row_capacity == H + n)
        want_plain = plain_node(oracle_lib, inst, [], n - 1)
        t, _ = E.root_tableau(lib, inst, n - 1)
        for call in (t.applyMIRCuts, t.mirRound):
            with pytest.raises(_capi.EngineError, match=capacity):
                call()
            usable_again(t, want_plain, [])
        t.close()
    # the one-call form: width_16's last node runs two rounds (9 rows, then 8) behind one branching cut
    inst = E.BY_NAME["width_16"]
    cuts = E.nodes_of(inst)[4]
    _, root_eval, ex = expectation(oracle_lib, "width_16")
    e = ex[4]
    assert [n for _, n in e["per_round"]] == [9, 8] and e["record"][:2] == (2, 17)
    fits = inst["H"] + len(cuts) + 17 - inst["H"]
    for extra, ok in ((fits, True), (fits - 1, False), (len(cuts) + 9, False), (len(cuts) + 8, False)):
        want_plain = plain_node(oracle_lib, inst, cuts, extra)
        t, _ = E.root_tableau(lib, inst, extra)
        if batch:
            t.applyCutsBatch([cuts] * 3)  # (three slots in sync with the saved root: the calls below are the one-launch shapes)
        if ok:
            same_node(t.applyCutsMIR(cuts), e, t.evaluation)
        else:
            with pytest.raises(_capi.EngineError, match=capacity):
                t.applyCutsMIR(cuts)
        usable_again(t, want_plain, cuts)
        if batch:
            if ok:
                prev = t.evaluation
                results, ocs, rhs, vibr = t.applyCutsBatchMIR([cuts, [], cuts])
                for i, j in ((0, 4), (1, 0), (2, 4)):
                    same_node((results[i], ocs[i], rhs[i], vibr[i]), ex[j], prev)
            else:
                with pytest.raises(_capi.EngineError, match=capacity):
                    t.applyCutsBatchMIR([cuts, [], cuts])
            usable_again(t, want_plain, cuts)
            r, x, w = t.applyCutsBatch([cuts] * 3)  # the calls after a refused batch (tests/test_mir_one_call_gpu.py::test_errors)
            for i in range(3):
                h = r[i].height
                a = r[i].as_dict()
                b = dict(want_plain[0])
                a.pop("evaluation"), b.pop("evaluation")
                assert a == b and np.array_equal(u64(x[i, :h]), u64(want_plain[1])) and np.array_equal(w[i, :h], want_plain[2])
        t.close()


def test_capacity_on_the_oracle(oracle_lib):
    check_capacity(oracle_lib, oracle_lib, batch=True)


LOOP_EXTRA_ROWS = 2 + 10 * _capi.JSLPR_MAX_ROUNDS  # up to ten rows a round


def check_round_limit(lib, oracle_lib, batch):
    """a NaN right-hand side in an integer row: the volume is NaN on every round, the rule never stops the loop.  max_rounds = 63 and 64 end
    after exactly that many rounds without an error; the unbounded loop ends in JSLP_ERR_CAPACITY with the JSLPR_MAX_ROUNDS text;
    max_rounds = 0 makes zero rounds and leaves both volumes 0.0"""
    assert _capi.JSLPR_MAX_ROUNDS == 64
    inst = E.BY_NAME["loop_nan"]
    nodes = E.nodes_of(inst)[:3]
    ref, _ = E.root_tableau(oracle_lib, inst, LOOP_EXTRA_ROWS)
    root_eval = ref.evaluation
    want = {rounds: [by_hand(ref, set(inst["ints"]), cuts, rounds, False) for cuts in nodes] for rounds in (0, 63, 64)}
    want_plain = ref.applyCuts(nodes[2])
    want_plain = (want_plain[0].as_dict(), want_plain[1].copy(), want_plain[2].copy())
    ref.close()
    for rounds in (63, 64):
        assert [e["record"][0] for e in want[rounds]] == [rounds] * 3 and all(math.isnan(v) for e in want[rounds] for v in e["volumes"])
        assert want[rounds][0]["record"][1] == 3 * rounds and want[rounds][2]["record"][1] > 9 * rounds  # three rows a round; nearly ten behind a pivot
    assert [e["record"][:2] for e in want[0]] == [(0, 0)] * 3 and all(u64(v)[()] == 0 for e in want[0] for v in e["volumes"])
    t, _ = E.root_tableau(lib, inst, LOOP_EXTRA_ROWS)
    if batch:
        t.applyCutsBatch(nodes)
    for rounds in (0, 63, 64):
        prev = t.evaluation
        for cuts, e in zip(nodes, want[rounds]):
            got = t.applyCutsMIR(cuts, max_rounds=rounds)
            same_node(got, e, prev)
            prev = got[0].evaluation
        if batch:
            t.restore()
            results, ocs, rhs, vibr = t.applyCutsBatchMIR(nodes, max_rounds=rounds)
            for i, e in enumerate(want[rounds]):
                same_node((results[i], ocs[i], rhs[i], vibr[i]), e, prev)
    calls = [lambda: t.applyCutsMIR(nodes[0]), lambda: t.applyCutsMIR(nodes[2])]
    if batch:
        calls.append(lambda: t.applyCutsBatchMIR(nodes))
    for call in calls:
        with pytest.raises(_capi.EngineError, match=r"\(%d\).*JSLPR_MAX_ROUNDS" % _capi.JSLP_ERR_CAPACITY):
            call()
        usable_again(t, want_plain, nodes[2])
    t.close()


def test_round_limit_on_the_oracle(oracle_lib):
    check_round_limit(oracle_lib, oracle_lib, batch=True)
