"""The branch-and-bound NODE (restore + addCutConstraints + simplex + read-back: one unit of jslp_engine_relax*) at the shape, cut and
error edges of its kernels, on every launch shape the dispatcher (relax_batch_impl) has for it, HIP against the CPU oracle bit for bit.

Roots are synthetic and integer-valued (the generator of test_edge_cases.test_hip_equals_oracle_beyond_the_register_resident_sizes:
costs 1..29, entries 1..8 at a density, right-hand sides 50..399, every other one plus 0.5), solved, save()d and read once on the oracle;
the node family of a root is chosen from that read (family()).  The oracle evaluates every node alone -- restore(), applyCuts(cuts) --
and the outcome of every node of every call on the GPU must be that outcome: feasible, bounded, optimal, height, both pivot counts,
the cycle flag, the evaluation's bits and the bytes of the RHS column and of the row map up to the height; the compact read-back and the
branch records are derived from the same outcome.  A node without an optimum reports the evaluation its CALL started from (fill_result),
which the worker tracks.  No tolerance anywhere.

The GPU part runs in tests/node_edges_worker.py, one subprocess per setting of the JSLP_* knobs (most are read once per process), on one
engine per root, the calls back to back so that each starts from what the last left in the slots.  With JSLP_DEBUG_LAUNCH=1 the engine
names the node kernel of every launch; the worker restates the dispatcher's choice (Dispatch) and asserts each call's lines, so a case
that silently took another path fails.

Shapes (rows x columns of the root with row 0 / column 0; spare = row_capacity - height):
  tiny                    2 x 2, 2 x 17, 7 x 6
  ld, W against the 64-lane x 4 pair copy of add_cuts_waves
                          15 rows x 16, 17, 113, 127, 128, 129, 143, 144, 511, 512, 513, 527, 528, 1023, 1024, 1025, 1040 columns
  H against blockDim and 2 x blockDim (preload of node_lds_run, compact gather)
                          511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049 rows x 15 columns
  LDS fit, both sides     2590 x 15 with row_capacity 2608 (k_node_lds) and 2610 (k_node_wg); 15 x 1040 with row_capacity 1788 and 1790
  out_stride modulo 4     41 x 15 with row_capacity 44, 45, 46, 47
  more dirty rows than k_node_wg's list holds (density 1: a pivot writes every row; proven by the engine's restored_rows counter)
                          2700 x 15, row_capacity 2720: a batch on k_node_wg<512,2048>  (oracle: root + 35 nodes in 0.04 s)
                          4200 x 15, row_capacity 4220: single nodes on k_node_wg<1024,4096>  (oracle: 0.05 s)
  cell limits             15 x 1040 with row_capacity 1788 / 1790: 1.86 M cells, between the single-child limit (1.5 M: a node alone runs on the
                          chip-wide path) and the batch limit (4 M: batches keep their one-workgroup kernels); 15 x 1040 with row_capacity 4100:
                          4.26 M cells, every node chip-wide, one after the other  (oracle: 0.08 s)
Every root also with an unrestricted structural variable ("+unr", not the 2-row and the large ones), the small ones with two optional
objective rows ("+opt").  The defaults run every root; JSLP_NODE_COW=0 and JSLP_NO_WGLDS=1 every root but the "+unr" twins of the ld and
H families; the other settings every tiny and out_stride root and the mid-size roots of THIN (JSLP_NO_NODE_KERNEL=1 and
JSLP_WG_BATCH_THREADS=256, where every node goes through k_add_cuts / k_simplex_* / k_gather, the whole ld row too); the large roots run
under the first three settings only.  Per root: every node alone (after restore() and without, twice; compact once), the family cut
into batches of 2, 8, 16, 17 and all of it, each batch twice in each read-back, and the family 30 times over (more where that is fewer
nodes than the queue kernel has resident workgroups), whose repetitions are compared with the first one array-wise.

Errors: the element-index capacity cannot overflow while the rows fit -- n_idx = width + 2 * row_capacity + 2 and the next index after
`spare` cuts is width + row_capacity - 2 -- so that case is unreachable through the ABI and absent; the other three are here.
A cut on the slack variable that an EARLIER cut of the same list created is not in the families either: the reference never builds one.

GPU time of this module on an MI355X: 67 s (22 tests) on a box where the same tests before the settings were thinned took 115 s; those took
171 s inside a full `-m gpu` run of 628 s on another, slower box, which leaves 457 s for the parent's suite there: the module is 22 % of the
parent's wall time on either box's scale (the bound is a quarter).  The whole CPU plan of the oracle takes 1.2 s.
"""
import math
import os
import pickle
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from jslpsolver_amd import _capi
from jslpsolver_amd.engine import Tableau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "node_edges_worker.py")
KNOBS = ("JSLP_FORCE_PATH", "JSLP_NODE_COW", "JSLP_NODE_COW_SMALL", "JSLP_NODE_COW_SINGLE", "JSLP_NODE_QUEUE", "JSLP_SNAPSHOT_TRANSPOSE",
         "JSLP_ZERO_COPY", "JSLP_BATCH_POLL", "JSLP_NO_WGLDS", "JSLP_NO_NODE_KERNEL", "JSLP_WG_BATCH_THREADS", "JSLP_SMALL_BATCH_1024",
         "JSLP_GROUP_MAX", "JSLP_WG_CELLS_CHILD", "JSLP_NODE_QUEUE_ORDER_FULL", "JSLP_DEBUG_STALL", "JSLP_XL", "JSLP_NO_RESIDENT")
WGLDS_MAX_BYTES = 64 * 1024
ERR_CODE = re.compile(r"failed \((-?\d+)\)")
SPARE = 70  # row_capacity - height where the shape does not say otherwise: room for the 65-cut list


def wglds_bytes(ld, cap_rows):
    """jslp_wglds.hip.h: dynamic LDS of the LDS-resident node kernels"""
    hc = (cap_rows + 1) & ~1
    return 8 * (2 * ld + 2 * hc) + 4 * hc + 4 * hc + 4 * ld + hc


def largest_cap_that_fits(ld):
    cap = 2
    while wglds_bytes(ld, cap + 2) <= WGLDS_MAX_BYTES:
        cap += 2
    return cap


# ---- roots ------------------------------------------------------------------------------------------------------------------------
def make_root(rows, cols, seed, density=0.6):
    m, n = rows - 1, cols - 1
    rng = np.random.default_rng(seed)
    A = np.zeros((m + 1, n + 1))
    A[1:, 1:] = rng.integers(1, 9, (m, n)) * (rng.random((m, n)) < density)
    A[0, 1:] = rng.integers(1, 30, n)
    rhs = rng.integers(50, 400, m).astype(np.float64)
    rhs[::2] += 0.5  # fractional basic values at the optimum
    A[1:, 0] = rhs
    vibr = np.concatenate(([-1], np.arange(m))).astype(np.int32)  # slack i on row i + 1
    vibc = np.concatenate(([-1], m + np.arange(n))).astype(np.int32)  # structural variable m + j on column j + 1
    return A, vibr, vibc


def _shape_list():
    """(name, rows, cols, row_capacity, has +opt variant, thin)"""
    out = [("tiny 2x2", 2, 2, 2 + SPARE, True), ("tiny 2x17", 2, 17, 2 + SPARE, True), ("tiny 7x6", 7, 6, 7 + SPARE, True)]
    for w in (16, 17, 113, 127, 128, 129, 143, 144, 511, 512, 513, 527, 528, 1023, 1024, 1025, 1040):
        out.append(("ld 15x%d" % w, 15, w, 15 + SPARE, w in (16, 129, 1040)))
    for h in (511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049):
        out.append(("H %dx15" % h, h, 15, h + SPARE, h == 513))
    out.append(("fit 2590x15 cap 2608", 2590, 15, 2608, False))
    out.append(("fit 2590x15 cap 2610", 2590, 15, 2610, False))
    cap = largest_cap_that_fits(1040)
    out.append(("fit 15x1040 cap %d" % cap, 15, 1040, cap, False))
    out.append(("fit 15x1040 cap %d" % (cap + 2), 15, 1040, cap + 2, False))
    for c in (44, 45, 46, 47):
        out.append(("stride 41x15 cap %d" % c, 41, 15, c, c == 45))
    return out


# the mid-size roots every setting runs; the other settings (THIN_SETTINGS) run these and every tiny and out_stride root (thin_roots())
THIN = ("ld 15x129+unr", "ld 15x1040", "H 513x15+opt", "H 2049x15", "fit 2590x15 cap 2610")
ERROR_ROOTS = ("tiny 7x6", "stride 41x15 cap 45", "H 513x15+opt")


def thin_roots(setting):
    """the tiny and the out_stride roots under every setting, the mid-size ones of THIN; where the node goes through several launches
    whatever the call (k_add_cuts, k_simplex_*, k_gather instead of the node kernels) the whole ld row too"""
    names = [s["name"] for s in root_specs() if s["name"].startswith(("tiny", "stride")) or s["name"] in THIN]
    if setting in ("nonodekernel", "threads256"):
        names += [s["name"] for s in root_specs() if s["name"].startswith("ld ") and "+" not in s["name"] and s["name"] not in names]
    return names


def most_roots():
    """every root but the "+unr" twins of the ld and H families (those run under the defaults): what JSLP_NODE_COW=0 and JSLP_NO_WGLDS=1 run"""
    return [s["name"] for s in root_specs() if not (s["unr"] and s["name"].startswith(("ld ", "H ")) and s["name"] not in THIN)]


# (name, rows, cols, row_capacity, density): sized on the CPU oracle, see the docstring
LARGE = (("dirty 2700x15", 2700, 15, 2720, 1.0), ("dirty 4200x15", 4200, 15, 4220, 1.0), ("cells 15x1040 cap 4100", 15, 1040, 4100, 0.6))


def root_specs(large=False):
    out = []
    if large:
        for name, rows, cols, cap, density in LARGE:
            out.append(dict(name=name, rows=rows, cols=cols, cap=cap, seed=1000 + 7 * rows + cols, unr=False, opt=False, density=density))
        return out
    for k, (name, rows, cols, cap, opt) in enumerate(_shape_list()):
        seed = 1000 + 7 * rows + cols
        out.append(dict(name=name, rows=rows, cols=cols, cap=cap, seed=seed, unr=False, opt=False))
        if rows > 2:
            out.append(dict(name=name + "+unr", rows=rows, cols=cols, cap=cap, seed=seed, unr=True, opt=False))
        if opt:
            out.append(dict(name=name + "+opt", rows=rows, cols=cols, cap=cap, seed=seed, unr=False, opt=True))
    return out


def build_root(spec):
    # (the tiny roots at density 1: a column without an entry would leave them unbounded)
    A, vibr, vibc = make_root(spec["rows"], spec["cols"], spec["seed"], spec.get("density", 1.0 if spec["name"].startswith("tiny") else 0.6))
    m = spec["rows"] - 1
    unr = [m + spec["cols"] - 2] if spec["unr"] else []  # the last structural variable
    if unr:  # a free variable under "<=" rows of one sign is unbounded unless the dual has a solution: cost = 30 x its column sum gives it one
        A[1:, -1] = np.maximum(A[1:, -1], 1.0)  # (y = 30 on every row covers every other column: costs < 30, an entry >= 1 in each)
        A[0, -1] = 30.0 * A[1:, -1].sum()
    oo = None
    if spec["opt"]:
        rng = np.random.default_rng(spec["seed"] + 1)
        oo = rng.integers(-5, 6, (2, spec["cols"])).astype(np.float64)
    return dict(spec, A=A, vibr=vibr, vibc=vibc, unr_list=unr, oo=oo, check=spec["rows"] * spec["cols"] < 20000)


def tableau(lib, root):
    return Tableau(root["A"], root["vibr"], root["vibc"], root["unr_list"], lib=lib, row_capacity=root["cap"], optional_objectives=root["oo"])


# ---- node families ----------------------------------------------------------------------------------------------------------------
def _cut(kind, var, value):
    return {"type": kind, "varIndex": int(var), "value": float(value)}


def family(root, rhs, rows, vibc):
    """cut lists chosen from the solved root: rhs / rows = its RHS column and row map, vibc = its column map"""
    H, W, spare = len(rows), len(vibc), root["cap"] - len(rows)
    m = root["rows"] - 1
    basic = [(int(rows[r]), float(rhs[r])) for r in range(1, H)]
    frac = [b for b in basic if abs(b[1] - round(b[1])) > 1e-6]
    whole = [b for b in basic if abs(b[1] - round(b[1])) <= 1e-6]

    def spread(xs, k):
        if len(xs) <= k:
            return list(xs)
        return [xs[(len(xs) - 1) * i // (k - 1)] for i in range(k)] if k > 1 else [xs[0]]

    chosen = spread(frac, 3)
    rest = [b for b in whole + frac if b not in chosen]
    slack_first = sorted(rest, key=lambda b: (b[0] >= m, ))  # slack variables of the root's rows first
    chosen += spread(slack_first, 2)
    nonbasic = [int(v) for v in vibc[1:]]  # by column: the first, the middle and the LAST column (W - 1: the edge of the pair copy)
    nb = spread(nonbasic, 3)
    if not any(v < m for v in nb) and any(v < m for v in nonbasic) and len(nb) == 3:
        nb[1] = next(v for v in nonbasic if v < m)  # a cut on a non-basic slack variable
    for u in root["unr_list"]:  # the unrestricted variable itself is cut on, wherever the root left it
        hit = [b for b in basic if b[0] == u]
        if hit and hit[0] not in chosen:
            chosen[-1] = hit[0]
        elif not hit and u not in nb:
            nb[-2 if len(nb) > 1 else 0] = u
    nodes, what = [[]], ["no cuts"]
    if spare < 1:
        return nodes, what
    for v, x in chosen:
        for kind, val, label in (("max", math.floor(x), "floor"), ("min", math.ceil(x), "ceil"), ("max", x, "x"), ("min", x, "x")):
            nodes.append([_cut(kind, v, val)])
            what.append("basic %d %s %s" % (v, kind, label))
    for v in nb:
        for kind, val in (("min", 1.0), ("max", 0.0), ("min", 1e9)):
            nodes.append([_cut(kind, v, val)])
            what.append("non-basic %d %s %g" % (v, kind, val))
    pool = [_cut("max", v, math.floor(x)) for v, x in chosen] + [_cut("min", v, 1.0) for v in nb]
    if spare >= 2 and chosen:
        v, x = chosen[0]
        nodes.append([_cut("max", v, math.floor(x)), _cut("min", v, math.floor(x))])
        what.append("two cuts on basic %d" % v)
        if nb:
            nodes.append([_cut("min", nb[0], 1.0), _cut("max", nb[0], 3.0)])
            what.append("two cuts on non-basic %d" % nb[0])
            b, c = _cut("min", chosen[-1][0], math.ceil(chosen[-1][1])), _cut("min", nb[-1], 1.0)
            nodes.append([b, c])
            what.append("basic then non-basic")
            nodes.append([c, b])
            what.append("non-basic then basic")
    if pool:
        nodes.append([pool[i % len(pool)] for i in range(spare)])
        what.append("exactly spare = %d cuts" % spare)
        if spare >= 65:
            nodes.append([pool[(i * 3 + 1) % len(pool)] for i in range(65)])
            what.append("65 cuts")
    return nodes, what


def bad_lists(root, fam):
    """(label, cut list) the engine must refuse; n_idx = width + 2 * row_capacity + 2 (jslp_engine_create)"""
    n_idx = root["cols"] + 2 * root["cap"] + 2
    good = next((c for c in fam if len(c) == 1), None)
    filler = good[0] if good else _cut("min", int(root["vibc"][1]), 1.0)
    spare = root["cap"] - root["H"]
    out = [("index out of range", [_cut("max", n_idx + 5, 1.0)]),
           ("negative index", ([filler] if spare >= 2 else []) + [_cut("min", -1, 1.0)]),
           ("neither basic nor non-basic", [_cut("max", n_idx - 1, 1.0)]),  # an element index no row or column holds yet
           ("spare + 1 cuts", [filler] * (spare + 1))]
    return out


def outcome(res, rhs, rows):
    h = res.height
    return dict(feasible=bool(res.feasible), bounded=bool(res.bounded), optimal=bool(res.optimal), height=h, p1=res.pivots_phase1,
                p2=res.pivots_phase2, cycle=res.cycle_phase, unbounded_var=res.unbounded_var_index, obj_cell=float(res.obj_cell),
                evaluation=float(res.evaluation), rhs=np.ascontiguousarray(rhs[:h], dtype=np.float64).tobytes(),
                rows=np.ascontiguousarray(rows[:h], dtype=np.int32).tobytes())


def error_code(exc):
    m = ERR_CODE.search(str(exc))
    assert m, str(exc)
    return int(m.group(1))


def plan_root(oracle_lib, spec):
    """the root solved on the oracle, its family and the oracle's outcome of every node, the refused lists and their codes"""
    root = build_root(spec)
    t0 = time.time()
    t = tableau(oracle_lib, root)
    try:
        res = t.simplex(check_cycles=root["check"])
        assert res.feasible and res.bounded and res.optimal, (spec["name"], res.as_dict())
        t.save()
        rhs, rows = t.read_rhs()
        vibc = t.download()[2]
        root.update(H=len(rows), root_eval=float(t.evaluation), root_rhs=rhs.tobytes(), root_rows=rows.tobytes())
        fam, what = family(root, rhs, rows, vibc)
        want = []
        for cuts in fam:
            t.restore()
            r, nrhs, nrows = t.applyCuts(cuts, check_cycles=True)
            want.append(outcome(r, nrhs, nrows))
        bad = []
        for label, cuts in bad_lists(root, fam):
            with pytest.raises(_capi.EngineError) as ei:
                t.applyCuts(cuts, check_cycles=True)
            bad.append((label, cuts, error_code(ei.value)))
            # the node after a refused one, without a restore() in between
            k = len(bad) % len(fam)
            r, nrhs, nrows = t.applyCuts(fam[k], check_cycles=True)
            got = outcome(r, nrhs, nrows)
            for key in ("feasible", "bounded", "optimal", "height", "p1", "p2", "rhs", "rows"):
                assert got[key] == want[k][key], (spec["name"], label, key)
    finally:
        t.close()
    # the variables the compact read-back watches: every variable a family cuts on, the structural ones, one of them twice
    watched = sorted({c["varIndex"] for cuts in fam for c in cuts} | set(range(spec["rows"] - 1, spec["rows"] - 1 + min(spec["cols"] - 1, 40))))
    root.update(family=fam, what=what, want=want, bad=bad, watched=watched, oracle_s=time.time() - t0)
    return root


_PLAN = {}


def plan(oracle_lib):
    if not _PLAN:
        for spec in root_specs() + root_specs(large=True):
            _PLAN[spec["name"]] = plan_root(oracle_lib, spec)
    return _PLAN


def dirty_node(root):
    """a feasible node that pivots (on a root without a zero entry that dirties every row)"""
    return next((k for k, w in enumerate(root["want"]) if w["optimal"] and w["p1"] + max(w["p2"], 0) > 0 and len(root["family"][k]) == 1), None)


def wg_list_cap(name):
    """rows the dirty-row list of the k_node_wg instance holds that the root is meant for: <512, 2048> batches, <1024, 4096> single nodes"""
    return 2048 if name == "dirty 2700x15" else 4096


# ---- CPU: the generator on the oracle alone ---------------------------------------------------------------------------------------
def test_shapes_sit_on_the_edges_they_name():
    names = [s[0] for s in _shape_list()]
    assert len(set(names)) == len(names)
    assert wglds_bytes(16, 2608) <= WGLDS_MAX_BYTES < wglds_bytes(16, 2610)
    cap = largest_cap_that_fits(1040)
    assert wglds_bytes(1040, cap) <= WGLDS_MAX_BYTES < wglds_bytes(1040, cap + 2) and cap > 15 + 2
    lds = {(w + 15) // 16 * 16 for w in (16, 17, 113, 127, 128, 129, 143, 144, 511, 512, 513, 527, 528, 1023, 1024, 1025, 1040)}
    assert lds == {16, 32, 128, 144, 512, 528, 1024, 1040}
    assert {c % 4 for c in (44, 45, 46, 47)} == {0, 1, 2, 3}
    assert wglds_bytes(16, 2720) > WGLDS_MAX_BYTES and 15 * 1040 < 4100 * 1040 and 4100 * 1040 > 4 * 1024 * 1024 > 1790 * 1040 > 1536 * 1024
    for name in THIN + ERROR_ROOTS:
        assert name in {s["name"] for s in root_specs()}, name


def test_families_on_the_oracle(oracle_lib):
    """every root: optimal, its family mixed (>= 10 feasible and >= 3 infeasible nodes; the tiny roots >= 1 of each), the refused lists
    refused with the codes the ABI names, and the node after a refused one correct (asserted in plan_root)"""
    p = plan(oracle_lib)
    stride_cases = set()
    for name, root in p.items():
        want = root["want"]
        feas = sum(1 for w in want if w["feasible"] and w["optimal"])
        infeas = sum(1 for w in want if not w["feasible"])
        assert all(w["bounded"] and w["cycle"] == 0 for w in want), name
        spare = root["cap"] - root["H"]
        if name.startswith("tiny"):
            assert feas >= 1 and infeas >= 1, (name, feas, infeas)
        else:
            assert feas >= 10 and infeas >= 3 and len(want) >= 30, (name, feas, infeas, len(want))
            labels = " | ".join(root["what"])
            for needle in ("no cuts", "max floor", "min ceil", "max x", "min x", "non-basic", "two cuts on basic", "two cuts on non-basic",
                           "basic then non-basic", "non-basic then basic", "exactly spare"):
                assert needle in labels, (name, needle)
            assert ("65 cuts" in labels) == (spare >= 65), name
        assert max(len(c) for c in root["family"]) == (spare if len(root["family"]) > 1 else 0), name
        codes = {label: code for label, _, code in root["bad"]}
        assert codes == {"index out of range": _capi.JSLP_ERR_ARG, "negative index": _capi.JSLP_ERR_ARG,
                         "neither basic nor non-basic": _capi.JSLP_ERR_ARG, "spare + 1 cuts": _capi.JSLP_ERR_CAPACITY}, (name, codes)
        if name.startswith("stride 41x15") and "+" not in name:
            stride_cases |= {(root["cap"] % 4, w["height"] % 2) for w in want}
    # the row capacity modulo 4 against odd and even final heights: the engine's own read-back rounds its stride up to a multiple of 4, so here
    # these roots all take the 16-byte stores; tests/test_pool_device_edges.py is where the residues meet both branches of the gather (the pool's
    # shared buffer is laid out with the plain row capacity, a `_device` caller passes its own row_stride)
    assert stride_cases == {(c, o) for c in range(4) for o in range(2)}, stride_cases
    print({n: round(r["oracle_s"], 2) for n, r in p.items() if r["oracle_s"] > 0.5})
    slow = {n: round(r["oracle_s"], 1) for n, r in p.items() if r["oracle_s"] > 30}
    assert not slow, slow
    # the dirty-row roots: some node repairs with a pivot, and a pivot on a dense column writes every row
    for name, rows, cols, cap, density in LARGE:
        if name.startswith("dirty"):
            assert dirty_node(p[name]) is not None and (p[name]["A"][1:, 1:] != 0).all() and wg_list_cap(name) < rows - 1, name


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
ALL_SETTINGS = {
    "defaults": {},
    "cow0": {"JSLP_NODE_COW": "0"},
    "nowglds": {"JSLP_NO_WGLDS": "1"},
}
THIN_SETTINGS = {
    "group4": {"JSLP_GROUP_MAX": "4"},
    "group4-cow0": {"JSLP_GROUP_MAX": "4", "JSLP_NODE_COW": "0"},
    "cowsmall0": {"JSLP_NODE_COW_SMALL": "0"},
    "cowsingle0": {"JSLP_NODE_COW_SINGLE": "0"},
    "queue0": {"JSLP_NODE_QUEUE": "0"},
    "queue1": {"JSLP_NODE_QUEUE": "1"},
    "notranspose": {"JSLP_SNAPSHOT_TRANSPOSE": "0"},
    "nozerocopy": {"JSLP_ZERO_COPY": "0"},
    "nopoll": {"JSLP_BATCH_POLL": "0"},
    "nonodekernel": {"JSLP_NO_NODE_KERNEL": "1"},
    "threads1024": {"JSLP_WG_BATCH_THREADS": "1024"},
    "threads256": {"JSLP_WG_BATCH_THREADS": "256"},
    "small1024-0": {"JSLP_SMALL_BATCH_1024": "0"},
}


@pytest.fixture(scope="module")
def plan_file(oracle_lib, tmp_path_factory):
    """the oracle's answers, computed once and handed to every worker in a file"""
    path = tmp_path_factory.mktemp("node_edges") / "plan.pkl"
    with open(path, "wb") as fh:
        pickle.dump(plan(oracle_lib), fh, protocol=pickle.HIGHEST_PROTOCOL)
    return str(path)


def _worker(plan_file, mode, extra, names, timeout):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(extra)
    env["JSLP_DEBUG_LAUNCH"] = "1"
    try:
        out = subprocess.run([sys.executable, WORKER, mode, plan_file, "\n".join(names)], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        pytest.exit("the node worker hung (%s): nothing more is started on this GPU" % extra, returncode=3)
    print(out.stdout[-8000:])
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):  # killed by a signal: a fault, not a wrong answer
        pytest.exit("the node worker died with %d (%s): nothing more is started on this GPU\n%s" % (out.returncode, extra, out.stdout[-3000:]), returncode=3)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-3000:] + out.stderr[-5000:]
    return out.stdout


def _kernels(out):
    """root name -> the node kernels the worker saw it launch (every call's lines were already compared with Dispatch there)"""
    return {m.group(1): set(m.group(2).split(" ; ")) for m in re.finditer(r"^root ok \| (.+?) \| .*? \| (.*)$", out, re.M)}


def _meant(kernels, setting):
    """the kernels a root is in the list for, said once more in plain words"""
    lds_off = setting == "nowglds"
    for name, ks in kernels.items():
        joined = " ; ".join(sorted(ks))
        if lds_off or name.endswith(("cap 2610", "cap 2610+unr", "cap 1790", "cap 1790+unr")) or name.startswith("dirty") or "cap 4100" in name:
            assert "k_node_lds" not in joined and "k_node_queue" not in joined and "k_simplex_lds" not in joined, (setting, name, joined)
            if "cap 4100" not in name and setting not in ("nonodekernel", "threads1024", "threads256"):  # (those have no one-launch batch)
                assert "k_node_wg<512,2048>" in ks, (setting, name, joined)
        else:
            assert "k_node_wg" not in joined and "k_simplex_wg<512" not in joined, (setting, name, joined)
            assert ("opt 1" in joined and "opt 0" not in joined) if name.endswith("+opt") else "opt 1" not in joined, (setting, name, joined)
        if "cap 1788" in name or "cap 1790" in name or "cap 4100" in name:  # beyond the single-child cell limit: a node alone is solved chip-wide
            assert "restore+add_cuts+simplex+gather chip-wide" in ks and "k_node_wg<1024,4096>" not in ks, (setting, name, joined)
        else:
            assert any(k.startswith(("k_node_lds<1024", "k_node_wg<1024")) for k in ks) or setting == "nonodekernel", (setting, name, joined)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(ALL_SETTINGS))
def test_node_families_on_every_root(hip_lib, plan_file, setting):
    names = [s["name"] for s in root_specs()] if setting == "defaults" else most_roots()
    out = _worker(plan_file, "families", ALL_SETTINGS[setting], names, 900)
    assert out.count("root ok") == len(names)
    kernels = _kernels(out)
    _meant(kernels, setting)
    if setting == "defaults":
        assert "k_node_queue<512,cow 1,opt 0>" in kernels["H 2049x15"] and "k_node_queue<512,cow 0,opt 1>" in kernels["H 513x15+opt"]
        assert "k_node_lds<1024,opt 0,cow 1>" in kernels["fit 2590x15 cap 2608"] and "k_node_wg<1024,4096>" in kernels["fit 2590x15 cap 2610"]
    if setting == "cow0":
        assert "k_node_queue<512,cow 0,opt 0>" in kernels["H 2049x15"] and "k_node_lds<1024,opt 0,cow 0>" in kernels["H 2049x15"]


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(THIN_SETTINGS))
def test_node_families_under_the_other_knobs(hip_lib, plan_file, setting):
    names = thin_roots(setting)
    out = _worker(plan_file, "families", THIN_SETTINGS[setting], names, 600)
    assert out.count("root ok") == len(names)
    kernels = _kernels(out)
    _meant(kernels, setting)
    ks = kernels["H 2049x15"]
    want = {"group4": "k_node_queue<512,cow 1,opt 0>", "group4-cow0": "k_node_queue<512,cow 0,opt 0>", "cowsmall0": "k_node_lds<1024,opt 0,cow 0>", "cowsingle0": "k_node_lds<1024,opt 0,cow 0>",
            "queue0": "k_node_lds<512,opt 0,cow 0>", "queue1": "k_node_queue<512,cow 1,opt 0>", "notranspose": "k_node_queue<512,cow 1,opt 0>",
            "nozerocopy": "k_node_queue<512,cow 1,opt 0>", "nopoll": "k_node_lds<1024,opt 0,cow 1>",
            "nonodekernel": "restore+add_cuts+simplex+gather k_simplex_lds<1024,opt 0>", "threads1024": "restore+add_cuts+simplex+gather k_simplex_lds<1024,opt 0>",
            "threads256": "restore+add_cuts+simplex+gather k_simplex_wg<256,1024>", "small1024-0": "k_node_lds<512,opt 0,cow 0>"}[setting]
    assert want in ks, (setting, sorted(ks))
    if setting in ("queue0", "nonodekernel", "threads1024", "threads256"):
        assert not any(k.startswith("k_node_queue") for k in ks), (setting, sorted(ks))
    if setting == "nonodekernel":
        assert not any(k.startswith("k_node_") for k in ks), sorted(ks)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["defaults", "cow0", "nowglds"])
def test_large_roots(hip_lib, plan_file, setting):
    """more dirty rows than k_node_wg's list holds (the list-free restore loop, proven by the restored_rows counter) and a row capacity x ld
    beyond the 4 M cell batch limit (every node on the chip-wide path, one after the other)"""
    names = [s["name"] for s in root_specs(large=True)]
    out = _worker(plan_file, "large", ALL_SETTINGS[setting], names, 900)
    assert out.count("root ok") == len(names)
    _meant(_kernels(out), setting)
    assert len(re.findall(r"restored_rows \+(\d+)", out)) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["defaults", "cow0", "nowglds"])
def test_refused_cut_lists_and_the_calls_after_them(hip_lib, plan_file, setting):
    out = _worker(plan_file, "errors", ALL_SETTINGS[setting], list(ERROR_ROOTS), 600)
    assert out.count("root ok") == len(ERROR_ROOTS)
