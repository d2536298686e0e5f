"""Shared by tests/test_tree_tol_cpu.py and tests/test_tree_tol_gpu.py: packs whose LPs carry options.tolerance
(include/jslpg_tree_tolerance.h) built from the items of tests/tree_pack_util.py, tree_mir_util.py and tree_inc_util.py, the reference's
recorded runs with a tolerance (tests/golden/tolerance.json.gz, the tolerance records of mir.json.gz), and the state such a pack leaves, as
bytes."""
import copy
import gzip
import json
import os

import numpy as np

import golden_util as G
import tree_inc_util as I
import tree_mir_util as M
import tree_pack_util as U
from jslpsolver_amd.engine import TableauPack
from jslpsolver_amd.model import Model, UnsupportedModel

TOLERANCES = (None, 1e-9, 0.05, 0.5, 3)


def make_pack(lib, items, policies, tolerance, minimize, trace_cap=8192, heap_cap=256, max_nodes=0, max_pivots=0, with_arrays=True):
    """tree_inc_util.make_pack with, per item, its tolerance (None: none) and whether its model minimises.  with_arrays=False: the same pack
    made without the two arrays (every tolerance must then be None)"""
    is_inc = [isinstance(p, I.Inc) for p in policies]
    mir = [bool(getattr(it, "mir", False)) for it in items]
    optional = [getattr(it, "optional", None) for it in items]
    pairs = [(p[0], p[1]) if p is not None else (None, None) for p in policies]
    extra = {} if not with_arrays else dict(tolerance=list(tolerance), minimize=[bool(f) for f in minimize])
    return TableauPack([it.lp for it in items], precision=[it.precision for it in items], lib=lib, trace_cap=trace_cap, max_pivots=max_pivots,
                       integers=[it.integers for it in items], cut_rows=[it.cut_rows for it in items], heap_cap=heap_cap, max_nodes=max_nodes,
                       node_selection=[p[0] for p in pairs], branching=[p[1] for p in pairs], incremental=is_inc if any(is_inc) else None,
                       max_checkpoints=[p.max_checkpoints if f else 0 for p, f in zip(policies, is_inc)],
                       row_extra=[it.row_extra if f or m else -1 for it, f, m in zip(items, is_inc, mir)] if any(is_inc) or any(mir) else None,
                       optional_objectives=optional if any(o is not None for o in optional) else None, mir=mir if any(mir) else None, **extra)


def solve(lib, items, policies, tolerance, minimize, **kw):
    """the solved pack.  Its tolerance records start as 0x5a bytes, so that zeros in them after the call are the call's own"""
    pack = make_pack(lib, items, policies, tolerance, minimize, **kw)
    pack.tolerance[:] = np.frombuffer(b"\x5a" * pack.tolerance.nbytes, dtype=pack.tolerance.dtype)
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    return pack


def state(pack, i):
    """tree_inc_util.state with the LP's tolerance record"""
    s = I.state(pack, i)
    s["tolerance"] = pack.tolerance[i].tobytes()
    return s


def states(pack):
    return [state(pack, i) for i in range(len(pack))]


def against_host(hip_lib, oracle_lib, items, policies, tolerance, minimize, **kw):
    """one pack on the GPU, one call; every LP against the Python host tree on the oracle, everything as bytes"""
    host = solve(oracle_lib, items, policies, tolerance, minimize, **kw)
    pack = solve(hip_lib, items, policies, tolerance, minimize, **kw)
    for i, (a, b) in enumerate(zip(states(pack), states(host))):
        assert a == b, "LP %d (%s, tolerance %s, minimize %s) differs from the host tree: %s" % (
            i, policies[i], tolerance[i], minimize[i], [k for k in a if a[k] != b[k]])
    return pack, host


def lp_of(model_json):
    """(item, policy) of a model as solve_packed(..., incremental=True, tolerance=True) gives it to the pack; None where it does not go
    there (a service combination the pack does not have, no room for a cut row, a model the Python host refuses)"""
    try:
        m = Model(model_json, None)
    except UnsupportedModel:
        return None
    o = m.options
    _, oo = m.optional_objectives()
    if len(m.integerVariables) == 0 or (oo is not None and len(oo) > 0):
        return None
    enhanced = bool(o.get("nodeSelection") or o.get("branching"))
    if o.get("useIncremental") is True:
        if m.useMIRCuts:
            return None
        it, policy = I.Item(model_json), I.inc_of(o)
        return (it, policy) if it.row_extra >= 1 else None
    if m.useMIRCuts:
        if enhanced:
            return None
        it = M.MirItem(model_json)
        return (it, None) if it.row_extra >= 1 else None
    it = U.Item(model_json)
    if it.cut_rows < 1:
        return None
    return it, ((o.get("nodeSelection"), o.get("branching")) if enhanced else None)


def negated(model_json):
    """the same model with the other sense and the objective negated: the same tableau, the other acceptableThreshold"""
    m = copy.deepcopy(model_json)
    m["opType"] = "min" if m.get("opType") == "max" else "max"
    for v in m["variables"].values():
        if m["optimize"] in v:
            v[m["optimize"]] = -v[m["optimize"]]
    return m


def golden_records():
    """every record of tests/golden/tolerance.json.gz and the tolerance records of mir.json.gz (none has a timeout) with its model:
    [(record, model json)]"""
    with gzip.open(os.path.join(G.GOLDEN, "tolerance.json.gz"), "rt") as fh:
        cases = json.load(fh)
    with gzip.open(os.path.join(G.GOLDEN, "mir.json.gz"), "rt") as fh:
        cases += [c for c in json.load(fh)["cases"] if "tolerance" in c["options"] and "timeout" not in c["options"]]
    fuzz = U._cases("fuzz_services.jsonl.gz")
    out = []
    for c in cases:
        if "file" in c:
            model = dict(G.load(os.path.join(G.GOLDEN, c["file"]))["model"])
            assert c["presolveFixed"] == 0
        else:
            model = dict(fuzz[c["line"]]["model"])
            assert (fuzz[c["line"]]["gen"], fuzz[c["line"]]["seed"]) == (c["gen"], c["seed"])
        model["options"] = dict(c["options"])
        out.append((c, model))
    return out


def check_golden(pack, i, item, c):
    where = (c.get("file", c.get("gen")), c.get("seed"), c["options"])
    U.check_record(pack, i, item, c["nPivots"], c["pivotDigest"], c["iterations"], c["resultKeys"], c["result"], where)
    assert int(pack.tree[i]["final_height"]) == c["height"], where
    if "bestPossibleEval" in c:
        assert np.float64(pack.tolerance[i]["best_possible"]).tobytes() == np.float64(G.num(c["bestPossibleEval"])).tobytes(), where


def host_walk(lib, item, policy, tolerance, minimize, _late_stop=True, heap_cap=256, max_nodes=1 << 20):
    """the Python host tree of one LP on an engine of `lib` (the oracle), as TableauPack's restatement runs it, with _late_stop handed
    through: (iterations, the tolerance record as a dict, the tableau's evaluation, per simplex whether it ended optimal)"""
    from jslpsolver_amd import branch_and_cut as bc
    from jslpsolver_amd import incremental_branch_and_cut as ibc
    from jslpsolver_amd.engine import Tableau, _TreeModel
    m, vibr, vibc, unr = item.lp
    mir = bool(getattr(item, "mir", False))
    is_inc = isinstance(policy, I.Inc)
    rows = item.row_extra if mir or is_inc else item.cut_rows
    t = Tableau(m, vibr, vibc, unr, precision=item.precision, row_capacity=m.shape[0] + rows, lib=lib, integer_variables=item.integers if mir else None)
    optimal, absorb = [], t._absorb

    def spy(res):
        optimal.append(bool(res.optimal))
        return absorb(res)

    t._absorb = spy
    model = _TreeModel(item.integers, item.check, mir=mir, tolerance=tolerance or 0, minimize=minimize)
    out = {}
    try:
        if policy is None:
            iterations, _ = bc.branch_and_cut(t, model, heap=bc.CountingHeap(heap_cap=heap_cap, cut_rows=item.cut_rows), max_nodes=max_nodes,
                                              tolerance_out=out, _late_stop=_late_stop)
        else:
            boxes = ibc.CountingContainers(heap_cap=heap_cap, cut_rows=item.cut_rows, max_nodes=max_nodes)
            kw = dict(node_selection=policy[0] or "hybrid", branching=policy[1] or "pseudocost", containers=boxes, tolerance_out=out, _late_stop=_late_stop)
            if is_inc:
                iterations, _ = ibc.incremental_branch_and_cut(t, model, max_checkpoints=policy.max_checkpoints, **kw)
            else:
                iterations, _ = ibc.enhanced_branch_and_cut(t, model, **kw)
        return iterations, out, t.evaluation, optimal
    finally:
        t.close()


def _model(op, constraints, variables):
    return {"optimize": "obj", "opType": op, "constraints": constraints, "variables": variables, "ints": {v: 1 for v in variables}}


# The edge models: tiny, found by a seeded search over random models on the CPU oracle and fixed here.
# LATE (a minimisation, default service, tolerance 0.5): the turn that lowers the flag still evaluates its node, the 9th, which becomes
# the incumbent (28 instead of 29) -- a walk that breaks at once has 8 iterations and the other result.
LATE = _model("min", {"c0": {"min": 15}, "c1": {"min": 29}},
              {"x0": {"obj": 5, "c0": 2, "c1": 7}, "x1": {"obj": 5, "c0": 1, "c1": 4}, "x2": {"obj": 4, "c0": 5, "c1": 3}})
# EXACT (a minimisation): bestPossibleEval 100 and an incumbent of 125 with entries waiting, all integers: at tolerance 0.25 the threshold
# is 125 exactly and the strict comparison does not stop (5 iterations); at the next tolerance whose factor 1 + tolerance differs --
# nextafter(1.25) - 1: the doubles between 0.25 and it round to the same factor in the reference too -- it stops (3 iterations, 2 left).
EXACT = _model("min", {"c0": {"min": 1.5}, "c1": {"min": 5.0}, "c2": {"min": 3.0}},
               {"x0": {"obj": 25, "c1": 2, "c2": 1}, "x1": {"obj": 75, "c0": 3, "c1": 2, "c2": 1}})
EXACT_UP = float(np.nextafter(1.25, 2)) - 1.0
# MAXI (a maximisation, root -31.5): a walk of some twenty nodes under every service; at tolerance >= 1 its factor is <= 0
MAXI = _model("max", {"c0": {"max": 22}, "c1": {"max": 21}}, {"x0": {"obj": 4, "c1": 4}, "x1": {"obj": 6, "c0": 2, "c1": 4}})
# LATE_ROOT (a maximisation): the root's simplex ends unbounded, the second node's optimal at -8: bestPossibleEval comes from that node
LATE_ROOT = _model("max", {"c0": {"min": 8}, "c1": {"min": 3}},
                   {"x0": {"obj": 0, "c0": -3, "c1": -4}, "x1": {"obj": 2, "c0": 3, "c1": 2}, "x2": {"obj": 2, "c0": 0, "c1": -3}})
# NO_OPTIMUM: an infeasible root, one iteration, bestPossibleEval stays 0
NO_OPTIMUM = _model("min", {"c0": {"min": 5}, "c1": {"max": 3}}, {"x0": {"obj": 1, "c0": 1, "c1": 1}})
# INTEGRAL_ROOT: the root is integral: one iteration, no threshold but the root turn's 0, nothing stopped, nothing left
INTEGRAL_ROOT = _model("min", {"c0": {"min": 2}}, {"x0": {"obj": 25, "c0": 1}})
