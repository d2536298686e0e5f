"""A node's MIR loop inside ONE engine call (include/jslpr_mir.h; Tableau.applyCutsMIR / applyCutsBatchMIR), on the CPU: the oracle library
does not export the extension, so the calls are restated from applyCuts / applyCutsFrom + mirRound (engine.py) -- what is pinned here is
the host side: the trees that use the one-call form (JSLP_TREE_MIR=1) and the speculative MIR batches give the sequential run, bit for bit.
"""
import copy
import gzip
import json
import math
import os

import numpy as np
import pytest

import golden_util as G
from jslpsolver_amd import Model, Tableau, pivot_digest, solver
from test_mir_cuts import CASES, case_id, heavy, run_case

# mir.json.gz holds 17 default-service cases that are not skipped (22 with mirCuts > 0, 5 of them with presolveFixed > 0); mir_extra.json.gz adds two
# more, recorded from the reference in the same way and in the same format:
#   node tests/golden/gen_golden_mir.js --case mir_extra/RandomLP_5x4_seed<N>.json.gz '{"useMIRCuts":true,"presolve":false}'
# on generators.random_lp_model(N, 5, 4) with every variable an integer (N = 35, 12).  Both trees hold nodes whose first simplex is optimal and
# whose later MIR round ends infeasible (the fold's "evaluation kept" arm), which no case of mir.json.gz has.
with gzip.open(os.path.join(G.GOLDEN, "mir_extra.json.gz"), "rt") as _fh:
    EXTRA_CASES = json.load(_fh)["cases"]
MIR_CASES = [c for c in CASES if c["mirCuts"] > 0 and not heavy(c)] + EXTRA_CASES
DEFAULT_CASES = [c for c in MIR_CASES if not c["options"].get("useIncremental")]


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("case", MIR_CASES, ids=case_id)
def test_trees_with_one_call_per_node(oracle_lib, case, monkeypatch):
    """nPivots, pivotDigest, iterations, result keys and values, matrixSha of the golden (run_case asserts them)"""
    monkeypatch.setenv("JSLP_TREE_MIR", "1")
    run_case(oracle_lib, case)


def solve_tree(lib, case, speculate):
    g = G.load(os.path.join(G.GOLDEN, case["file"]))
    model = copy.deepcopy(g["model"])
    model["options"] = case["options"]
    m, t, n_int, incremental = solver._prepare(model, None, lib, 0, None)
    try:
        assert not incremental
        out = solver._solve_on(t, m, n_int, False, speculate, None, True)
        out["speculated"] = getattr(t, "speculated_nodes", 0)
        return out
    finally:
        t.close()


def check_speculative(lib, case, specs=(2, 8)):
    if case["presolveFixed"] > 0:
        pytest.skip("the reference's presolve pre-pass fixed variables: host pre-pass out of scope")
    seq = solve_tree(lib, case, 1)
    assert seq["speculated"] == 0
    for spec in specs:
        par = solve_tree(lib, case, spec)
        assert par["iter"] == seq["iter"] == case["iterations"]
        assert par["result"] == seq["result"] and list(par["result"]) == list(seq["result"]) == case["resultKeys"]
        for k, v in case["result"].items():
            ref = v if isinstance(v, bool) else G.num(v)
            assert par["result"][k] == ref or (isinstance(ref, float) and np.isnan(ref) and np.isnan(par["result"][k])), k
        assert par["matrix"].tobytes() == seq["matrix"].tobytes()
        assert np.array_equal(par["varIndexByRow"], seq["varIndexByRow"]) and np.array_equal(par["varIndexByCol"], seq["varIndexByCol"])
        if seq["iter"] > 1:
            assert par["speculated"] > 0, "speculation was switched off"


@pytest.mark.parametrize("case", DEFAULT_CASES, ids=case_id)
def test_speculative_mir_tree_gives_the_sequential_run(oracle_lib, case):
    check_speculative(oracle_lib, case)


def test_enough_default_cases_run():
    """at least 18 default-service cases run (are not skipped): the 17 of mir.json.gz and the two of mir_extra.json.gz"""
    assert sum(1 for c in DEFAULT_CASES if c["presolveFixed"] == 0) >= 18
    assert sum(1 for c in DEFAULT_CASES if c["presolveFixed"] == 0 and c not in EXTRA_CASES) == 17 and len(EXTRA_CASES) == 2


# ---- the calls themselves on Knapsack_1's recorded nodes ------------------------------------------------------------
def volume(ints, rhs, vibr, precision):
    """computeFractionalVolume(true), mip-utils.ts:67-92, written out once more for the test"""
    vol = -1.0
    for r in range(1, len(vibr)):
        if int(vibr[r]) not in ints:
            continue
        d = abs(float(rhs[r]))
        if math.isfinite(d) and min(d - math.floor(d), math.floor(d + 1)) < precision:
            continue
        vol = d if vol == -1.0 else vol * d
    return 0.0 if vol == -1.0 else vol


def load_nodes(name, limit=None):
    g = G.load(os.path.join(G.GOLDEN, "fixtures", name + ".json.gz"))
    tab = g["tableau"]
    nodes = [c["cuts"] or [] for c in g["simplexCalls"][1:]]
    return tab, nodes[:limit] if limit else nodes


def root_tableau(lib, tab, nodes):
    m, vibr, vibc = G.dense_tableau(tab)
    t = Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], row_capacity=tab["height"] + max(len(n) for n in nodes) + 320,
                lib=lib, integer_variables=tab["integerVarIndexes"])
    t.applyCuts([], check_cycles=True)
    t.save()
    return t


def by_hand(t, ints, cuts, max_rounds, need_feasible):
    """the sequence the one-call form stands for, on a tableau holding the saved root.  Returns a dict: the last result, whether any of
    the node's simplexes set the evaluation and to what, the outcome record's fields, the final RHS column and row map"""
    res, rhs, vibr = t.applyCuts(cuts, check_cycles=True)
    rounds = rows = 0
    sets = bool(res.optimal) or not res.bounded
    n_optimal, pivots = int(bool(res.optimal)), res.pivots_phase1 + max(res.pivots_phase2, 0)  # (-1: phase 2 was not entered)
    before = after = 0.0
    per_round = []  # (candidate rows of the round, rows it added)
    if not (need_feasible and not res.feasible):
        while max_rounds < 0 or rounds < max_rounds:
            before = volume(ints, rhs, vibr, t.precision)
            frac = [float(x) - (math.floor(x) if math.isfinite(x) else float(x)) for x, v in zip(rhs[1:len(vibr)], vibr[1:]) if int(v) in ints]  # (NaN for a non-finite row)
            n, res, rhs, vibr = t.mirRound(check_cycles=True)
            per_round.append((sum(1 for f in frac if not (f < t.precision or f > 1 - t.precision)), n))
            after = volume(ints, rhs, vibr, t.precision)
            rounds += 1
            rows += n
            sets = sets or bool(res.optimal) or not res.bounded
            n_optimal += int(bool(res.optimal))
            pivots += res.pivots_phase1 + max(res.pivots_phase2, 0)
            if after >= 0.9 * before:
                break
    return {"res": res, "sets": sets, "evaluation": t.evaluation, "record": (rounds, rows, n_optimal, pivots), "volumes": (before, after),
            "rhs": rhs.copy(), "vibr": vibr.copy(), "per_round": per_round}


def same_node(got, e, prev):
    """got = (result, outcome, rhs, vibr) of a one-call node; prev: the evaluation a node none of whose simplexes set it keeps"""
    res, oc, rhs, vibr = got
    d, x = res.as_dict(), e["res"].as_dict()
    d.pop("evaluation"), x.pop("evaluation")
    d["obj_cell"], x["obj_cell"] = int(u64(d["obj_cell"]).reshape(-1)[0]), int(u64(x["obj_cell"]).reshape(-1)[0])
    assert d == x
    assert u64(res.evaluation)[()] == u64(e["evaluation"] if e["sets"] else prev)[()]
    assert (int(oc["rounds"]), int(oc["rows_added"]), int(oc["optimal_count"]), int(oc["pivots"])) == e["record"]
    assert u64(oc["volume_before"])[()] == u64(e["volumes"][0])[()] and u64(oc["volume_after"])[()] == u64(e["volumes"][1])[()]
    h = res.height
    assert np.array_equal(u64(rhs[:h]), u64(e["rhs"])) and np.array_equal(vibr[:h], e["vibr"])


def expectations(oracle_lib, tab, nodes, max_rounds, need_feasible):
    """(the root's evaluation, by_hand of every node) on the oracle library"""
    ref = root_tableau(oracle_lib, tab, nodes)
    root_eval = ref.evaluation
    out = [by_hand(ref, set(tab["integerVarIndexes"]), cuts, max_rounds, need_feasible) for cuts in nodes]
    ref.close()
    return root_eval, out


@pytest.mark.parametrize("max_rounds,need_feasible", [(-1, False), (3, True)])
def test_batch_equals_node_by_node_equals_the_sequence(oracle_lib, max_rounds, need_feasible):
    tab, nodes = load_nodes("Knapsack_1")
    root_eval, expect = expectations(oracle_lib, tab, nodes, max_rounds, need_feasible)
    assert any(e["record"][0] > 1 for e in expect) and any(e["record"][1] > 0 for e in expect)
    rounds = None if max_rounds < 0 else max_rounds
    one = root_tableau(oracle_lib, tab, nodes)
    iters0, prev = one.simplexIters, one.evaluation
    for cuts, e in zip(nodes, expect):
        got = one.applyCutsMIR(cuts, max_rounds=rounds, need_feasible=need_feasible)
        same_node(got, e, prev)
        prev = got[0].evaluation
        assert one.evaluation == prev and one.feasible == bool(got[0].feasible)
    assert one.simplexIters == iters0 + sum(e["record"][2] for e in expect)
    one.close()
    batch = root_tableau(oracle_lib, tab, nodes)
    before = (batch.evaluation, batch.simplexIters, batch.feasible)
    results, ocs, rhs, vibr = batch.applyCutsBatchMIR(nodes, max_rounds=rounds, need_feasible=need_feasible)
    assert (batch.evaluation, batch.simplexIters, batch.feasible) == before  # a batch folds nothing into the object
    for i, e in enumerate(expect):
        same_node((results[i], ocs[i], rhs[i], vibr[i]), e, root_eval)
    batch.close()


# ---- the fold's "evaluation kept" arm: a node whose first simplex is optimal and whose later MIR round ends infeasible -------------
# None of the recorded inputs has one; a search over generators.random_lp_model (5 variables, 4 constraints, all integer) found seed 35.
KEPT_MODEL = {"name": "RandomLP_5x4_seed35", "optimize": "objective", "opType": "min",
              "constraints": {"c0": {"max": 587.0}, "c1": {"min": 473.0}, "c2": {"min": 525.0}, "c3": {"max": 575.0}},
              "variables": {"x0": {"objective": 1.0, "c0": 39.0, "c1": 22.0, "c2": 68.0, "c3": 75.0}, "x1": {"objective": 51.0, "c2": 100.0, "c3": 33.0},
                            "x2": {"objective": 73.0, "c1": 80.0, "c2": 14.0}, "x3": {"objective": 89.0, "c0": 63.0, "c1": 2.0, "c2": 96.0, "c3": 57.0},
                            "x4": {"objective": 40.0, "c1": 97.0, "c2": 12.0, "c3": 56.0}},
              "ints": {"x0": 1, "x1": 1, "x2": 1, "x3": 1, "x4": 1}, "options": {"useMIRCuts": True, "presolve": False}}
KEPT_CUTS = [{"type": "max", "varIndex": 6, "value": 3.0}, {"type": "min", "varIndex": 4, "value": 6.0}, {"type": "max", "varIndex": 8, "value": 1.0}]


def kept_root(lib):
    """the model's tableau as the default service saves it: the root's simplex and MIR loop, then save()"""
    from jslpsolver_amd.branch_and_cut import mir_loop
    m, t, _n_int, _incremental = solver._prepare(copy.deepcopy(KEPT_MODEL), None, lib, 0, None)
    _res, rhs, vibr = t.applyCuts([], check_cycles=m.checkForCycles)
    mir_loop(t, m, rhs, vibr, m.checkForCycles)
    t.save()
    return m, t


def check_evaluation_kept(lib, oracle_lib, monkeypatch):
    m, ref = kept_root(oracle_lib)
    ints = set(int(i) for i in m.integer_index_array)
    first = ref.applyCuts(KEPT_CUTS)[0]
    first_eval = ref.evaluation
    e = by_hand(ref, ints, KEPT_CUTS, -1, False)
    ref.close()
    assert first.optimal and e["record"][0] >= 1 and not e["res"].feasible and not e["res"].optimal and e["res"].bounded  # the case itself
    assert e["sets"] and e["evaluation"] == first_eval and e["record"][2] >= 1
    _m, t = kept_root(lib)
    got = t.applyCutsMIR(KEPT_CUTS)
    same_node(got, e, float("nan"))
    assert t.evaluation == first_eval and not t.feasible
    t.restore()
    results, ocs, rhs, vibr = t.applyCutsBatchMIR([KEPT_CUTS, [], KEPT_CUTS])
    same_node((results[0], ocs[0], rhs[0], vibr[0]), e, float("nan"))
    same_node((results[2], ocs[2], rhs[2], vibr[2]), e, float("nan"))
    t.close()
    seq = solver.Solve(copy.deepcopy(KEPT_MODEL), full=True, lib=oracle_lib)
    for spec, knob in ((1, "1"), (8, "0")):
        monkeypatch.setenv("JSLP_TREE_MIR", knob)
        par = solver.Solve(copy.deepcopy(KEPT_MODEL), full=True, lib=lib, speculate=spec)
        assert par["iter"] == seq["iter"] == 11 and par["result"] == seq["result"] and par["matrix"].tobytes() == seq["matrix"].tobytes()


def test_evaluation_kept_when_a_later_round_ends_infeasible(oracle_lib, monkeypatch):
    check_evaluation_kept(oracle_lib, oracle_lib, monkeypatch)


# ---- a MIR tree that finds no incumbent: the tableau is left on the node evaluated last, with that node's MIR rows -------------------
# (an infeasible integer program behind a fractional root; no recorded case is one)
NO_INCUMBENT_MODEL = {"optimize": "obj", "opType": "max",
                      "constraints": {"c0": {"equal": 7}, "c1": {"min": 11}, "c2": {"max": 3}, "u0": {"max": 2}, "u1": {"max": 4}, "u2": {"max": 1}},
                      "variables": {"x0": {"obj": 7, "c0": 6, "c1": 2, "c2": 2, "u0": 1}, "x1": {"obj": 4, "c1": 5, "u1": 1},
                                    "x2": {"obj": 9, "c0": 3, "c1": 2, "c2": 3, "u2": 1}},
                      "ints": {"x0": 1, "x1": 1, "x2": 1}, "options": {"useMIRCuts": True, "presolve": False}}


def check_no_incumbent(lib, oracle_lib, monkeypatch):
    seq = solver.Solve(copy.deepcopy(NO_INCUMBENT_MODEL), full=True, lib=oracle_lib)
    assert seq["iter"] > 1 and not seq["result"]["feasible"] and "isIntegral" not in seq["result"]  # the case itself
    for spec, knob in ((1, "1"), (2, "0"), (8, "0")):
        monkeypatch.setenv("JSLP_TREE_MIR", knob)
        par = solver.Solve(copy.deepcopy(NO_INCUMBENT_MODEL), full=True, lib=lib, speculate=spec)
        assert par["iter"] == seq["iter"] and par["result"] == seq["result"] and list(par["result"]) == list(seq["result"])
        assert par["matrix"].shape == seq["matrix"].shape and par["matrix"].tobytes() == seq["matrix"].tobytes()
        assert np.array_equal(par["varIndexByRow"], seq["varIndexByRow"]) and np.array_equal(par["varIndexByCol"], seq["varIndexByCol"])


def test_tree_without_an_incumbent_ends_on_the_last_node_with_its_mir_rows(oracle_lib, monkeypatch):
    check_no_incumbent(oracle_lib, oracle_lib, monkeypatch)


def test_one_call_refusals(oracle_lib):
    from jslpsolver_amd import _capi
    tab, nodes = load_nodes("Knapsack_1", 4)
    m, vibr, vibc = G.dense_tableau(tab)
    t = Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], row_capacity=tab["height"] + 330, lib=oracle_lib)
    t.applyCuts([], check_cycles=True)
    with pytest.raises(_capi.EngineError, match=r"\(%d\)" % _capi.JSLP_ERR_STATE):  # no integer variables registered
        t.applyCutsMIR(nodes[0])
    t.close()
    t = root_tableau(oracle_lib, tab, nodes)
    with pytest.raises(_capi.EngineError, match=r"\(%d\)" % _capi.JSLP_ERR_ARG):
        t.applyCutsMIR(nodes[0], max_rounds=_capi.JSLPR_MAX_ROUNDS + 1)
    t.close()
