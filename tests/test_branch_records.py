"""Branch records on the GPU (include/jslpx_branch.h): isIntegral() / getMostFractionalVar() of every node, decided on the device.

1. against the reference: every decision tests/golden/gen_golden_branch.js recorded, replayed as single nodes, one-group batches of 2-16 and
   one queue batch, under JSLP_FORCE_PATH=wg and the default policy;
2. against the restatement (engine.branch_record_from_watched) on the compact read-back of the same call: bench.py's 2416-node Monster_II batch;
3. edge cases: .5 ties (positive and negative), equal fractions, a fraction equal to the precision, all-integral nodes, a watched list of more
   than 1024 entries with duplicates, infeasible and unbounded nodes;
4. whole speculative solves with JSLP_TREE_BRANCH=1 against the goldens."""
import os

import numpy as np
import pytest

import golden_util as G
from jslpsolver_amd import Solve, _capi
from jslpsolver_amd.engine import Tableau, branch_record_from_watched
from jslpsolver_amd.model import Model

pytestmark = pytest.mark.gpu
NAMES = ["Monster_II", "LargeFarmMIP", "Knapsack_1", "Integer_Wood_Shop_Problem", "Sudoku4x4"]


def bits(recs):
    return np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1).view(np.int64)


def f64bits(x):
    return int(np.float64(x).view(np.int64))


def fixture_tableau(lib, name, extra_rows=0):
    g = G.load(os.path.join(G.GOLDEN, "fixtures", name + ".json.gz"))
    tab = g["tableau"]
    m, vibr, vibc = G.dense_tableau(tab)
    calls = g["simplexCalls"]
    # (the engine watches at most row_capacity variables: LargeFarmMIP has 100 integer variables over 36 rows)
    cap = max(tab["height"] + max([len(c["cuts"] or []) for c in calls] + [0]), len(tab["integerVarIndexes"])) + extra_rows
    t = Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], row_capacity=cap, lib=lib)
    t.applyCuts([], check_cycles=tab["checkForCycles"])
    t.save()
    t.set_watched_variables(tab["integerVarIndexes"])
    return t, g


def shapes(n):
    """the batch shapes a decision is replayed in: single nodes, one-group batches of 2..16, the whole list in one call"""
    yield "single", [[i] for i in range(n)]
    groups, i, k = [], 0, 2
    while i < n:
        groups.append(list(range(i, min(n, i + k))))
        i += k
        k = 2 + (k - 1) % 15
    yield "groups", groups
    yield "queue", [list(range(n))]


@pytest.mark.parametrize("path", ["wg", None])
@pytest.mark.parametrize("name", NAMES)
def test_records_match_the_reference_decisions(hip_lib, name, path, monkeypatch):
    if path:
        monkeypatch.setenv("JSLP_FORCE_PATH", path)
    b = G.load(os.path.join(G.GOLDEN, "branch", name + ".json.gz"))
    t, g = fixture_tableau(hip_lib, name)
    calls = g["simplexCalls"]
    assert b["rhsShas"] == [c["rhsSha"] for c in calls]
    check = g["tableau"]["checkForCycles"]
    decisions = b["decisions"]
    node_cuts = [calls[d["call"]]["cuts"] or [] for d in decisions]
    for shape, batches in shapes(len(decisions)):
        if shape == "single" and len(decisions) > 200:
            batches = batches[::7]  # (LargeFarmMIP: a sample of its 1249 decisions one call each)
        for idx in batches:
            results, recs = t.applyCutsBatchBranch([node_cuts[i] for i in idx], check_cycles=check)
            for j, i in enumerate(idx):
                d, call, r, res = decisions[i], calls[decisions[i]["call"]], recs[j], results[j]
                where = "%s %s node %d (call %d)" % (name, shape, i, d["call"])
                assert bool(r["flags"] & _capi.BRANCH_INTEGRAL) == d["isIntegral"], where
                assert int(r["branch_var_index"]) == d["index"], where
                assert f64bits(r["branch_var_value"]) == f64bits(G.num(d["value"])), where
                assert int(r["height"]) == call["height"] and bool(r["flags"] & _capi.BRANCH_FEASIBLE) == call["feasible"], where
                assert res.height == call["height"] and bool(res.feasible) == call["feasible"], where
                if res.optimal:
                    assert f64bits(res.evaluation) == f64bits(G.num(call["evaluation"])), where
    t.close()


def test_records_match_the_restatement_on_the_bench_batch(hip_lib):
    """bench.py's strong-scaling batch: Monster_II's 151 node relaxations x 16 = 2416 nodes, the compact and the record call of the same
    batch, every record compared as int64 bit patterns (host copy and pinned view)"""
    t, g = fixture_tableau(hip_lib, "Monster_II")
    nodes = [c["cuts"] or [] for c in g["simplexCalls"][1:]] * 16
    assert len(nodes) == 2416
    pk = t.pack_cut_lists(nodes)
    watched = g["tableau"]["integerVarIndexes"]
    for copy in (True, False):
        res_c, rows, vals = t.applyCutsBatchWatched(None, check_cycles=True, packed=pk)
        want = branch_record_from_watched([res_c[i] for i in range(len(nodes))], rows[:len(nodes)], vals[:len(nodes)], watched, t.precision)
        results, recs = t.applyCutsBatchBranch(None, check_cycles=True, packed=pk, copy=copy)
        assert len(recs) == len(nodes)
        assert np.array_equal(bits(recs), bits(want))
        for i in range(len(nodes)):
            assert results[i].optimal == res_c[i].optimal and (not res_c[i].optimal or results[i].evaluation == res_c[i].evaluation)
    t.close()


def _tableau(lib, model, cap=8, precision=None):
    m = Model(model)
    mat, vibr, vibc = m.build_tableau()
    t = Tableau(mat, vibr, vibc, m.unrestricted, precision=precision or m.precision, row_capacity=mat.shape[0] + cap, lib=lib)
    t.applyCuts([])
    t.save()
    return t, m


TIES = {"optimize": "v", "opType": "max", "constraints": {"a": {"max": 5}, "b": {"max": 5}},
        "variables": {"x": {"v": 1, "a": 2}, "y": {"v": 1, "b": 2}}, "ints": {"x": 1, "y": 1}}  # x = y = 2.5
NEG = {"optimize": "v", "opType": "min", "constraints": {"a": {"min": -5}, "b": {"min": -7}},
       "variables": {"x": {"v": 1, "a": 2}, "y": {"v": 1, "b": 2}}, "ints": {"x": 1, "y": 1}, "unrestricted": {"x": 1, "y": 1}}
UNBOUNDED = {"optimize": "v", "opType": "max", "constraints": {"a": {"min": 1}}, "variables": {"x": {"v": 1, "a": 1}}, "ints": {"x": 1}}


def _check(t, nodes, watched):
    """the device's records == the restatement of the compact read-back of the same nodes; returns the records"""
    t.set_watched_variables(watched)
    res_c, rows, vals = t.applyCutsBatchWatched(nodes)
    want = branch_record_from_watched([res_c[i] for i in range(len(nodes))], rows[:len(nodes)], vals[:len(nodes)], watched, t.precision)
    for k in range(len(nodes)):  # one node per call (the single-node shapes) ...
        _r, one = t.applyCutsBatchBranch([nodes[k]])
        assert np.array_equal(bits(one), bits(want[k:k + 1])), k
    _r, recs = t.applyCutsBatchBranch(nodes)  # ... and all of them in one call
    assert np.array_equal(bits(recs), bits(want))
    return recs


def test_edge_ties_equal_fractions_precision_and_integral_nodes(hip_lib):
    t, m = _tableau(hip_lib, TIES)
    x, y = (int(v) for v in m.integer_index_array)
    nodes = [[], [{"type": "max", "varIndex": x, "value": 2.0}], [{"type": "max", "varIndex": x, "value": 2.0}, {"type": "max", "varIndex": y, "value": 2.0}],
             [{"type": "min", "varIndex": x, "value": 100.0}]]
    recs = _check(t, nodes, [x, y])
    assert recs["branch_var_index"][0] == x and recs["branch_var_value"][0] == 2.5 and not recs["flags"][0] & _capi.BRANCH_INTEGRAL  # equal: the first
    assert recs["branch_var_index"][1] == y and recs["branch_var_value"][1] == 2.5
    assert recs["branch_var_index"][2] == -1 and recs["branch_var_value"][2] == 0.0 and recs["flags"][2] & _capi.BRANCH_INTEGRAL  # all integral
    assert not recs["flags"][3] & _capi.BRANCH_FEASIBLE  # infeasible: still a record, from the node's final column
    recs = _check(t, nodes[:1], [y, x])  # the earlier in REGISTRATION order wins
    assert recs["branch_var_index"][0] == y
    t.close()
    # a fraction equal to the precision is integral (strict >), and still the most fractional variable (> 0)
    t, m = _tableau(hip_lib, TIES, precision=0.5)
    recs = _check(t, [[]], [x, y])
    assert recs["flags"][0] & _capi.BRANCH_INTEGRAL and recs["branch_var_index"][0] == x
    t.close()


def test_edge_negative_half_rounds_up(hip_lib):
    t, m = _tableau(hip_lib, NEG)
    x, y = (int(v) for v in m.integer_index_array)
    recs = _check(t, [[{"type": "min", "varIndex": x, "value": 100.0}]], [x, y])
    # y = -3.5: Math.round(-3.5) = -3, fraction 0.5
    assert recs["flags"][0] & _capi.BRANCH_FEASIBLE and recs["branch_var_index"][0] == y and recs["branch_var_value"][0] == -3.5
    t.close()


def test_edge_unbounded_node(hip_lib):
    t, m = _tableau(hip_lib, UNBOUNDED)
    recs = _check(t, [[]], list(m.integer_index_array))
    assert not recs["flags"][0] & _capi.BRANCH_BOUNDED and recs["unbounded_var_index"][0] >= 0
    results = t.results_from_branch_records(recs, 1)
    assert results[0].evaluation == float("-inf")
    t.close()


def test_edge_long_watched_list_with_duplicates(hip_lib):
    """more watched entries than a workgroup has threads (the per-thread loop), the same variables listed many times (no position map):
    the first listed occurrence of the most fractional variable wins"""
    t, m = _tableau(hip_lib, TIES, cap=1400)
    x, y = (int(v) for v in m.integer_index_array)
    nodes = [[], [{"type": "max", "varIndex": x, "value": 2.0}], [{"type": "max", "varIndex": x, "value": 2.0}, {"type": "max", "varIndex": y, "value": 2.0}]]
    watched = [x] * 700 + [y] * 500 + [x, y] * 50
    assert len(watched) > 1024
    recs = _check(t, nodes, watched)
    assert list(recs["branch_var_index"]) == [x, y, -1]
    t.close()


@pytest.mark.parametrize("name", ["Monster_II", "LargeFarmMIP", "Knapsack_1", "Sudoku4x4"])
def test_speculative_tree_on_branch_records(hip_lib, name, monkeypatch):
    g = G.load(os.path.join(G.GOLDEN, "fixtures", name + ".json.gz"))
    ref = {k: (G.num(v) if not isinstance(v, bool) else v) for k, v in g["result"].items()}
    monkeypatch.setenv("JSLP_TREE_BRANCH", "1")
    out = Solve(g["model"], full=True, lib=hip_lib, speculate=16)
    assert out["result"] == ref and out["iter"] == g["final"]["branchAndCutIterations"]
