"""A node's MIR loop inside ONE engine call on the GPU (jslpr_engine_relax_mir, include/jslpr_mir.h): every launch shape against the oracle
library's composition of the existing calls (applyCuts + mirRound + the volume rule, tests/test_mir_one_call.by_hand), node by node and
bit for bit -- results, outcome records, RHS columns, row maps, the live tableau, the pivot trace, the error codes, and that a call whose
plain twin is one launch of an LDS node kernel is one launch too.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
from jslpsolver_amd import Tableau, _capi
from test_mir_cuts import case_id
from test_mir_one_call import (DEFAULT_CASES, MIR_CASES, check_evaluation_kept, check_no_incumbent, check_speculative, expectations, load_nodes, root_tableau, run_case, same_node, u64)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = {"LargeFarmMIP": 400, "Monster_II": None, "Knapsack_1": None}
MODES = {"default": (-1, False), "incremental": (3, True)}
_cache = {}


def expected(oracle_lib, name, mode):
    """(tableau, nodes, root evaluation, per-node expectations) of an input, computed once"""
    if (name, mode) not in _cache:
        tab, nodes = load_nodes(name, INPUTS[name])
        _cache[(name, mode)] = (tab, nodes) + expectations(oracle_lib, tab, nodes, *MODES[mode])
    return _cache[(name, mode)]


def test_the_inputs_are_what_the_cases_need(oracle_lib):
    tab, nodes, _, ex = expected(oracle_lib, "LargeFarmMIP", "default")
    rounds = [x for e in ex for x in e["per_round"]]
    assert (tab["height"], tab["width"], len(nodes)) == (36, 101, 400)
    assert (min(e["record"][0] for e in ex), max(e["record"][0] for e in ex), max(e["record"][1] for e in ex)) == (1, 7, 60)
    assert sum(1 for c, _ in rounds if c > 10) == 61 and sum(1 for _, n in rounds if n == 10) == 107
    tab, nodes, _, ex = expected(oracle_lib, "Monster_II", "default")
    rounds = [x for e in ex for x in e["per_round"]]
    assert (tab["height"], tab["width"], len(nodes)) == (935, 925, 151) and 2 * len(nodes) > 256
    assert sum(1 for e in ex if not e["res"].feasible and not e["sets"]) == 14 and sum(1 for _, n in rounds if n == 0) == 104
    assert max(e["record"][1] for e in ex) == 16
    assert sum(1 for e in expected(oracle_lib, "Monster_II", "incremental")[3] if e["record"][0] == 0) == 14  # need_feasible keeps them out
    tab, nodes, _, ex = expected(oracle_lib, "Knapsack_1", "default")
    assert (tab["height"], tab["width"], len(nodes)) == (52, 51, 79) and tab["height"] < 64


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(INPUTS))
def test_every_batch_size(hip_lib, oracle_lib, name, mode):
    """1 node, 2, 16, all, all twice over; then the same engine once more, reversed (slot reuse)"""
    tab, nodes, root_eval, ex = expected(oracle_lib, name, mode)
    max_rounds, need_feasible = MODES[mode]
    rounds = None if max_rounds < 0 else max_rounds
    t = root_tableau(hip_lib, tab, nodes)
    assert u64(t.evaluation)[()] == u64(root_eval)[()]
    prev = t.evaluation
    got = t.applyCutsMIR(nodes[0], max_rounds=rounds, need_feasible=need_feasible)
    same_node(got, ex[0], prev)
    t.restore()
    engine_eval = got[0].evaluation  # (the engine's own evaluation is the last node's: what a later node keeps)
    for idx in (list(range(2)), list(range(16)), list(range(len(nodes))), list(range(len(nodes))) * 2, list(range(len(nodes)))[::-1]):
        results, ocs, rhs, vibr = t.applyCutsBatchMIR([nodes[i] for i in idx], max_rounds=rounds, need_feasible=need_feasible)
        for k, i in enumerate(idx):
            same_node((results[k], ocs[k], rhs[k], vibr[k]), ex[i], engine_eval)
        engine_eval = results[-1].evaluation
    t.close()


def test_plain_calls_after_mir_batches(hip_lib, oracle_lib):
    """the slots the MIR builds leave behind serve the plain node kernels: a plain batch and a plain node after restore() equal a fresh engine's"""
    tab, nodes, _, _ = expected(oracle_lib, "Monster_II", "default")
    fresh = root_tableau(oracle_lib, tab, nodes)
    want_res, want_rhs, want_rows = fresh.applyCutsBatch(nodes)
    fresh.restore()
    one_res, one_rhs, one_rows = fresh.applyCuts(nodes[3])
    fresh.close()
    t = root_tableau(hip_lib, tab, nodes)
    t.applyCutsBatchMIR(nodes)
    t.applyCutsBatchMIR(nodes[::-1])
    res, rhs, rows = t.applyCutsBatch(nodes)
    for i in range(len(nodes)):
        h = want_res[i].height
        a, b = res[i].as_dict(), want_res[i].as_dict()
        a.pop("evaluation"), b.pop("evaluation")  # (what a node without an optimum keeps is the engine's evaluation before the call)
        assert a == b
        assert np.array_equal(u64(rhs[i, :h]), u64(want_rhs[i, :h])) and np.array_equal(rows[i, :h], want_rows[i, :h])
    t.restore()
    r, x, w = t.applyCuts(nodes[3])
    assert r.as_dict() == one_res.as_dict() and np.array_equal(u64(x), u64(one_rhs)) and np.array_equal(w, one_rows)
    t.close()


@pytest.mark.parametrize("name", ["Knapsack_1", "Monster_II"])
def test_one_node_from_a_checkpoint(hip_lib, oracle_lib, name):
    tab, nodes, _, _ = expected(oracle_lib, name, "incremental")
    base = next(n for n in nodes if 0 < len(n) < max(len(x) for x in nodes))
    ints = tab["integerVarIndexes"]
    outs = []
    for lib in (oracle_lib, hip_lib):
        t = root_tableau(lib, tab, nodes)
        _res, rhs, vibr = t.applyCuts(base)
        ck = t.createCheckpoint()
        # one more cut, on the first integer variable that is basic and fractional in the checkpointed node
        row = next(r for r in range(1, len(vibr)) if int(vibr[r]) in ints and abs(rhs[r] - round(rhs[r])) > 1e-6)
        cut = {"type": "max", "varIndex": int(vibr[row]), "value": float(np.floor(rhs[row]))}
        trace0 = len(t.pivot_trace())
        res, oc, x, w = t.applyCutsMIR([cut], max_rounds=3, need_feasible=True, checkpoint=ck)
        m, vr, vc, rbv, cbv = t.download()
        trace = t.pivot_trace()
        assert len(trace) - trace0 == int(oc["pivots"])
        outs.append((res.as_dict(), tuple(int(oc[k]) for k in ("rounds", "rows_added", "optimal_count", "pivots")),
                     u64(oc["volume_before"]).tobytes() + u64(oc["volume_after"]).tobytes(), x.tobytes(), w.tobytes(), m.tobytes(), vr.tobytes(), vc.tobytes(),
                     rbv[:int(max(vr.max(), vc.max())) + 1].tobytes(), cbv[:int(max(vr.max(), vc.max())) + 1].tobytes(), trace.tobytes(), t.evaluation, t.feasible, t.simplexIters))
        t.releaseCheckpoint(ck)
        t.close()
    assert outs[0][1][0] >= 1  # the loop ran
    for a, b in zip(outs[0], outs[1]):
        assert a == b


def test_live_tableau_and_trace_after_one_node(hip_lib, oracle_lib):
    tab, nodes, _, ex = expected(oracle_lib, "Knapsack_1", "default")
    i = max(range(len(nodes)), key=lambda k: ex[k]["record"][1])
    outs = []
    for lib in (oracle_lib, hip_lib):
        t = root_tableau(lib, tab, nodes)
        t.applyCuts(nodes[0])  # (slot 0 in sync with the saved root: the next node is the one-launch shape)
        t.applyCutsMIR(nodes[i])
        m, vr, vc, _, _ = t.download()
        outs.append((m.tobytes(), vr.tobytes(), vc.tobytes(), t.pivot_trace().tobytes(), t.height))
        t.close()
    assert outs[0] == outs[1]


def test_evaluation_kept_when_a_later_round_ends_infeasible_on_gpu(hip_lib, oracle_lib, monkeypatch):
    check_evaluation_kept(hip_lib, oracle_lib, monkeypatch)


def test_tree_without_an_incumbent_on_gpu(hip_lib, oracle_lib, monkeypatch):
    check_no_incumbent(hip_lib, oracle_lib, monkeypatch)


def test_errors(hip_lib, oracle_lib):
    tab, nodes, root_eval, ex = expected(oracle_lib, "Knapsack_1", "default")
    m, vibr, vibc = G.dense_tableau(tab)
    longest = max(len(n) for n in nodes)
    i = max(range(len(nodes)), key=lambda k: ex[k]["record"][1])  # the node that adds the most MIR rows
    # too small a row capacity: the node's branching cuts fit, its MIR rows do not
    assert ex[i]["record"][1] > 1
    small = Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], row_capacity=tab["height"] + len(nodes[i]) + 1, lib=hip_lib,
                    integer_variables=tab["integerVarIndexes"])
    small.applyCuts([])
    small.save()
    fresh = root_tableau(oracle_lib, tab, nodes)
    want = fresh.applyCuts(nodes[i])
    fresh.close()
    small.applyCutsBatch([nodes[i]] * 2)  # (two slots in sync with the saved root: the calls below are the one-launch shapes)
    for call in (lambda: small.applyCutsMIR(nodes[i]), lambda: small.applyCutsBatchMIR([nodes[i]] * 2)):
        with pytest.raises(_capi.EngineError, match=r"\(%d\)" % _capi.JSLP_ERR_CAPACITY):
            call()
        small.restore()
        got = small.applyCuts(nodes[i])
        assert got[0].as_dict() == want[0].as_dict() and np.array_equal(u64(got[1]), u64(want[1])) and np.array_equal(got[2], want[2])
        small.applyCutsBatch([nodes[i]] * 2)
    small.close()
    t = root_tableau(hip_lib, tab, nodes)
    ck = t.createCheckpoint()
    offs = np.array([0, 0, 0], dtype=np.int32)
    out = (_capi.SimplexResult * 2)()
    ocs = np.zeros(2, dtype=_capi.MIR_OUTCOME_DTYPE)
    rc = hip_lib.jslpr_engine_relax_mir(t._h, ck["id"], 2, _capi.ptr_i32(offs), None, None, None, 1, -1, 0, out, ocs.ctypes.data, None, None, t.row_capacity)
    assert rc == _capi.JSLP_ERR_ARG
    t.close()
    plain = Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], row_capacity=tab["height"] + 340, lib=hip_lib)
    plain.applyCuts([])
    with pytest.raises(_capi.EngineError, match=r"\(%d\)" % _capi.JSLP_ERR_STATE):
        plain.applyCutsMIR(nodes[0])
    plain.close()
    oo = np.zeros((1, tab["width"]))
    oo[0, 1] = 1.0
    opt = Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], row_capacity=tab["height"] + 340, lib=hip_lib, optional_objectives=oo,
                  integer_variables=tab["integerVarIndexes"])
    opt.applyCuts([])
    with pytest.raises(_capi.EngineError, match=r"\(%d\)" % _capi.JSLP_ERR_UNSUPPORTED):
        opt.applyCutsMIR(nodes[0])
    opt.close()


@pytest.mark.parametrize("group_max", [None, 64])
def test_one_launch(tmp_path, group_max):
    """a worker process under JSLP_DEBUG_LAUNCH=1 (the node-path knobs are latched per process): a 1-node, a 16-node and a 302-node Monster_II
    call print exactly one node-kernel line each, a MIR build's; with JSLP_GROUP_MAX=64 the 302 nodes go through the queue kernel"""
    env = dict(os.environ, JSLP_DEBUG_LAUNCH="1")
    if group_max:
        env["JSLP_GROUP_MAX"] = str(group_max)
    log = tmp_path / "stderr.txt"
    with open(log, "w") as fh:
        p = subprocess.run([sys.executable, os.path.join(HERE, "mir_launch_worker.py")], env=env, stderr=fh, stdout=subprocess.PIPE, text=True, timeout=120)
    text = open(log).read()
    assert p.returncode == 0, text[-3000:]
    calls = [c.split("### end")[0] for c in text.split("### mir call ")[1:]]
    assert [c.split("\n")[0] for c in calls] == ["1", "16", "302"]
    lines = [[l for l in c.split("\n")[1:] if l.startswith("[jslp] launch")] for c in calls]
    assert all(len(l) == 1 and "mir 1" in l[0] for l in lines), lines
    assert "k_node_lds<1024,opt 0,cow 0,mir 1> g 1 " in lines[0][0] and "k_node_lds<1024,opt 0,cow 0,mir 1> g 16 " in lines[1][0]
    if group_max:
        assert "k_node_queue<512,cow 0,opt 0,mir 1> g 64 n 302 " in lines[2][0]
    else:  # (one group when the chip keeps 302 workgroups of this tableau resident, else the queue)
        assert "k_node_lds<512,opt 0,cow 0,mir 1> g 302 " in lines[2][0] or "k_node_queue<512,cow 0,opt 0,mir 1> " in lines[2][0]


@pytest.mark.parametrize("case", MIR_CASES, ids=case_id)
def test_trees_with_one_call_per_node_on_gpu(hip_lib, case, monkeypatch):
    monkeypatch.setenv("JSLP_TREE_MIR", "1")
    run_case(hip_lib, case)


@pytest.mark.parametrize("case", DEFAULT_CASES, ids=case_id)
def test_speculative_mir_tree_on_gpu(hip_lib, case):
    check_speculative(hip_lib, case, specs=(8,))
