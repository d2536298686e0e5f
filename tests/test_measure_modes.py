"""The engine's two measurement modes -- jslp_engine_set_counting (bench.py's gated-bytes roofline) and jslp_engine_set_timing (the timed
steps of every published figure) -- on every launch shape: the answers stay the oracle's bit for bit, the work counters equal an
independent count of the pivot trace (tests/measure_modes.py) assembled by the contract of include/jslp_engine.h, and the timing values
count what that contract says they count.  Milliseconds are checked for sign and ordering only.

CPU part: the instances have the properties the GPU cases rely on, and the independent count equals the oracle's own counters."""
import hashlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import measure_modes as M
import test_engine_lifecycle as L
import test_node_edges as N
from jslpsolver_amd.engine import DevicePool, simplex_many
from test_selection_edges import KNOBS, PLAIN, UNR_MODES, _canon

ROOT_SPEC = L.spec(40, 30, 60, 1)
COMPARED = ("relaxations", "simplex_calls", "pivots", "gated_cells", "gated_rows", "cut_rows", "height_sum")
EAGER = "restore+add_cuts+simplex+gather "
LABELS = ["single 1", "single 2", "batch 20", "batch 300", "batch 300 again", "batch 1100", "batch 1100 again", "watched 20", "branch 20", "relax_from", "pool 300"]
_WANT = {}


def want(oracle_lib, name):
    """the oracle's counted solve of an instance and the independent count of its trace, computed once"""
    if name not in _WANT:
        inst = M.instance(name)
        t = M.tableau(oracle_lib, inst)
        try:
            t.set_counting(True)
            res = t.simplex(check_cycles=inst["check"])
            ans = M.full_answer(t, res)
            counters, trace, H = t.get_counters(), t.pivot_trace().copy(), t.height
        finally:
            t.close()
        count, final = M.replay_count(oracle_lib, inst, trace)
        _WANT[name] = dict(inst=inst, ans=ans, counters=counters, count=count, p1=res.pivots_phase1, p2=res.pivots_phase2, H=H, W=inst["A"].shape[1],
                           final=final, res=res.as_dict())
    return _WANT[name]


# ---- CPU: the instances and the count ------------------------------------------------------------------------------------------------
def test_instance_s_has_what_the_gpu_cases_need(oracle_lib):
    w = want(oracle_lib, "S")
    res, count = w["res"], w["count"]
    assert (w["H"], w["W"]) == (257, 801)
    assert res["feasible"] and res["bounded"] and res["optimal"] and res["cycle_phase"] == 0, res
    assert w["p1"] > 0  # k_fused_p1 has pivots to report
    assert w["p2"] > 1520  # the fused chunk (16, doubling: 16 + .. + 256 = 496) reaches its cap of 512 twice: the event pool grows to 1024
    gated, nz, dense = (M.totals(count, rule) for rule in ("gated", "nz", "dense"))
    assert len({gated[0], nz[0], dense[0]}) == 3 and len({gated[1], nz[1], dense[1]}) == 3, (gated, nz, dense)  # no rule passes for another
    for lo, hi in ((0, w["p1"]), (w["p1"], None)):  # ... in either phase
        assert M.totals(count, "gated", lo, hi) != M.totals(count, "dense", lo, hi)
    assert count["tiny_col"].sum() > 0 and count["tiny_row"].sum() > 0
    assert count["undecidable"].sum() == 0  # every pivot of a fused pipeline is the pipeline's own


@pytest.mark.parametrize("name", ("S", "S+unr", "S+opt") + M.SLOW + M.MANY)
def test_independent_count_equals_the_oracles_counters(oracle_lib, name):
    w = want(oracle_lib, name)
    c = w["counters"]
    assert w["res"]["feasible"] and w["res"]["optimal"] and w["res"]["cycle_phase"] == 0
    assert len(w["count"]) == c["pivots"] == w["p1"] + max(w["p2"], 0)
    assert M.totals(w["count"], "gated") == (c["gated_rows"], c["gated_cells"])
    assert (c["simplex_calls"], c["relaxations"], c["height_sum"]) == (1, 0, w["H"])
    assert hashlib.sha256(_canon(w["final"])).hexdigest() == w["ans"]["arrays"][0]  # the replay ends on the solve's final tableau
    assert M.expected_counters(w["count"], w["p1"], w["H"], "wg")["gated_cells"] == c["gated_cells"]


def test_variants_of_s_differ_from_it_where_they_should(oracle_lib):
    s, unr, opt = (want(oracle_lib, n) for n in ("S", "S+unr", "S+opt"))
    assert unr["ans"]["trace"] != s["ans"]["trace"] and unr["p1"] > 0 and unr["p2"] > 0
    assert opt["ans"]["objectives"] != _canon(opt["inst"]["oo"])  # the objective rows were pivoted on


@pytest.mark.parametrize("name", M.SLOW)
def test_undecidable_instances_hold_exactly_that_pivot(oracle_lib, name):
    w = want(oracle_lib, name)
    assert len(w["count"]) == 1 and w["count"]["undecidable"][0] == 1
    assert (w["p1"], max(w["p2"], 0)) == ((1, 0) if name.startswith("slow_p1") else (0, 1))
    assert M.totals(w["count"], "gated") != M.totals(w["count"], "dense")


# ---- GPU: simplex() ------------------------------------------------------------------------------------------------------------------
OPT_MODES = ("auto", "wg", "wggen", "sp", "fused", "resident")  # the shapes with a build for optional objectives


def _simplex_params():
    out = [("S", m) for m in PLAIN]
    out += [("S+unr", m) for m in UNR_MODES]
    out += [("S+opt", m) for m in OPT_MODES]
    out += [(n, "fused") for n in M.SLOW]
    out += [(n, "g3") for n in M.SLOW if n.startswith("slow_p1")]  # a register-resident phase 2 behind a fused phase 1 with a handed-over pivot
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", _simplex_params(), ids=["%s-%s" % p for p in _simplex_params()])
def test_simplex_under_counting_and_timing(hip_lib, hip_hooks_lib, oracle_lib, monkeypatch, name, mode):
    """four solves on fresh engines, counting off / on x timing off / on: the oracle's answer, the launch shape the mode names, the contract's
    counters and launch count each time (measure_modes.run_case)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in M.mode_env(mode).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    M.run_case(hip_hooks_lib if mode == "xl" else hip_lib, name, mode, want(oracle_lib, name))


@pytest.mark.gpu
def test_simplex_with_phase_1_through_select_and_update(oracle_lib, tmp_path):
    """JSLP_FUSED_P1=0 (latched per process: a worker): phase 1 is k_select + k_update's and counted through the gate, phase 2 is k_pivot_fused's"""
    wants = {n: {k: want(oracle_lib, n)[k] for k in ("inst", "ans", "count", "p1", "p2", "H")} for n in ("S", "S+unr", "S+opt")}
    plan = tmp_path / "wants.pkl"
    plan.write_bytes(pickle.dumps(wants))
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(M.mode_env("fused-p1off"), JSLP_DEBUG_LAUNCH="1")
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "measure_modes_worker.py"), str(plan)], env=env,
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-6000:])
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-3000:] + out.stderr[-5000:]


@pytest.mark.gpu
def test_simplex_many_counts_every_engine_on_its_own(hip_lib, oracle_lib, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    ws = [want(oracle_lib, n) for n in M.MANY]
    ts = [M.tableau(hip_lib, w["inst"]) for w in ws]
    try:
        for t in ts:
            t.set_counting(True)
        results = simplex_many(ts, check_cycles=[w["inst"]["check"] for w in ws])
        for n, t, r, w in zip(M.MANY, ts, results, ws):
            assert t.last_path() == "workgroup-many", n
            assert M.full_answer(t, r) == w["ans"], n
            c, exp = t.get_counters(), M.expected_counters(w["count"], w["p1"], w["H"], "many")
            assert {k: c[k] for k in M.WORK_FIELDS + M.HEALTH_FIELDS} == exp, n
    finally:
        for t in ts:
            t.close()


# ---- GPU: node calls -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def node_root(oracle_lib):
    root = L.plan_root(oracle_lib, ROOT_SPEC)
    # the child of the checkpoint: a cut list that reaches an optimum from the checkpointed node too
    t = N.tableau(oracle_lib, root)
    try:
        t.simplex(True)
        t.save()
        t.applyCuts(root["good"][0])
        ck = t.createCheckpoint()
        root["child"] = next(cuts for cuts in root["good"][1:] if len(cuts) == 1 and cuts[0]["varIndex"] != root["good"][0][0]["varIndex"] and
                             t.applyCutsFrom(ck, [cuts])[0][0].optimal)
    finally:
        t.close()
    return root


def _node_script(lib, root, counting, timing):
    """-> per call (label, outcomes, counters, timing, launch lines); the pool's call reads the pool's counters"""
    steps = []
    t = N.tableau(lib, root)
    try:
        t.simplex(True)
        t.save()
        t.set_watched_variables(root["watch"])
        if counting:
            t.set_counting(True)
        if timing:
            t.set_timing(True)
        good = root["good"]
        mixed = good + [[]]  # (a node without cuts leaves the root's rows alone: where a batch starts from copies in sync, the product restores less)

        def step(label, call, counters=None):
            with M.StderrLines() as err:
                outcomes = call()
            steps.append(dict(label=label, outcomes=outcomes, counters=(counters or t.get_counters)(), timing=t.get_timing() if timing else None,
                              lines=err.launches()))

        def watched():
            out, rows, vals = t.applyCutsBatchWatched(L.cycled(mixed, 20, 3))
            return [(out[i].as_dict(), rows[i].tobytes(), vals[i].tobytes()) for i in range(20)]

        def branch():
            results, recs = t.applyCutsBatchBranch(L.cycled(mixed, 20, 4))
            return np.ascontiguousarray(recs).tobytes(), [(r.feasible, r.bounded, r.optimal, r.height, r.evaluation) for r in results[:20]]

        def from_checkpoint():
            t.restore()
            first = L.node_obs(*t.applyCuts(good[0]))
            ck = t.createCheckpoint()
            try:
                return [first] + [L.node_obs(*x) for x in t.applyCutsFrom(ck, [root["child"]])]
            finally:
                t.releaseCheckpoint(ck)

        step("single 1", lambda: [L.node_obs(*t.applyCuts(good[0]))])
        step("single 2", lambda: [L.node_obs(*t.applyCuts(good[1]))])
        step("batch 20", lambda: L.batch_obs(t, L.cycled(mixed, 20, 1)))
        # a batch starts from tableau copies in sync with the saved root or fills them first (the eager sequence): every size twice.  1100 nodes are
        # more than the chip keeps workgroups of the queue kernel resident (at most 4 of 512 threads on each of 256 CUs): the second goes through it
        step("batch 300", lambda: L.batch_obs(t, L.cycled(mixed, 300, 2)))
        step("batch 300 again", lambda: L.batch_obs(t, L.cycled(mixed, 300, 2)))
        step("batch 1100", lambda: L.batch_obs(t, L.cycled(mixed, 1100, 5)))
        step("batch 1100 again", lambda: L.batch_obs(t, L.cycled(mixed, 1100, 5)))
        step("watched 20", watched)
        step("branch 20", branch)
        step("relax_from", from_checkpoint)
        if counting and not timing:
            t.restore()
            pool = DevicePool(t, [0, 0])
            try:
                pool.set_counting(True)

                def pooled():
                    out, rhs, rows = pool.applyCutsBatch(L.cycled(mixed, 300, 2))
                    return [L.node_obs(out[i], rhs[i], rows[i]) for i in range(300)]

                step("pool 300", pooled, pool.get_counters)
            finally:
                pool.close()
        if timing:
            t.set_timing(True)
            steps.append(dict(label="set_timing again", timing=t.get_timing()))
        return steps
    finally:
        t.close()


@pytest.fixture(scope="module")
def oracle_nodes(oracle_lib, node_root):
    return _node_script(oracle_lib, node_root, True, False)


def test_node_script_on_the_oracle(oracle_nodes, node_root):
    """every node reaches an optimum, and the counters move with every call"""
    assert [s["label"] for s in oracle_nodes] == LABELS
    for s in oracle_nodes[:7] + oracle_nodes[9:]:
        assert all(o["optimal"] and o["feasible"] and o["bounded"] for o in s["outcomes"]), s["label"]
    relax = [s["counters"]["relaxations"] for s in oracle_nodes]
    assert relax == [1, 2, 22, 322, 622, 1722, 2822, 2842, 2862, 2864, 300]
    for a, b in zip(oracle_nodes[:9], oracle_nodes[1:10]):
        assert all(b["counters"][k] > a["counters"][k] for k in COMPARED), (a["label"], b["label"])


@pytest.mark.gpu
def test_node_calls_count_what_the_oracle_counts(hip_lib, oracle_nodes, node_root, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    got = _node_script(hip_lib, node_root, True, False)
    queue_before = 0
    for g, w in zip(got, oracle_nodes):
        print(g["label"], g["lines"], g["counters"])
        assert g["label"] == w["label"]
        assert g["outcomes"] == w["outcomes"], g["label"]
        for k in COMPARED:
            assert g["counters"][k] == w["counters"][k], (g["label"], k, g["counters"], w["counters"])
        # the restore differs by design: the product brings back the rows a node dirtied, the oracle every row.  The eager sequence restores the
        # whole root too, and on this small dense root the second child finds every row dirtied: equal until a batch starts from copies in sync
        if LABELS.index(g["label"]) < LABELS.index("batch 300 again"):
            assert g["counters"]["restored_rows"] == w["counters"]["restored_rows"] > 0, g["label"]
        elif g["label"] == "pool 300":  # (new members: their first batch fills their copies)
            assert 0 < g["counters"]["restored_rows"] <= w["counters"]["restored_rows"], g["label"]
        else:
            assert 0 < g["counters"]["restored_rows"] < w["counters"]["restored_rows"], g["label"]
        assert g["counters"]["node_queue_launches"] == queue_before + (g["label"] == "batch 1100 again"), (g["label"], g["counters"])
        queue_before = g["counters"]["node_queue_launches"] if g["label"] != "relax_from" else 0  # (the pool's counters start over)
    # the launch shapes the script is meant to run: several launches, the polled single-child kernel, one launch per group, the queue kernel
    lines = {g["label"]: g["lines"] for g in got}
    assert len(lines["single 1"]) == 1 and lines["single 1"][0].startswith(EAGER), lines["single 1"]
    assert len(lines["single 2"]) == 1 and lines["single 2"][0].startswith("k_node_lds<1024,"), lines["single 2"]
    # (of the first 1100 nodes only as many as the queue kernel has slots start eagerly: the rest finds copies in sync by then)
    assert all(x.startswith(EAGER) for x in lines["batch 300"]) and lines["batch 1100"][0].startswith(EAGER), lines
    assert len(lines["batch 300 again"]) == 1 and lines["batch 300 again"][0].startswith("k_node_lds<512,"), lines["batch 300 again"]
    assert len(lines["batch 1100 again"]) == 1 and lines["batch 1100 again"][0].startswith("k_node_queue<512,"), lines["batch 1100 again"]
    assert len(got) == len(oracle_nodes)


@pytest.mark.gpu
@pytest.mark.parametrize("counting", [False, True])
def test_timed_node_calls_run_the_eager_sequence(hip_lib, oracle_nodes, node_root, monkeypatch, counting):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    got = _node_script(hip_lib, node_root, counting, True)
    total = 0.0
    for g, w in zip(got[:-1], oracle_nodes):
        print(g["label"], g["lines"], g["counters"], g["timing"])
        assert g["label"] == w["label"]
        assert g["outcomes"] == w["outcomes"], g["label"]
        assert g["lines"] and all(x.startswith(EAGER) for x in g["lines"]), (g["label"], g["lines"])
        if counting:
            for k in COMPARED:
                assert g["counters"][k] == w["counters"][k], (g["label"], k)
        upd_ms, launches, total_ms = g["timing"]
        assert total_ms > total and launches == 0 and upd_ms == 0.0, (g["label"], g["timing"], total)  # (one-workgroup kernels: no update launches)
        total = total_ms
    assert got[-1]["label"] == "set_timing again" and got[-1]["timing"] == (0.0, 0, 0.0)


# ---- GPU: a node with its MIR loop -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mir_node(oracle_lib):
    """Knapsack_1's first recorded node whose MIR loop runs more than one round, by hand on the oracle with counting on"""
    import test_mir_one_call as R
    tab, nodes = R.load_nodes("Knapsack_1")
    ints = set(tab["integerVarIndexes"])
    for i, cuts in enumerate(nodes):
        ref = R.root_tableau(oracle_lib, tab, nodes)
        try:
            prev = ref.evaluation
            ref.set_counting(True)
            e = R.by_hand(ref, ints, cuts, -1, False)
            c = ref.get_counters()
        finally:
            ref.close()
        if e["record"][0] > 1 and e["record"][1] > 0:
            return dict(tab=tab, nodes=nodes, i=i, expect=e, counters=c, prev=prev)
    raise AssertionError("no node with a MIR loop of several rounds")


def test_mir_node_by_hand_counts_its_simplexes(mir_node):
    e, c = mir_node["expect"], mir_node["counters"]
    assert c["simplex_calls"] == 1 + e["record"][0] and c["pivots"] == e["record"][3] and c["relaxations"] == 1
    assert c["height_sum"] > c["simplex_calls"] * mir_node["tab"]["height"]  # (the heights grow with the cuts and the MIR rows)


@pytest.mark.gpu
@pytest.mark.parametrize("measure", ["counting", "timing"])
def test_mir_node_call_under_counting_and_timing(hip_lib, mir_node, monkeypatch, measure):
    import test_mir_one_call as R
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    t = R.root_tableau(hip_lib, mir_node["tab"], mir_node["nodes"])
    try:
        t.applyCuts(mir_node["nodes"][0])  # (slot 0 in sync with the saved root: untimed, the next node is the one-launch shape)
        t.restore()
        if measure == "counting":
            t.set_counting(True)
        else:
            t.set_counting(True)
            t.set_timing(True)
        got = t.applyCutsMIR(mir_node["nodes"][mir_node["i"]])
        R.same_node(got, mir_node["expect"], mir_node["prev"])
        c = t.get_counters()
        for k in ("simplex_calls", "pivots", "height_sum"):
            assert c[k] == mir_node["counters"][k], (k, c, mir_node["counters"])
        if measure == "timing":
            assert t.get_timing()[2] > 0
    finally:
        t.close()
