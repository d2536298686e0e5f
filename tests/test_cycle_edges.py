"""checkForCycles (simplex.ts:415-440) at the history lengths where its implementations change code paths.

The one-workgroup LDS kernels (jslp_wglds.hip.h) test histories shorter than WGL_HIST = 128 pairs in wave 0 on an LDS copy and longer
ones block-wide on the global copy; the lean register-resident kernel (jslp_resident_pipe.hip.h) keeps pairs 0..4095 in LDS and reads
later ones from the workgroup's global slice, behind a pair filter that decides whether the suffix test runs at all.  The instances of
tests/cycle_edges.py put a DETECTED cycle of the reference -- goldens recorded from the reference itself by
tests/golden/gen_golden_cycle_edges.js, tests/golden/cycle_edges/ -- on every side of both boundaries:

  boundary 128 (k fillers + a small cycling LP)          boundary 4096 (dense block + 650 / 600 / 700 fillers + a small cycling LP)
    below            deg_35358_k84, unr_3_k122 (127)       late_deg_292715_k650 (4091), late_deg_347708_k650 (4092), late_deg_35358_k600 (4064)
    n == B           deg_35358_k85, unr_3_k123,            late_deg_233528_k650 (+ _tall, _wide)
                     deg_233528_k103, deg_178868_k102
    n == B + 1       deg_35358_k86, unr_3_k124,            late_deg_178868_k650 (+ _tall, _wide)
                     deg_233528_k104, deg_178868_k103
    second copy      deg_35358_k87 (130)                   late_deg_398167_k650 (4101), late_deg_137788_k650 (4102)
    first copy       deg_35358_k100 (143)                  late_deg_35358_k650 (4114; + _tall, _wide)
    beyond           deg_35358_k110 (153)                  late_deg_35358_k700 (4164)

CPU (not marked gpu): the oracle equals every golden; the history rebuilt from the trace makes the literal restatement of the check
stop where the reference stopped and nowhere earlier; every instance sits in the class above; the runs of the 4096 set select
hundreds of pairs seen before that complete no square (the filter-says-seen, suffix-says-no path), some beyond pair 4096; the fillers
shift the base run by exactly k; the launch policy sends every case to the kernel it names.  The oracle's solves (31: every instance,
and the runs without fillers) are computed side by side the first time a test needs one: 80 s on 8 threads.
GPU: every instance through every kernel that keeps a history, each run against its golden to the bit, with the kernel that ran
read from the engine's JSLP_DEBUG_LAUNCH lines (a one-workgroup solve prints none: last_path() names it)."""
import os
import re
import subprocess
import sys
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np
import pytest

import cycle_edges as E
import golden_util as G
from jslpsolver_amd.engine import Tableau, pivot_digest, simplex_many
from test_cycle_goldens import _messages
from test_grid_edges import Inst as GridInst, _grid, _ld, _rpb, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "cycle_edges_worker.py")
KNOBS = ("JSLP_FORCE_PATH", "JSLP_RES_CPT", "JSLP_RES_LEAN", "JSLP_RES_GEOM", "JSLP_RES_RPB", "JSLP_RES_WIDE_TALL", "JSLP_XL", "JSLP_NO_WGLDS",
         "JSLP_NO_RESIDENT", "JSLP_INJECT_RESIDENT_ABORT_US", "JSLP_TEST_RESIDENT_LATE_WAVE0", "JSLP_TEST_RESIDENT_ABORT", "JSLP_WG_BATCH_THREADS")
LAUNCH = re.compile(r"^\[jslp\] launch (.*)$", re.M)

WHERE = {"deg_35358_k84": "below", "deg_35358_k85": "n == B", "deg_35358_k86": "n == B + 1", "deg_35358_k87": "second copy across",
         "deg_35358_k100": "first copy across", "deg_35358_k110": "beyond",
         "unr_3_k122": "below", "unr_3_k123": "n == B", "unr_3_k124": "n == B + 1", "unr_3_k125": "between the copies",
         "deg_233528_k103": "n == B", "deg_233528_k104": "n == B + 1", "deg_178868_k102": "n == B", "deg_178868_k103": "n == B + 1",
         "late_deg_292715_k650": "below", "late_deg_347708_k650": "below", "late_deg_233528_k650": "n == B", "late_deg_178868_k650": "n == B + 1",
         "late_deg_398167_k650": "second copy across", "late_deg_137788_k650": "second copy across", "late_deg_35358_k650": "first copy across",
         "late_deg_35358_k600": "below", "late_deg_35358_k700": "beyond",
         "late_deg_233528_k650_tall": "n == B", "late_deg_178868_k650_tall": "n == B + 1", "late_deg_35358_k650_tall": "first copy across",
         "late_deg_233528_k650_wide": "n == B", "late_deg_178868_k650_wide": "n == B + 1", "late_deg_35358_k650_wide": "first copy across"}
HIST_LEN = {"deg_35358_k84": 127, "deg_35358_k85": 128, "deg_35358_k86": 129, "deg_35358_k87": 130, "deg_35358_k100": 143, "deg_35358_k110": 153,
            "unr_3_k122": 127, "unr_3_k123": 128, "unr_3_k124": 129, "unr_3_k125": 130,
            "deg_233528_k103": 128, "deg_233528_k104": 129, "deg_178868_k102": 128, "deg_178868_k103": 129,
            "late_deg_292715_k650": 4091, "late_deg_347708_k650": 4092, "late_deg_233528_k650": 4096, "late_deg_178868_k650": 4097,
            "late_deg_398167_k650": 4101, "late_deg_137788_k650": 4102, "late_deg_35358_k650": 4114, "late_deg_35358_k600": 4064,
            "late_deg_35358_k700": 4164}
CLASSES = ("below", "n == B", "n == B + 1", "first copy across", "second copy across", "beyond")
LARGE = E.EDGE_4096 + E.TALL_WIDE
IDS = [i.name for i in E.INSTANCES]


# ---- instances and their goldens -----------------------------------------------------------------------------------------------
def golden(inst):
    return G.load(os.path.join(E.EDGES, "%s.json.gz" % inst.name))


@lru_cache(maxsize=3)  # (a large tableau is 22-29 MB: the parametrised tests below run instance by instance)
def built(inst):
    return E.build(inst)


def start_length(g):
    assert g["messages"][0] == "Cycle in phase 2", g["messages"]
    return int(g["messages"][1].split(":")[1]), int(g["messages"][2].split(":")[1])


def check_run(t, res, g, whole=True):
    """what test_cycle_goldens._check asserts of a finished solve"""
    call = g["simplexCalls"][0]
    assert _messages(res) == g["messages"]
    assert bool(res.feasible) == call["feasible"] is False
    assert (res.pivots_phase1, res.pivots_phase2) == (call["p1"], call["p2"])
    rhs, rows = t.read_rhs()
    assert G.sha_rhs(rhs, rows) == call["rhsSha"]
    if whole:
        trace = t.pivot_trace()
        assert len(trace) == g["nPivots"] and pivot_digest(trace) == g["pivotDigest"]
        assert G.sha_matrix(t.download()[0]) == g["final"]["matrixSha"]


# ---- the oracle, once per instance ---------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_one(lib, inst):
    m, vibr, vibc, unr = E.build(inst)
    t = Tableau(m, vibr, vibc, unr, lib=lib)
    try:
        res = t.simplex(check_cycles=True)
        rhs, rows = t.read_rhs()
        final = t.download()
        return {"messages": _messages(res), "feasible": bool(res.feasible), "p": (res.pivots_phase1, res.pivots_phase2), "trace": t.pivot_trace().copy(),
                "rhsSha": G.sha_rhs(rhs, rows), "matrixSha": G.sha_matrix(final[0]), "vibr": final[1].copy(), "vibc": final[2].copy(),
                "shape": m.shape, "initSha": G.sha_matrix(m), "vibr0": vibr.copy(), "vibc0": vibc.copy()}
    finally:
        t.close()


def bases():
    """the runs the filler shift is measured against: every (kind, small LP) without fillers and without the embedding"""
    return sorted({E.base_of(i) for i in E.INSTANCES})


def oracle(lib, inst):
    if inst.name not in _ORACLE:
        todo = sorted(set(E.INSTANCES + bases()), key=lambda i: (-(i.n + i.k), i.name))  # the large ones first
        todo = [i for i in todo if i.name not in _ORACLE]
        workers = max(1, min(16, len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "16") or 16)))
        with ThreadPoolExecutor(workers) as ex:  # (the oracle's calls release the GIL; it keeps no shared state)
            for i, out in zip(todo, ex.map(lambda i: _oracle_one(lib, i), todo)):
                _ORACLE[i.name] = out
    return _ORACLE[inst.name]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_goldens_are_there_and_are_the_instances():
    have = sorted(os.path.basename(p)[:-len(".json.gz")] for p in G.glob.glob(os.path.join(E.EDGES, "*.json.gz")))
    assert have == sorted(IDS) and sorted(WHERE) == sorted(IDS)
    for inst in E.INSTANCES:
        meta = golden(inst)["meta"]
        extra = tuple(meta["extra"]) if meta["extra"] else None
        assert (meta["kind"], meta["small"], meta["k"], meta["n"], meta["seed"], extra) == ("cycle_edge_" + inst.kind, inst.small, inst.k, inst.n, inst.seed, inst.extra)


def test_first_hit_is_the_literal_check_on_every_prefix_of_every_small_history():
    """first_hit(pairs) against check_for_cycles(pairs[:n]) for every n: the small goldens of tests/golden/cycles, the whole 128 set, and
    histories made to tempt it -- squares inside squares, a repeat too far back (the reference's `break`), repeated pairs without a square"""
    hists = []
    for inst in E.EDGE_128:
        g = golden(inst)
        _, p2, _, _ = E.replay(np.asarray(g["pivots"]).reshape(-1, 2), g["tableau"]["varIndexByRow"], g["tableau"]["varIndexByCol"], g["simplexCalls"][0]["p1"])
        hists.append(E.with_stop(p2, *start_length(g)))
    for path in sorted(G.glob.glob(os.path.join(E.CYCLES, "*.json.gz"))):
        g = G.load(path)
        if g["model"] is None:
            continue
        _, p2, _, _ = E.replay(np.asarray(g["pivots"]).reshape(-1, 2), g["tableau"]["varIndexByRow"], g["tableau"]["varIndexByCol"], g["simplexCalls"][0]["p1"])
        hists.append(E.with_stop(p2, *start_length(g)))
    a, b, c, d = (1, 2), (3, 4), (5, 6), (1, 4)
    hists += [[a, a], [a, b, a, b], [a, b, c, a, b, c], [a, b, c, a, b, d, a, b, c, a, b, d], [a, b, c, d, a, c, b, d, a], [a, b, a, c, a, b, a, c],
              [a, b, c, a, d, b, c, a, d, b], [a, b, b], [a, b, c, d, c, d], [a, b, c, b, a, b, c, b, a], [a]]
    rng = np.random.default_rng(5)
    for _ in range(200):  # two-letter alphabets: squares everywhere
        hists.append([(int(x), 7) for x in rng.integers(0, 3, rng.integers(2, 14))])
    n_hits = 0
    for h in hists:
        stop, hit = E.first_hit(h)
        last = stop if stop is not None else len(h)
        for n in range(0, last + 1):
            assert E.check_for_cycles(h[:n]) == (hit if n == stop else []), (h, n)
        n_hits += stop is not None
        assert E.seen_without_square(h[:last]) == [n for n in range(1, last + 1) if h[n - 1] in h[:n - 1] and n != stop]
    assert n_hits > 100


@pytest.mark.parametrize("inst", E.INSTANCES, ids=IDS)
def test_oracle_equals_the_golden(oracle_lib, inst):
    g, o = golden(inst), oracle(oracle_lib, inst)
    call = g["simplexCalls"][0]
    assert o["shape"] == (g["tableau"]["height"], g["tableau"]["width"])
    assert o["initSha"] == g["tableau"]["matrixSha"], "the rebuilt tableau is not the reference's"
    assert o["vibr0"].tolist() == g["tableau"]["varIndexByRow"] and o["vibc0"].tolist() == g["tableau"]["varIndexByCol"]
    assert o["messages"] == g["messages"] and o["feasible"] == call["feasible"] is False
    assert o["p"] == (call["p1"], call["p2"])
    assert len(o["trace"]) == g["nPivots"] and pivot_digest(o["trace"]) == g["pivotDigest"]
    assert o["trace"].reshape(-1).tolist() == g["pivots"]
    assert o["matrixSha"] == g["final"]["matrixSha"] and o["rhsSha"] == call["rhsSha"]


def _history(inst):
    """-> (the golden, the phase-2 history at the stop, the index maps after the last pivot)"""
    g = golden(inst)
    assert g["simplexCalls"][0]["p1"] == 0 and len(g["pivots"]) == 2 * g["nPivots"]
    tab = g["tableau"]
    _, pairs, vibr, vibc = E.replay(np.asarray(g["pivots"]).reshape(-1, 2), tab["varIndexByRow"], tab["varIndexByCol"], 0)
    return g, E.with_stop(pairs, *start_length(g)), vibr, vibc


@pytest.mark.parametrize("inst", E.INSTANCES, ids=IDS)
def test_python_reference_agrees_with_the_stop(inst):
    """the reference's trace, replayed: the literal check reports the golden's [start, length] on the history at the stop, nothing on
    the history one pair shorter (the large instances: through first_hit, which is the literal check on every prefix), and the pair
    that completes the square is one the final tableau can select (leaving variable basic, entering variable non-basic)"""
    g, hist, vibr, vibc = _history(inst)
    start, length = start_length(g)
    assert len(hist) == start + 2 * length == g["nPivots"] + 1
    assert g["final"]["varIndexByRow"] == vibr  # the replay's maps are the reference's
    assert hist[-1][0] in vibr[1:] and hist[-1][1] in vibc[1:]
    assert E.check_for_cycles(hist) == [start, length]
    assert E.first_hit(hist) == (len(hist), [start, length])  # nothing earlier
    if inst in E.EDGE_128:
        assert E.check_for_cycles(hist[:-1]) == []
    else:
        assert E.first_hit(hist[:-1]) == (None, [])


@pytest.mark.parametrize("inst", E.INSTANCES, ids=IDS)
def test_the_instance_sits_where_its_name_says(inst):
    g = golden(inst)
    start, length = start_length(g)
    n = start + 2 * length
    assert E.classify(n, start, length, inst.B) == WHERE[inst.name]
    assert n == HIST_LEN[inst.name.replace("_tall", "").replace("_wide", "")]
    assert g["simplexCalls"][0]["p2"] == n - 1  # pivots done: the newest pair was selected, not pivoted


def test_the_table_covers_every_class_at_both_boundaries():
    for B, insts in ((E.WGL_HIST, E.EDGE_128), (E.PIPE_LHIST, E.EDGE_4096)):
        assert {WHERE[i.name] for i in insts} >= set(CLASSES), B
    for tag in ("_tall", "_wide"):
        assert {WHERE[i.name] for i in E.TALL_WIDE if tag in i.name} == {"n == B", "n == B + 1", "first copy across"}
    names = {(i.small, WHERE[i.name]) for i in E.EDGE_128}
    assert {("deg_233528", "n == B"), ("deg_233528", "n == B + 1"), ("deg_178868", "n == B"), ("deg_178868", "n == B + 1")} <= names  # lengths 7 and 6


@pytest.mark.parametrize("inst", LARGE, ids=[i.name for i in LARGE])
def test_the_negative_path_runs(inst):
    """pairs selected before in the phase that complete no square: where the lean kernel's pair filter says "seen" and its suffix test
    must say "no" and go on -- hundreds per run, and at least one with the newest pair beyond the LDS part of the history wherever
    the hit itself lies beyond it (the second copy of the repeated block repeats the first)"""
    g, hist, _, _ = _history(inst)
    seen = E.seen_without_square(hist)
    assert len(seen) > 0
    if inst.name == "late_deg_35358_k650":
        assert len(seen) == 363
    if len(hist) > inst.B + 1:
        assert max(seen) > inst.B, (max(seen), len(hist))


@pytest.mark.parametrize("inst", E.INSTANCES, ids=IDS)
def test_the_fillers_shift_the_base_run_by_k(oracle_lib, inst):
    """the first k pivots are the fillers', in order, on the diagonal; the rest is the run without fillers k rows and k columns later.
    The embedding (zero-cost columns and their rows, appended last) changes nothing: same trace as the instance without it"""
    trace = np.asarray(golden(inst)["pivots"]).reshape(-1, 2)
    k = inst.k
    assert trace[:k].tolist() == [[i + 1, i + 1] for i in range(k)]
    base = oracle(oracle_lib, E.base_of(inst))
    assert base["messages"][0] == "Cycle in phase 2"
    assert (trace[k:] - k).tolist() == base["trace"].tolist()
    if inst.extra:
        assert trace.reshape(-1).tolist() == golden(E.BY_NAME[inst.name[:-5]])["pivots"]


# ---- which kernel ---------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id inst mode env geom lib")
PolicyCase = namedtuple("PolicyCase", "inst env")  # what test_grid_edges.policy reads
MODES_128 = {"auto": {}, "wg": {"JSLP_FORCE_PATH": "wg"}, "sp": {"JSLP_FORCE_PATH": "sp"}, "fused": {"JSLP_FORCE_PATH": "fused"},
             "resident": {"JSLP_FORCE_PATH": "resident"}, "nowglds": {"JSLP_NO_WGLDS": "1"}}
MODES_4096 = {"auto": {}, "cpt4": {"JSLP_RES_CPT": "4"}, "general": {"JSLP_RES_LEAN": "0", "JSLP_FORCE_PATH": "resident"}, "fused": {"JSLP_FORCE_PATH": "fused"}}
GEOM_OF_MODE = {"auto": "g1", "cpt4": "g2", "general": "g1", "fused": "fused"}


def _cases():
    out = []
    for inst in E.EDGE_128:
        for mode, env in MODES_128.items():
            geom = {"auto": "workgroup", "wg": "workgroup", "nowglds": "workgroup", "sp": "select+update", "fused": "fused", "resident": "g1"}[mode]
            out.append(Case("%s-%s" % (inst.name, mode), inst, mode, env, geom, "hip"))
    for inst in E.EDGE_4096:
        for mode, env in MODES_4096.items():
            out.append(Case("%s-%s" % (inst.name, mode), inst, mode, env, GEOM_OF_MODE[mode], "hip"))
        if WHERE[inst.name] in ("n == B", "n == B + 1"):
            out.append(Case("%s-chaos" % inst.name, inst, "chaos", {"JSLP_TEST_RESIDENT_LATE_WAVE0": "3"}, "g1", "hooks"))
    for inst in E.TALL_WIDE:
        out.append(Case("%s-auto" % inst.name, inst, "auto", {}, "g3" if "_tall" in inst.name else "g4", "hip"))
    return out


CASES = _cases()
GEOM = {"g1": (1024, 2, 8), "g2": (512, 4, 8), "g3": (512, 4, 16), "g4": (512, 6, 12)}


def _shape(inst):
    tab = golden(inst)["tableau"]
    return tab["height"], tab["width"], len(tab["unrestricted"])


def expected_lines(case):
    """the JSLP_DEBUG_LAUNCH lines of the solve (jslp_hip.hip run_simplex); a one-workgroup solve prints none"""
    H, W, n_unr = _shape(case.inst)
    unr = int(n_unr > 0)
    if case.geom == "workgroup":
        return []
    if case.geom == "select+update":
        return ["select+update"]
    nt = (_ld(W) + 2047) // 2048
    if case.geom == "fused":
        return ["k_fused_p1<%d,%d>" % (nt, unr), "k_pivot_fused<%d,%d,0>" % (nt, unr)]
    lean = int(case.env.get("JSLP_RES_LEAN") != "0")
    T, C, R = GEOM[case.geom]
    line = "k_simplex_resident<%d,%d,%d> unr %d lean %d opt 0 chk 1 xl 0 G %d rpb %d" % (T, C, R, unr, lean, _grid(H), _rpb(H))
    return [line] if case.geom in ("g1", "g2") else ["k_fused_p1<%d,%d>" % (nt, unr), line]  # (tall / wide: phase 1 through the fused pipeline)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_case_takes_the_kernel_it_names(case):
    """test_grid_edges.policy (resident_geometry / fused_eligible / use_wg_single restated) for the settings it knows; JSLP_FORCE_PATH=wg
    and sp are the engine's own words for one workgroup and for select + update (jslp_engine_create)"""
    H, W, n_unr = _shape(case.inst)
    if case.mode in ("wg", "sp"):
        assert case.geom == {"wg": "workgroup", "sp": "select+update"}[case.mode]
        return
    env = {k: v for k, v in case.env.items() if k not in ("JSLP_NO_WGLDS", "JSLP_TEST_RESIDENT_LATE_WAVE0")}  # (neither changes the path)
    assert policy(PolicyCase(GridInst(H, W, n_unr, 0, False, None), env)) == case.geom
    if case.inst in E.TALL_WIDE:
        if "_tall" in case.inst.name:
            assert H > 2048 and W - 1 <= 2047
        else:
            assert 2049 <= _ld(W) <= 3072 and W - 1 < 2601
    if case.inst in LARGE:
        assert W - 1 < 2601 and (W - 1) > 100  # partial pricing, 50 columns a batch


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_hip_stops_where_the_reference_stops(hip_lib, hip_hooks_lib, monkeypatch, capfd, case):
    """one solve, against the golden to the bit, on the kernel the case names.  A kernel that misses the hit pivots on to the
    engine's iteration cap (2 000 000 + 200 (rows + columns) pivots: minutes) and then fails with the cap's error"""
    _set_env(monkeypatch, case.env)
    g = golden(case.inst)
    m, vibr, vibc, unr = built(case.inst)
    assert G.sha_matrix(m) == g["tableau"]["matrixSha"] and unr == g["tableau"]["unrestricted"]
    capfd.readouterr()
    t = Tableau(m, vibr, vibc, unr, precision=g["tableau"]["precision"], lib=hip_hooks_lib if case.lib == "hooks" else hip_lib)
    try:
        res = t.simplex(check_cycles=True)
        lines = LAUNCH.findall(capfd.readouterr().err)
        cnt = t.get_counters()
        assert lines == expected_lines(case), lines
        resident = case.geom in GEOM
        assert t.last_path() == ("resident" if resident else "workgroup" if case.geom == "workgroup" else case.geom)
        check_run(t, res, g)
        if resident:
            assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_handovers"]) == (1, 0, 0), cnt
    finally:
        t.close()


def _non_cycling():
    """a small LP with an optimum and no cycle (the README's Berlin airlift)"""
    A = np.array([[0.0, 20000.0, 30000.0], [44.0, 1.0, 1.0], [512.0, 8.0, 16.0], [300000.0, 5000.0, 9000.0]])
    return A, np.array([-1, 0, 1, 2], dtype=np.int32), np.array([-1, 3, 4], dtype=np.int32), []


MANY = re.compile(r"^k_simplex_lds_many<(\d+),opt (\d)> n (\d+) lds \d+$")


@pytest.mark.gpu
def test_simplex_many_one_batch_across_the_128_boundary(hip_lib, oracle_lib, monkeypatch, capfd):
    """k_simplex_lds_many<512>: histories of 127, 128, 129 and 130 pairs (two families) and an LP that does not cycle, one workgroup
    each, side by side in ONE launch"""
    _set_env(monkeypatch, {})
    insts = [E.BY_NAME[n] for n in ("deg_35358_k84", "deg_35358_k85", "deg_35358_k86", "deg_35358_k87", "unr_3_k122", "unr_3_k123", "unr_3_k124", "unr_3_k125")]
    ts = [Tableau(*E.build(i), lib=hip_lib) for i in insts]
    ts.insert(4, Tableau(*_non_cycling(), lib=hip_lib))
    try:
        capfd.readouterr()
        res = simplex_many(ts, check_cycles=True)
        lines = [MANY.match(x) for x in LAUNCH.findall(capfd.readouterr().err)]
        assert len(lines) == 1 and lines[0] and lines[0].groups() == ("512", "0", str(len(ts))), lines
        twin = Tableau(*_non_cycling(), lib=oracle_lib)
        want = twin.simplex(check_cycles=True)
        assert want.optimal and want.cycle_phase == 0 and abs(twin.evaluation) == 1080000
        assert (res[4].optimal, res[4].cycle_phase, ts[4].evaluation, ts[4].pivot_trace().tolist()) == (1, 0, twin.evaluation, twin.pivot_trace().tolist())
        twin.close()
        for inst, t, r in zip(insts, ts[:4] + ts[5:], res[:4] + res[5:]):
            assert t.last_path() == "workgroup-many"
            check_run(t, r, golden(inst))
    finally:
        for t in ts:
            t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deg_35358_k84", "deg_35358_k85", "deg_35358_k86", "deg_35358_k87", "unr_3_k123", "unr_3_k124"])
def test_simplex_many_single_lp_takes_the_1024_thread_instance(hip_lib, monkeypatch, capfd, name):
    _set_env(monkeypatch, {})
    inst = E.BY_NAME[name]
    t = Tableau(*E.build(inst), lib=hip_lib)
    try:
        capfd.readouterr()
        res = simplex_many([t], check_cycles=True)
        lines = [MANY.match(x) for x in LAUNCH.findall(capfd.readouterr().err)]
        assert len(lines) == 1 and lines[0] and lines[0].groups() == ("1024", "0", "1"), lines
        check_run(t, res[0], golden(inst))
    finally:
        t.close()


WORKER_ENV = {"nodes": {}, "queue": {"JSLP_GROUP_MAX": "100"}, "threads1024": {"JSLP_WG_BATCH_THREADS": "1024"}, "threads256": {"JSLP_WG_BATCH_THREADS": "256"}}
NODE_NAMES = ("deg_35358_k84", "deg_35358_k85", "deg_35358_k86", "deg_35358_k87", "unr_3_k123", "unr_3_k124")  # (cycle_edges_worker.NAMES)


@pytest.mark.parametrize("name", NODE_NAMES)
def test_oracle_nodes_from_the_unsolved_root(oracle_lib, name):
    """the engine accepts save() on an unsolved upload; a node with an empty cut list is then restore + simplex of that root: the
    golden's run, node after node (what cycle_edges_worker.py asks of the node kernels)"""
    inst = E.BY_NAME[name]
    g = golden(inst)
    call, (start, length) = g["simplexCalls"][0], start_length(g)
    t = Tableau(*E.build(inst), lib=oracle_lib)
    try:
        t.save()
        for n in (1, 3):
            res, rhs, rows = t.applyCutsBatch([[] for _ in range(n)], check_cycles=True)
            for i, r in enumerate(res):
                assert (bool(r.feasible), bool(r.bounded), bool(r.optimal), r.height, r.cycle_phase) == (False, True, False, g["tableau"]["height"], 2)
                assert (r.pivots_phase1, r.pivots_phase2, r.cycle_start, r.cycle_length) == (call["p1"], call["p2"], start, length)
                assert G.sha_rhs(rhs[i, :r.height], rows[i, :r.height]) == call["rhsSha"]
    finally:
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(WORKER_ENV))
def test_node_and_batch_kernels_across_the_128_boundary(hip_lib, mode, tmp_path):
    """tests/cycle_edges_worker.py, one process per setting (JSLP_WG_BATCH_THREADS and JSLP_GROUP_MAX are read once per process): the
    histories of 127 .. 130 pairs as nodes of their unsolved root through k_node_lds<1024> / <512>, k_node_queue<512> and the eager
    sequence's k_simplex_lds<1024> / <512> / k_simplex_wg<256,1024>, and side by side through k_simplex_lds_many<512> / <1024>"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS and k != "JSLP_GROUP_MAX"}
    env.update(WORKER_ENV[mode], JSLP_DEBUG_LAUNCH="1")
    out = subprocess.run([sys.executable, WORKER, mode, str(tmp_path / "stderr.txt")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    tail = out.stdout[-2000:] + (tmp_path / "stderr.txt").read_text(errors="replace")[-3000:] if (tmp_path / "stderr.txt").exists() else out.stdout[-2000:] + out.stderr[-3000:]
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), tail
