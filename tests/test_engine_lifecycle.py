"""Engines that take over what destroyed engines parked (the resource pool of jslp_hip.hip: stream, events, pinned state, arenas, staging
pairs) against engines that allocate everything themselves, and both against the CPU oracle: bit for bit, no tolerance.

ONE script of calls (run_script) runs three times: on the oracle in this process, and on the product library in two worker processes
(JSLP_NO_POOL is latched), once with the pool and once with JSLP_NO_POOL=1.  Every observation -- result structs, RHS columns, row maps,
pivot traces, branch records, optional objective rows -- must be equal in all three.  The cut lists come from the plan, chosen on the
oracle so that every node reaches an optimum (a node without one reports the evaluation its call started from, which a batch and the
sequential oracle define differently: tests/test_node_edges.py).

The script, in order:
  * "flag": a 40 x 30 engine whose ONLY polled call leaves the completion flag at 1, destroyed; its successor's first polled call must
    carry the inherited sequence on (a fresh counter would take the flag's 1 for its own first completion and read a stale outcome);
  * "recycle": engines "a" 40 x 30 (row capacity 60: takes the flag pair's bundle, same size), "b" 14 x 11 (takes "a"'s: every arena
    reused), "c" 200 x 150 (capacity 260; takes the same bundle, still sized for 40 x 30: static arena replaced, the spare slot arena too
    small and dropped), "d" 40 x 30 again (takes "c"'s, larger than it needs), each destroyed before the next is created; each solves,
    relaxes three single children (the first through several launches, then the polled one-launch kernel), a 20-node batch and a
    branch-record batch; then jslp_release_pooled_resources() empties the shelf;
  * "five": five engines (14 x 11) alive at once, all new, destroyed together (the pool keeps four), then five created: four take a
    parked bundle, the fifth is new;
  * "grow", one engine (40 x 30, capacity 110; it takes a parked 14 x 11 bundle: static arena replaced, spare dropped, and the slots
    then grow on it): batches of 4, 300 and 4 nodes with restore() + read_rhs() on either side of the growth;
    20 nodes of 1 cut, then of 50 cuts (the cut staging grows); optional objectives 0 -> 2 -> 1 -> 0 across uploads with a solve after
    each; the fp32 twin's first use (against tests/fp32_reference.py); checkpoint create / release / create;
  * "resident": 257 x 256 dense, one cell row past the one-workgroup limit (65 792 cells: the smallest tableau the register-resident
    path takes, tests/test_grid_edges.py `policy`), solved with the cycle check off and then on, which carves the hand-off arena again
    for the history; the engine's counters must show two accepted register-resident launches, no refusal, roll-back or hand-over.
The whole script takes ~1 s on the oracle and a few seconds per worker."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import fp32_reference
import test_node_edges as N
from jslpsolver_amd import _capi, generators
from jslpsolver_amd.engine import Tableau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "engine_lifecycle_worker.py")
F32_PRECISION = 1e-4


def spec(rows, cols, cap, seed):
    return dict(name="%dx%d cap %d seed %d" % (rows, cols, cap, seed), rows=rows, cols=cols, cap=cap, seed=seed, unr=False, opt=False, density=0.6)


SPECS = {"flag0": spec(40, 30, 60, 11), "flag1": spec(40, 30, 60, 12), "a": spec(40, 30, 60, 1), "b": spec(14, 11, 20, 2), "c": spec(200, 150, 260, 3),
         "d": spec(40, 30, 60, 4), "grow": spec(40, 30, 110, 5), "grow2": spec(40, 30, 110, 6)}
SPECS.update({"five%d" % i: spec(14, 11, 20, 20 + i) for i in range(10)})


# ---- the plan: roots and cut lists, chosen on the oracle ----------------------------------------------------------------------------
def plan_root(oracle_lib, sp):
    """the root and cut lists whose nodes all reach an optimum: `good` (single cuts and pairs, each checked alone on the oracle)"""
    root = N.build_root(sp)
    t = N.tableau(oracle_lib, root)
    res = t.simplex(True)
    assert res.optimal, sp["name"]
    rhs, rows = t.read_rhs()
    t.save()
    basic = [(int(rows[r]), float(rhs[r])) for r in range(1, len(rows)) if abs(rhs[r] - round(rhs[r])) > 1e-6]
    singles = [[N._cut(kind, v, val)] for v, x in basic for kind, val in (("max", np.floor(x)), ("min", np.ceil(x)))]
    pairs = [singles[i] + singles[(i + 2) % len(singles)] for i in range(0, len(singles), 2) if singles[i][0]["varIndex"] != singles[(i + 2) % len(singles)][0]["varIndex"]]
    good = []
    for cuts in singles + pairs:
        r, _, _ = t.applyCuts(cuts)
        if r.optimal and r.feasible and r.bounded:
            good.append(cuts)
    t.close()
    assert len(good) >= 4, (sp["name"], len(good))
    m = sp["rows"] - 1
    return dict(root, good=good, watch=list(range(m, m + sp["cols"] - 1)))


@pytest.fixture(scope="module")
def plan(oracle_lib):
    p = {k: plan_root(oracle_lib, sp) for k, sp in SPECS.items()}
    A, vibr, vibc = generators.dense_resource_allocation_tableau(12345, 255, 256)
    assert A.shape == (257, 256) and 257 * 256 > 64 * 1024 >= 256 * 256  # one row past what one workgroup takes
    p["resident"] = dict(A=A, vibr=vibr, vibc=vibc)
    return p


def cycled(good, n, first=0):
    return [good[(first + i) % len(good)] for i in range(n)]


# ---- observations -------------------------------------------------------------------------------------------------------------------
def node_obs(res, rhs, rows):
    o = N.outcome(res, rhs, rows)
    assert not np.isnan(o["obj_cell"]) and not np.isnan(o["evaluation"])  # (equality below is plain ==)
    return o


def batch_obs(t, lists):
    out, rhs, rows = t.applyCutsBatch(lists)
    return [node_obs(out[i], rhs[i], rows[i]) for i in range(len(lists))]


def objectives_obs(t):
    rows = np.zeros((4, t.width), dtype=np.float64)
    n = _capi.C.c_int32(-1)
    t.lib.check(t.lib.jslp_engine_get_optional_objectives(t._h, _capi.ptr_f64(rows), _capi.C.byref(n)), "jslp_engine_get_optional_objectives")
    return n.value, rows[:n.value].tobytes()


def set_objectives(t, oo):
    oo = np.ascontiguousarray(oo, dtype=np.float64)
    t.lib.check(t.lib.jslp_engine_set_optional_objectives(t._h, int(oo.shape[0]), _capi.ptr_f64(oo)), "jslp_engine_set_optional_objectives")


def solve_obs(t, check_cycles=True):
    res = t.simplex(check_cycles)
    rhs, rows = t.read_rhs()
    return node_obs(res, rhs, rows), t.pivot_trace().tobytes()


def f32_obs(t, root, is_hip):
    """what jslp_engine_simplex_f32 hands back, as fp32_reference.Outcome.observable() states it; the oracle has no fp32 twin: the restated core stands in"""
    if not is_hip:
        return fp32_reference.solve(root["A"], root["vibr"], root["vibc"], precision=F32_PRECISION, check_cycles=True).observable()
    res, rhs, rows, _ = t.simplex_f32(F32_PRECISION, True)
    return (res.feasible, res.bounded, res.optimal, res.unbounded_var_index, res.pivots_phase1, res.pivots_phase2, res.cycle_phase, res.height,
            fp32_reference._bits(res.obj_cell), np.asarray(rhs, dtype=np.float64).view(np.uint64).tolist(), np.asarray(rows).tolist())


# ---- the script ---------------------------------------------------------------------------------------------------------------------
def exercise(t, root, singles=3, batch=20):
    """a solve, single children, a batch, a branch-record batch"""
    obs = [solve_obs(t)]
    t.save()
    for cuts in cycled(root["good"], singles):
        obs.append(node_obs(*t.applyCuts(cuts)))
    if batch:
        obs.append(batch_obs(t, cycled(root["good"], batch, 1)))
        t.set_watched_variables(root["watch"])
        results, recs = t.applyCutsBatchBranch(cycled(root["good"], batch, 2))
        obs.append((np.ascontiguousarray(recs).tobytes(), [(r.feasible, r.bounded, r.optimal, r.height, r.evaluation) for r in results[:batch]]))
    return obs


def run_script(lib, plan, is_hip):
    obs = {}

    def engine(key):
        return N.tableau(lib, plan[key])

    # the completion flag's first value changes hands
    t = engine("flag0")
    obs["flag0"] = exercise(t, plan["flag0"], singles=2, batch=0)  # (the first single child: several launches; the second: the polled kernel)
    t.close()
    t = engine("flag1")
    obs["flag1"] = exercise(t, plan["flag1"], singles=2, batch=0)
    t.close()
    # one engine after the other
    for k in ("a", "b", "c", "d"):
        t = engine(k)
        obs[k] = exercise(t, plan[k])
        t.close()
        if k == "d":
            lib.jslp_release_pooled_resources()  # (behind "c" and "d": in front of "c" it would hand "c" an empty shelf)
    # five alive at once
    for first in (0, 5):
        ts = [engine("five%d" % (first + i)) for i in range(5)]
        for i, t in enumerate(ts):
            obs["five%d" % (first + i)] = exercise(t, plan["five%d" % (first + i)], singles=2, batch=0)
        for t in ts:
            t.close()
    # one engine grows
    root = plan["grow"]
    t = engine("grow")
    g = obs["grow"] = [solve_obs(t)]
    t.save()
    for n in (4, 300, 4):
        t.restore()
        g.append(("live tableau in front of %d nodes" % n, [x.tobytes() for x in t.read_rhs()]))
        g.append(batch_obs(t, cycled(root["good"], n)))
        t.restore()
        g.append(("live tableau behind %d nodes" % n, [x.tobytes() for x in t.read_rhs()]))
    assert g[1][1] == g[3][1] == g[4][1] == g[6][1] == g[7][1] == g[9][1], "restore() + read_rhs() around the growth of the slots"
    one = [c for c in root["good"] if len(c) == 1]
    g.append(batch_obs(t, cycled(one, 20)))
    g.append(batch_obs(t, [c * 50 for c in cycled(one, 20)]))  # 1000 cuts: the staging pair grows
    # optional objectives 0 -> 2 -> 1 -> 0 across uploads
    second = plan["grow2"]
    rng = np.random.default_rng(99)
    for i, n_opt in enumerate((2, 1, 0)):
        r = second if i % 2 == 0 else root
        t.upload(r["A"], r["vibr"], r["vibc"])
        if n_opt:
            set_objectives(t, rng.integers(-5, 6, (n_opt, r["cols"])).astype(np.float64))
        g.append((solve_obs(t), objectives_obs(t)))
    # the fp32 twin's first use (the live tableau: `second`, solved -- the twin starts from a fresh upload)
    t.upload(second["A"], second["vibr"], second["vibc"])
    g.append(f32_obs(t, second, is_hip))
    # checkpoint create / release / create
    g.append(solve_obs(t))
    ck = t.createCheckpoint()
    g.append([node_obs(*x) for x in t.applyCutsFrom(ck, [second["good"][0]])])
    t.restoreCheckpoint(ck)
    t.releaseCheckpoint(ck)
    ck2 = t.createCheckpoint()
    g.append([node_obs(*x) for x in t.applyCutsFrom(ck2, [second["good"][1]])])
    t.restoreCheckpoint(ck2)
    g.append([x.tobytes() for x in t.read_rhs()])
    t.close()
    # the smallest tableau of the register-resident path: cycle check off, then on
    r = plan["resident"]
    t = Tableau(r["A"], r["vibr"], r["vibc"], lib=lib)
    if is_hip:
        t.set_counting(True)  # (zeroes the launch counters asserted below)
    obs["resident"] = [solve_obs(t, False)]
    if is_hip:
        assert t.last_path() == "resident", t.last_path()
    t.upload(r["A"], r["vibr"], r["vibc"])
    obs["resident"].append(solve_obs(t, True))
    if is_hip:  # both solves ran register-resident, one accepted launch each: the second is the lean build with the check on, after the arena was carved again
        c = t.get_counters()
        assert t.last_path() == "resident" and (c["resident_launches"], c["resident_refusals"], c["resident_aborts"], c["resident_handovers"]) == (2, 0, 0, 0), (t.last_path(), c)
    t.close()
    return obs


def first_difference(a, b, path=""):
    if type(a) is not type(b):
        return "%s: %s against %s" % (path, type(a).__name__, type(b).__name__)
    if isinstance(a, dict):
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                return "%s: key %r on one side only" % (path, k)
            d = first_difference(a[k], b[k], "%s[%r]" % (path, k))
            if d:
                return d
        return None
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return "%s: %d entries against %d" % (path, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            d = first_difference(x, y, "%s[%d]" % (path, i))
            if d:
                return d
        return None
    if a != b:
        return "%s: %r against %r" % (path, a if not isinstance(a, bytes) else a[:32], b if not isinstance(b, bytes) else b[:32])
    return None


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_obs(oracle_lib, plan):
    return run_script(oracle_lib, plan, False)


def test_the_script_runs_on_the_oracle(oracle_obs):
    assert set(oracle_obs) >= {"flag0", "flag1", "a", "b", "c", "d", "five9", "grow", "resident"}
    assert oracle_obs["resident"][0] == oracle_obs["resident"][1]  # no cycle found: the check changes nothing
    assert [oracle_obs["grow"][i][1][0] for i in (12, 13, 14)] == [2, 1, 0]  # optional objectives after each upload
    nodes = []

    def walk(x):
        if isinstance(x, dict) and "optimal" in x:
            nodes.append(x)
        elif isinstance(x, (list, tuple)):
            for y in x:
                walk(y)

    walk(list(oracle_obs.values()))
    assert len(nodes) > 400 and all(n["optimal"] and n["feasible"] and n["bounded"] for n in nodes)  # (the module docstring: why)


@pytest.fixture(scope="module")
def gpu_obs(hip_lib, plan, tmp_path_factory):
    """the script on the product library: with the pool, and with JSLP_NO_POOL=1"""
    d = tmp_path_factory.mktemp("lifecycle")
    plan_file = str(d / "plan.pkl")
    with open(plan_file, "wb") as fh:
        pickle.dump(plan, fh)
    out = {}
    for name, extra in (("pool", {}), ("nopool", {"JSLP_NO_POOL": "1"})):
        env = {k: v for k, v in os.environ.items() if not k.startswith("JSLP_") or k == "JSLP_HIP_LIBRARY"}  # (no knob of the caller's; its library)
        env.update(extra)
        obs_file = str(d / (name + ".pkl"))
        run = subprocess.run([sys.executable, WORKER, plan_file, obs_file], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
        assert run.returncode == 0 and run.stdout.strip().endswith("ok"), (name, run.returncode, run.stdout[-3000:])
        with open(obs_file, "rb") as fh:
            out[name] = pickle.load(fh)
    return out


@pytest.mark.gpu
def test_recycled_engines_equal_fresh_ones_bit_for_bit(gpu_obs):
    assert first_difference(gpu_obs["pool"], gpu_obs["nopool"]) is None


@pytest.mark.gpu
@pytest.mark.parametrize("run", ["pool", "nopool"])
def test_recycled_and_fresh_engines_equal_the_oracle_bit_for_bit(gpu_obs, oracle_obs, run):
    assert first_difference(oracle_obs, gpu_obs[run]) is None
