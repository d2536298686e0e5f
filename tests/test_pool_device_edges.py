"""The two carriers of multi-GPU work at the node edges: the in-process device pool (jslp_pool_*) and the `_device` entry points of the
process-per-GPU path, HIP against the CPU oracle bit for bit.  Both reuse the node kernels of relax_batch_impl but switch on code no
other caller reaches: the pool hands every member a range of ONE pinned buffer laid out with the plain row capacity (NodeCall::shared:
no one-launch single child, no polled small batch, the scalar branch of gather_slot_lds unless the capacity is a multiple of 4), a
`_device` caller passes its own row_stride and its own device memory.

Reference: test_node_edges.plan() -- the oracle evaluating every node alone, restore() then applyCuts(cuts) -- and, for the roots the
primary saves anew (new_root()), the same on that root.  Never the oracle's own pool or `_device` entry points, never the HIP single
engine.  Compared without tolerance: feasible, bounded, optimal, height, both pivot counts, cycle_phase, the objective cell's and the
evaluation's bits, the RHS column and the row map up to the height; the compact read-back and the branch records are derived from the
same outcome.  A node without an optimum reports the evaluation the member that owns it had when the call began: a fan-out sets every
member's to the primary's, a non-empty share moves its member's to its last node's, an empty or a refused share leaves it alone; the
worker tracks it per member (include/jslp_engine.h says so in the pool comment).

Part 1, DevicePool(t, [0] * M), M = 1..4, per root back to back on one pool: n = 0, 1, M-1, M, M+1, 2M+1, the family, the family
repeated until one share passes 256 nodes; each in applyCutsBatch / applyCutsBatchWatched x copy / pinned, each twice (the second is
the one-launch shape in every member); the counters of a counted batch; on ERROR_ROOTS the four refused lists in member 0's share, the
last member's, and two members' at once (the call fails with the lower member's code and text; the next calls are right); then a new
root -- the primary saves after a relaxation grew its tableau and it was handed other optional objectives -- that the next call fans
out.  Part 2, one engine and memory of the caller's (one uint8 buffer, regions on multiples of 256 bytes, 4 KiB guard zones, all of it
pre-filled): relax_batch_device + results_from_states at row_stride cap .. cap + 3 and cap rounded up to 4, the watched and the
branch-record flavours (records as int64 bit patterns; 1100 more watched variables on H 2049x15), `_device` and host calls turn by
turn, refused lists and the batches after them; every guard zone and every node slice beyond height + (height & 1) entries must still
hold the fill.  Bases that are not 16-byte aligned are not tested: the header asks the caller for them.

The same script runs on the CPU against the oracle library with numpy memory (the twin below, unmarked), where two planted defects --
a node's slice read at stride cap + 1, shares cut as ceil(n / M) blocks -- must make the comparison fail at every stride residue.

Roots left out of the pool part: `fit 15x1040 cap 1788`, `fit 15x1040 cap 1790`, `cells 15x1040 cap 4100`, `dirty 2700x15`,
`dirty 4200x15`.  A lone node on them runs the chip-wide sequence, and a pool of virtual devices would put several members' chip-wide
launches on the one GPU at once: a combination that exists in tests only.  The two `fit 15x1040` roots are in part 2 with batches only.

GPU time of this module on an MI355X: 54 s (five workers: 12 s under the defaults with M = 1..4; 20, 8, 7 and 7 s under the other
settings with M = 2, 3) inside a full `-m gpu` run of 772 s on the same box, which leaves 718 s for the parent's suite in that run:
7.6 % of the parent's wall time (the bound is a tenth).  Run alone on that box the module takes 34 s.  The CPU twin takes 33 s.
"""
import ast
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from jslpsolver_amd import _capi
from jslpsolver_amd import engine

import test_node_edges as N
import pool_device_edges_worker as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "pool_device_edges_worker.py")

STRIDE_ROOTS = ("stride 41x15 cap 44", "stride 41x15 cap 45", "stride 41x15 cap 46", "stride 41x15 cap 47")
POOL_ROOTS = STRIDE_ROOTS + ("stride 41x15 cap 45+opt", "stride 41x15 cap 46+unr", "tiny 2x2", "tiny 7x6", "tiny 7x6+opt", "tiny 7x6+unr", "ld 15x129+unr", "ld 15x1040",
                             "H 513x15+opt", "H 2049x15", "fit 2590x15 cap 2608", "fit 2590x15 cap 2610")
FIT_CAP = N.largest_cap_that_fits(1040)
DEVICE_ONLY = ("fit 15x1040 cap %d" % FIT_CAP, "fit 15x1040 cap %d" % (FIT_CAP + 2))  # batches only: a lone node on them is solved chip-wide
DEVICE_ROOTS = POOL_ROOTS + DEVICE_ONLY

SETTINGS = {
    "defaults": {},
    "group4": {"JSLP_GROUP_MAX": "4"},
    "nozerocopy": {"JSLP_ZERO_COPY": "0"},
    "nowglds": {"JSLP_NO_WGLDS": "1"},
    "cow0": {"JSLP_NODE_COW": "0"},
}
MEMBERS = {"defaults": (1, 2, 3, 4)}  # the other settings: (2, 3)


# ---- the plan: test_node_edges' own, plus every pool root saved anew ---------------------------------------------------------------
def new_root(lib, root):
    """the root the primary saves in the middle of a pool's life: after the first node that grows the tableau, with other optional
    objectives (two rows where the root has none, three where it has two); a few cut lists and the oracle's outcome of each on it"""
    fam, want = root["family"], root["want"]
    k = next(k for k, w in enumerate(want) if w["optimal"] and w["height"] > root["H"])
    rng = np.random.default_rng(root["seed"] + 2)
    oo = rng.integers(-5, 6, (3 if root["oo"] is not None else 2, root["cols"])).astype(np.float64)
    t = N.tableau(lib, root)
    try:
        t.simplex(check_cycles=root["check"])
        t.save()
        r, rhs, rows = t.applyCuts(fam[k], check_cycles=True)
        got = N.outcome(r, rhs, rows)
        assert got["rhs"] == want[k]["rhs"] and got["rows"] == want[k]["rows"], root["name"]
        lib.check(lib.jslp_engine_set_optional_objectives(t._h, int(oo.shape[0]), _capi.ptr_f64(oo)), "jslp_engine_set_optional_objectives")
        t.save()
        spare = root["cap"] - want[k]["height"]
        singles = [c for c in fam if len(c) == 1]
        lists = [[]] + singles[::max(1, len(singles) // 8)] + [c for c in fam if len(c) == 2][:2]
        lists = [c for c in lists if len(c) <= spare]
        out = []
        for cuts in lists:
            t.restore()
            r, rhs, rows = t.applyCuts(cuts, check_cycles=True)
            out.append(N.outcome(r, rhs, rows))
    finally:
        t.close()
    return dict(k=k, oo=oo, family=lists, want=out, eval=want[k]["evaluation"])


_PLAN = {}


def pool_plan(oracle_lib):
    if not _PLAN:
        p = N.plan(oracle_lib)
        for name in DEVICE_ROOTS:
            root = dict(p[name])  # (test_node_edges' plan stays as it is)
            if name in POOL_ROOTS:
                root["new_root"] = new_root(oracle_lib, root)
            _PLAN[name] = root
    return _PLAN


def all_pool_cases():
    return {(c, o, f) for c in range(4) for o in range(2) for f in W.FLAVOURS}


# ---- CPU: the script itself against the oracle, and the defects it must see --------------------------------------------------------
def test_roots_are_the_ones_meant(oracle_lib):
    names = {s["name"] for s in N.root_specs()}
    assert set(DEVICE_ROOTS) <= names and DEVICE_ONLY == ("fit 15x1040 cap 1788", "fit 15x1040 cap 1790")
    assert set(N.ERROR_ROOTS) <= set(POOL_ROOTS) and W.BIG_WATCHED in POOL_ROOTS
    p = pool_plan(oracle_lib)
    assert [p[n]["cap"] % 4 for n in STRIDE_ROOTS] == [0, 1, 2, 3]
    for name in STRIDE_ROOTS:  # odd and even final heights at every residue
        assert {w["height"] % 2 for w in p[name]["want"]} == {0, 1}, name
    for name in POOL_ROOTS:
        root = p[name]
        assert root["cap"] * ((root["cols"] + 15) // 16 * 16) <= 1536 * 1024, name  # a lone node is not chip-wide
        nr = root["new_root"]
        assert len(nr["family"]) >= 2 and any(not w["optimal"] for w in root["want"]), name
        assert all(w["height"] > root["H"] for w in nr["want"]), name  # every node of the new root starts from the grown tableau
    big = p[W.BIG_WATCHED]
    assert len(W.watched_with_dup(big)) + 1100 > 1024 and len(W.watched_with_dup(big)) + 1100 <= big["cap"]
    for name in DEVICE_ONLY:  # a batch keeps its one-workgroup kernels, a lone node does not
        root = p[name]
        assert 1536 * 1024 < root["cap"] * 1040 <= 4 * 1024 * 1024, name


def test_a_call_without_nodes_hands_out_an_empty_view():
    v = engine._pinned_view(_capi._f64p(), (1, 44))
    assert v.shape == (0, 44) and v.dtype == np.float64


def test_cpu_twin_of_both_parts(oracle_lib):
    """the whole script on the oracle library, "device" memory a numpy buffer"""
    lines = []
    cov, seen = W.run(oracle_lib, pool_plan(oracle_lib), POOL_ROOTS, DEVICE_ROOTS, (1, 2, 3, 4), W.NumpyMemory, log=lines.append)
    assert cov == all_pool_cases(), sorted(all_pool_cases() - cov)
    assert {(n, b) for n in STRIDE_ROOTS for b in ("vector", "scalar")} <= seen
    assert sum(1 for s in lines if s.startswith("root ok")) == len(POOL_ROOTS) + len(DEVICE_ROOTS)


def ceil_blocks(n, M):
    """the wrong split: blocks of ceil(n / M) nodes"""
    b = -(-n // M) if n else 0
    return [(min(n, mi * b), min(n, (mi + 1) * b)) for mi in range(M)]


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("name", STRIDE_ROOTS)
def test_the_comparison_sees_a_wrong_stride_and_a_wrong_split(oracle_lib, monkeypatch, name, M):
    root = pool_plan(oracle_lib)[name]
    sizes = [M + 1, 2 * M + 1, len(root["family"])]
    W.run_pool(oracle_lib, root, M, set(), sizes)  # as it is: passes
    with monkeypatch.context() as m:
        m.setattr(W, "pool_stride", lambda cap: cap + 1)
        with pytest.raises(AssertionError, match="RHS column|row map"):
            W.run_pool(oracle_lib, root, M, set(), sizes)
    with monkeypatch.context() as m:
        m.setattr(W, "share_bounds", ceil_blocks)
        with pytest.raises(AssertionError, match="evaluation"):
            W.run_pool(oracle_lib, root, M, set(), sizes)
    assert any(ceil_blocks(n, M) != W.share_bounds(n, M) for n in sizes)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_file(oracle_lib, tmp_path_factory):
    """the oracle's answers, computed once and handed to every worker in a file"""
    path = tmp_path_factory.mktemp("pool_device_edges") / "plan.pkl"
    with open(path, "wb") as fh:
        pickle.dump(pool_plan(oracle_lib), fh, protocol=pickle.HIGHEST_PROTOCOL)
    return str(path)


def _worker(plan_file, extra, members, timeout):
    env = {k: v for k, v in os.environ.items() if k not in N.KNOBS}
    env.update(extra)
    env["JSLP_DEBUG_LAUNCH"] = "1"
    cmd = [sys.executable, WORKER, plan_file, "\n".join(POOL_ROOTS), "\n".join(DEVICE_ROOTS), ",".join(str(m) for m in members)]
    try:
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        pytest.exit("the pool worker hung (%s): nothing more is started on this GPU" % extra, returncode=3)
    print(out.stdout[-8000:])
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):  # killed by a signal: a fault, not a wrong answer
        pytest.exit("the pool worker died with %d (%s): nothing more is started on this GPU\n%s" % (out.returncode, extra, out.stdout[-3000:]), returncode=3)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-3000:] + out.stderr[-5000:]
    return out.stdout


def _kernels(out, part):
    return {m.group(1): set(m.group(2).split(" ; ")) for m in re.finditer(r"^root ok \| %s \| (.+?) \| .*? \| (.*)$" % part, out, re.M)}


def _compared(out, part):
    return set(ast.literal_eval(re.search(r"^compared \| %s \| (.*)$" % part, out, re.M).group(1)))


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_pool_and_device_entry_points_at_the_node_edges(hip_lib, plan_file, setting):
    members = MEMBERS.get(setting, (2, 3))
    out = _worker(plan_file, SETTINGS[setting], members, 600)
    assert out.count("root ok | pool |") == len(POOL_ROOTS) and out.count("root ok | device |") == len(DEVICE_ROOTS)
    # every combination was compared: the pool's stride modulo 4 x the parity of the final height x the read-back flavour; and
    # part 2 reached both branches of the gather on every stride root
    assert _compared(out, "pool") == all_pool_cases(), sorted(all_pool_cases() - _compared(out, "pool"))
    assert {(n, b) for n in STRIDE_ROOTS for b in ("vector", "scalar")} <= _compared(out, "device")
    # the kernels each root is there for (the members' lines interleave: per root, not per call)
    pool = _kernels(out, "pool")
    for name, ks in pool.items():
        joined = " ; ".join(sorted(ks))
        assert "chip-wide" not in joined, (setting, name, joined)
        if name.endswith("+opt") and setting != "nowglds":  # (the generic kernels carry no build per optional objectives)
            assert "opt 1" in joined and "opt 0" not in joined, (setting, name, joined)
        if setting == "group4" and name != "fit 2590x15 cap 2610":
            assert "k_node_queue<512," in joined, (setting, name, joined)
    assert "k_node_wg<512,2048>" in pool["fit 2590x15 cap 2610"], (setting, sorted(pool["fit 2590x15 cap 2610"]))
    if setting != "nowglds":
        assert any(k.startswith("k_node_lds") for k in pool["fit 2590x15 cap 2608"]), (setting, sorted(pool["fit 2590x15 cap 2608"]))
