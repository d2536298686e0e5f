"""jslpi_* on the MI355X: small MILPs with options.useIncremental in a pack, each tree walked under the INCREMENTAL service by one workgroup
inside one launch, parent checkpoints in the LP's arena on the device (the INC builds of k_tree_packed, include/jslpi_tree_incremental.h).

The yardsticks are the reference's recorded runs (fuzz_services, fuzz_soft, incremental.json.gz) and the Python host tree on the CPU oracle
(incremental_branch_and_cut.incremental_branch_and_cut behind TableauPack's restatement, its checkpoints the oracle engine's); the pack on
the GPU is never compared with itself."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import soft_pack_util as S
import tree_enh_util as E
import tree_inc_util as I
import tree_mir_util as M
import tree_pack_util as U
from jslpsolver_amd import Solve, _capi, solver
from jslpsolver_amd.engine import Tableau

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH = re.compile(r"\[jslp\] launch k_tree_packed<(\d+)(?:,(\w+) 1)?> n (\d+) lds (\d+)")
SIMPLEX_LAUNCH = re.compile(r"\[jslp\] launch k_simplex_packed<(\d+)(?:,(\w+) 1)?> n (\d+) lds (\d+)")
LDS_LIMIT = 65536
LIMITS = (50, 2, 1, 0)


def _with(model, **options):
    m = copy.deepcopy(model)
    m["options"] = dict(m.get("options") or {}, **options)
    return m


def test_recorded_fuzz_runs_in_one_pack(hip_lib, oracle_lib):
    services, soft = I.fuzz_incremental_cases()
    assert (len(services), len(soft)) == (89, 12)
    cases = services + soft
    items = [I.Item(c["model"]) for c in cases]
    pack, host = I.against_host(hip_lib, oracle_lib, items, [I.Inc()] * len(items), heap_cap=solver.TREE_HEAP_CAP, max_nodes=solver.TREE_MAX_NODES)
    assert 1 <= pack.launches <= 2 and not pack.status.any()
    for i, c in enumerate(cases):
        U.check_record(pack, i, items[i], c["nPivots"], c["digest"], c["iter"], c["keys"], c["result"], (c["gen"], c["seed"]))
    assert int(pack.tree["heap_high_water"].max()) == 42 and int(pack.tree["cuts_high_water"].max()) == 11
    assert int(pack.incremental["rows_high_water"].max()) == 24 and int(pack.incremental["checkpoints_used"].max()) == 27
    pack.close()
    host.close()


def test_fixture_records(hip_lib, oracle_lib):
    chosen = I.fixture_cases()
    assert len(chosen) == 115
    items = [it for _, it in chosen]
    pack, host = I.against_host(hip_lib, oracle_lib, items, [I.inc_of(c["options"]) for c, _ in chosen], heap_cap=256,
                                trace_cap=max(c["nPivots"] for c, _ in chosen) + 16)
    for i, (c, it) in enumerate(chosen):
        U.check_record(pack, i, it, c["nPivots"], c["pivotDigest"], c["iterations"], c["resultKeys"], c["result"], (c["file"], c["options"]))
    pack.close()
    host.close()


def test_both_builds_every_policy_every_checkpoint_limit(hip_lib, oracle_lib):
    """Integer_Wood_Shop_Problem (3 x 4, the one-wave build) and Knapsack_1 (52 x 51, 256 threads) under the nine policy pairs and
    max_checkpoints 50 / 2 / 1 / 0: states, tree / enhanced / incremental records and the pivot trace against the host walk"""
    shop, knap = I.Item(U.fixture("Integer_Wood_Shop_Problem")["model"]), I.Item(U.fixture("Knapsack_1")["model"])
    assert (shop.lp[0].shape[0] + shop.row_extra) * 4 <= 2048 < (52 + knap.row_extra) * 51 and knap.row_extra == 96
    items, policies = [], []
    for it in (shop, knap):
        for s, b in E.PAIRS:
            for k in LIMITS:
                items.append(it)
                policies.append(I.Inc(s, b, k))
    pack, host = I.against_host(hip_lib, oracle_lib, items, policies)
    assert pack.launches == 2
    st, inc = I.states(pack), pack.incremental
    for j, p in enumerate(policies):
        assert inc[j]["checkpoints_used"] <= p.max_checkpoints
        if p.node_selection == "best-first" or p.max_checkpoints == 0:  # best-first takes no checkpoint
            assert inc[j]["checkpoints_used"] == 0 and inc[j]["incremental_nodes"] == 0
        if p.branching == "strong":  # `strong` is pseudocost in this service
            assert st[j] == st[policies.index(p._replace(branching="pseudocost"), j - j % 36)], p
    by = {(j // 36, p): j for j, p in enumerate(policies)}
    # the reference's own limit: Knapsack_1 depth-first takes exactly 50 checkpoints over 189 nodes, 100 of them from a checkpoint -- the
    # children pushed after the 50th start from the root; hybrid takes 18 / 27 and moves checkpointed entries into the heap
    deep, hybrid = by[(1, I.Inc("depth-first", "pseudocost", 50))], by[(1, I.Inc("hybrid", "pseudocost", 50))]
    assert (int(inc[deep]["checkpoints_used"]), int(pack.tree[deep]["iterations"]), int(inc[deep]["incremental_nodes"])) == (50, 189, 100)
    assert (int(inc[hybrid]["checkpoints_used"]), int(inc[hybrid]["incremental_nodes"])) == (18, 27) and pack.enhanced[hybrid]["moved_to_heap"] > 0
    # a limit of 2 / 1 starts 4 / 2 nodes from a checkpoint at the most, and changes the walk's pivots but not its outcome
    for k in (2, 1):
        j = by[(1, I.Inc("depth-first", "pseudocost", k))]
        assert int(inc[j]["checkpoints_used"]) == k and 0 < int(inc[j]["incremental_nodes"]) <= 2 * k
        assert pack.evaluation[j] == pack.evaluation[deep] and st[j]["trace"] != st[deep]["trace"]
    # the stacked rows exceed the longest cut list (Integer_Wood_Shop_Problem depth-first: 7 rows against 5 cuts)
    j = by[(0, I.Inc("depth-first", "pseudocost", 50))]
    assert (int(inc[j]["rows_high_water"]), int(pack.tree[j]["cuts_high_water"])) == (7, 5)
    pack.close()
    host.close()


def test_copy_edges(hip_lib, oracle_lib, monkeypatch):
    """checkpoints whose height x width is odd (half a 16-byte word at the end) and even, at widths where a word holds the end of one row
    and the start of the next: 2 x 5, 4 x 3, 3 x 4 and 7 x 5 tableaus, several heights each"""
    names = ["TacoParty", "Integer_Wood_Problem", "Integer_Wood_Shop_Problem", "Integer_Sports_Complex_Problem"]
    items = [I.Item(U.fixture(n)["model"]) for n in names]
    assert [it.lp[0].shape for it in items] == [(2, 5), (4, 3), (3, 4), (7, 5)]
    seen, orig = [], Tableau.createCheckpoint

    def watched(self):
        seen.append((self.width, self.last.height))
        return orig(self)

    monkeypatch.setattr(Tableau, "createCheckpoint", watched)
    policies = [I.Inc("depth-first", b) for b in ("pseudocost", "most-fractional")]
    host = I.solve(oracle_lib, [it for it in items for _ in policies], policies * len(items))
    monkeypatch.setattr(Tableau, "createCheckpoint", orig)
    odd_tails = set()
    for w in (5, 3):  # odd widths: rows wrap inside a word, and the tail is half a word at every odd height
        heights = {h for ww, h in seen if ww == w}
        assert any(h % 2 for h in heights) and len({h for h in heights if h % 2 == 0}) >= 2, (w, sorted(heights))
        odd_tails |= {(w, h) for h in heights if h % 2}
    assert len(odd_tails) >= 4, sorted(odd_tails)
    assert len({h for ww, h in seen if ww == 4}) >= 3
    pack = I.solve(hip_lib, [it for it in items for _ in policies], policies * len(items))
    assert I.states(pack) == I.states(host) and (host.incremental["incremental_nodes"] > 0).all()
    pack.close()
    host.close()


def test_capacities(hip_lib, oracle_lib):
    shop_json = U.fixture("Integer_Wood_Shop_Problem")["model"]
    left, right = U.Item(U.fixture("Integer_Wood_Problem")["model"]), I.Item(U.fixture("TacoParty")["model"])
    policies = [("hybrid", None), I.Inc("depth-first"), I.Inc()]
    heap_hw, cuts_hw, nodes, rows_hw = 5, 5, 35, 7  # (tests/test_tree_inc_cpu.py measures them on the host)

    def both(heap_cap, cut_rows, max_nodes, row_extra):
        out = []
        for lib in (hip_lib, oracle_lib):
            items = [left, I.Item(shop_json, row_extra=row_extra, cut_rows=cut_rows), right]
            pack = I.make_pack(lib, items, policies, heap_cap=[256, heap_cap, 256], max_nodes=max_nodes)
            pack.results[:] = np.frombuffer(b"\x5a" * pack.results.nbytes, dtype=pack.results.dtype)  # sentinels in out / tree_out
            pack.tree[:] = np.frombuffer(b"\x5a" * pack.tree.nbytes, dtype=pack.tree.dtype)
            pack.incremental[:] = np.frombuffer(b"\x5a" * pack.incremental.nbytes, dtype=pack.incremental.dtype)
            try:
                pack.branch_and_cut(check_cycles=[it.check for it in items])
                err = None
            except _capi.EngineError as e:
                err = str(e)
            out.append((pack, err))
        return out

    (pack, err), (host, herr) = both(heap_hw, cuts_hw, nodes, rows_hw)  # exactly the host's measures
    assert err is None and herr is None and I.states(pack) == I.states(host)
    assert (int(pack.tree[1]["heap_high_water"]), int(pack.tree[1]["cuts_high_water"]), int(pack.tree[1]["iterations"]),
            int(pack.incremental[1]["rows_high_water"])) == (heap_hw, cuts_hw, nodes, rows_hw)
    want = I.states(host)
    pack.close()
    host.close()
    for caps, word in (((heap_hw - 1, cuts_hw, nodes, rows_hw), "heap_cap"), ((heap_hw, cuts_hw - 1, nodes, rows_hw), "cut_rows"),
                       ((heap_hw, cuts_hw, nodes - 1, rows_hw), "max_nodes"), ((heap_hw, cuts_hw, nodes, rows_hw - 1), "row_extra")):
        (pack, err), (host, herr) = both(*caps)
        assert err is not None and "(%d)" % _capi.JSLP_ERR_CAPACITY in err and "LP 1" in err and word in err, (caps, err)
        assert herr is not None and word in herr
        assert list(pack.status) == [_capi.JSLP_OK, _capi.JSLP_ERR_CAPACITY, _capi.JSLP_OK]
        assert pack.results[1].tobytes() == b"\x5a" * pack.results.itemsize and pack.tree[1].tobytes() == b"\x5a" * pack.tree.itemsize
        assert pack.incremental[1].tobytes() == b"\x5a" * pack.incremental.itemsize
        got = I.states(pack)
        assert got[0] == want[0] and got[2] == want[2]  # both neighbours are right
        pack.close()
        host.close()


def test_one_mixed_pack_equals_each_lp_alone(hip_lib, oracle_lib, monkeypatch, capfd):
    """default, optional objectives, MIR, enhanced and incremental LPs in ONE pack: every LP as in a pack of its own"""
    wood = U.fixture("Integer_Wood_Problem")["model"]
    soft = copy.deepcopy(wood)
    name = next(iter(soft["constraints"]))
    soft["constraints"][name] = dict(soft["constraints"][name], weight=1, priority=1)
    items = [U.Item(wood), S.SoftItem(soft), M.MirItem(_with(wood, useMIRCuts=True)), U.Item(U.fixture("Knapsack_1")["model"]),
             I.Item(U.fixture("Knapsack_1")["model"]), I.Item(U.fixture("Integer_Wood_Shop_Problem")["model"])]
    policies = [None, None, None, ("hybrid", "strong"), I.Inc(), I.Inc("depth-first", "most-fractional", 2)]
    assert items[1].n_optional > 0
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack, host = I.against_host(hip_lib, oracle_lib, items, policies)
    lines = LAUNCH.findall(capfd.readouterr().err)
    monkeypatch.delenv("JSLP_DEBUG_LAUNCH")
    assert sorted((int(t), kind or "plain", int(n)) for t, kind, n, _ in lines[-6:]) == [
        (64, "inc", 1), (64, "mir", 1), (64, "opt", 1), (64, "plain", 1), (256, "enh", 1), (256, "inc", 1)], lines
    got = I.states(pack)
    for i in range(len(items)):
        alone = I.solve(hip_lib, [items[i]], [policies[i]])
        assert I.state(alone, 0) == got[i], i
        if items[i].__class__ is S.SoftItem:
            assert alone.optional_objectives(0).tobytes() == pack.optional_objectives(i).tobytes() == host.optional_objectives(i).tobytes()
        alone.close()
    assert pack.mir[2]["simplexes"] > 0 and pack.incremental[4]["incremental_nodes"] > 0 and pack.incremental[5]["checkpoints_used"] == 2
    pack.close()
    host.close()


def one_lp_per_launch_group():
    """ten LPs, exactly one per launch group, in launch order: [(item, policy, threads, kind)].  Of the five 256-thread LPs two are
    Knapsack_1 as it is, three the small fixtures with cut_rows / row_extra pushed over 2048 cells of row capacity x width."""
    wood, shop = U.fixture("Integer_Wood_Problem")["model"], U.fixture("Integer_Wood_Shop_Problem")["model"]
    soft = copy.deepcopy(wood)
    name = next(iter(soft["constraints"]))
    soft["constraints"][name] = dict(soft["constraints"][name], weight=1, priority=1)
    tall_soft = S.SoftItem(soft)
    tall_soft.cut_rows = 680
    knap = U.fixture("Knapsack_1")["model"]  # (52 x 51: 256 threads by its own size, beside the inflated ones)
    return [(U.Item(wood), None, 64, "plain"), (U.Item(knap), None, 256, "plain"),
            (S.SoftItem(soft), None, 64, "opt"), (tall_soft, None, 256, "opt"),
            (M.MirItem(_with(wood, useMIRCuts=True)), None, 64, "mir"), (M.MirItem(_with(wood, useMIRCuts=True), row_extra=680), None, 256, "mir"),
            (U.Item(shop), ("depth-first", None), 64, "enh"), (U.Item(knap), ("hybrid", "strong"), 256, "enh"),
            (I.Item(shop), I.Inc("depth-first", "most-fractional", 2), 64, "inc"), (I.Item(shop, row_extra=520), I.Inc(), 256, "inc")]


def test_one_lp_per_launch_group_in_launch_order(hip_lib, oracle_lib, monkeypatch, capfd):
    """the ten LPs stand in the pack in the REVERSE of the launch order: the exact sequence of launch lines of branch_and_cut() and of
    simplex() (one wave before 256 threads; plain, optional objectives, MIR, enhanced, incremental), each line's LDS bytes, and every LP's
    records where the host walk, a pack of its own and the oracle-backed pack have them"""
    groups = one_lp_per_launch_group()
    want = [(threads, kind) for _, _, threads, kind in groups]
    assert want == [(64, "plain"), (256, "plain"), (64, "opt"), (256, "opt"), (64, "mir"), (256, "mir"), (64, "enh"), (256, "enh"), (64, "inc"), (256, "inc")]
    lds = []
    for it, _, threads, kind in groups:  # every LP's own byte count, on the CPU: below the 64 KiB refusal, and the thread count is the group's
        h, w = it.lp[0].shape
        rc = h + (it.row_extra if kind in ("mir", "inc") else it.cut_rows)
        count = {"mir": hip_lib.jslpc_tree_lds_bytes, "inc": hip_lib.jslpi_tree_lds_bytes, "enh": hip_lib.jslpt_lds_bytes}.get(kind)
        lds.append(count(h, w, rc) if count else hip_lib.jslps_tree_lds_bytes(h, w, rc, getattr(it, "n_optional", 0)))
        assert 0 < lds[-1] <= LDS_LIMIT and (rc * w > 2048) == (threads == 256), (kind, threads, rc, w)
    items, policies = [g[0] for g in groups][::-1], [g[1] for g in groups][::-1]
    checks = [it.check for it in items]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack, host = I.against_host(hip_lib, oracle_lib, items, policies)
    lines = LAUNCH.findall(capfd.readouterr().err)
    assert [(int(t), kind or "plain", int(n), int(b)) for t, kind, n, b in lines] == [(t, kind, 1, b) for (t, kind), b in zip(want, lds)], lines
    assert pack.launches == 10 and not pack.status.any()
    fresh = I.make_pack(hip_lib, items, policies)
    capfd.readouterr()
    fresh.simplex(check_cycles=checks)
    lines = SIMPLEX_LAUNCH.findall(capfd.readouterr().err)
    monkeypatch.delenv("JSLP_DEBUG_LAUNCH")
    assert [(int(t), kind or "plain", int(n), int(b)) for t, kind, n, b in lines] == [
        (t, "opt" if kind == "opt" else "plain", 1, b) for (t, kind), b in zip(want, lds)], lines
    assert fresh.launches == 10
    ref = I.make_pack(oracle_lib, items, policies)
    ref.simplex(check_cycles=checks)
    assert fresh.results.tobytes() == ref.results.tobytes() and fresh.evaluation.tobytes() == ref.evaluation.tobytes()
    got = I.states(pack)
    for i in range(len(items)):
        assert [a.tobytes() for a in fresh.read_rhs(i)] == [a.tobytes() for a in ref.read_rhs(i)], i
        assert fresh.pivot_trace(i).tobytes() == np.ascontiguousarray(ref.pivot_trace(i), dtype=np.int32).tobytes(), i
        assert [a.tobytes() for a in fresh.download(i)[:3]] == [a.tobytes() for a in ref.download(i)[:3]], i
        assert fresh.optional_objectives(i).tobytes() == ref.optional_objectives(i).tobytes(), i
        alone = I.solve(hip_lib, [items[i]], [policies[i]])
        assert I.state(alone, 0) == got[i], i
        assert alone.optional_objectives(0).tobytes() == pack.optional_objectives(i).tobytes() == host.optional_objectives(i).tobytes(), i
        alone.close()
    # (pack index = 9 - group) both MIR LPs ran their loop, the one-wave incremental LP spent its two checkpoints
    assert pack.mir[5]["simplexes"] > 0 and pack.mir[4]["simplexes"] > 0 and pack.incremental[1]["checkpoints_used"] == 2
    for p in (pack, host, fresh, ref):
        p.close()


def test_arena_addressing_under_oversubscription(hip_lib, oracle_lib):
    """1024 copies of three incremental LPs with different max_checkpoints -- arenas of different sizes -- interleaved in one launch: every
    copy equals the host walk"""
    base = [I.Item(U.fixture("Integer_Wood_Shop_Problem")["model"]), I.Item(U.fixture("Integer_Sports_Complex_Problem")["model"]),
            I.Item(U.fixture("TacoParty")["model"])]
    policies = [I.Inc("depth-first", None, 50), I.Inc("depth-first", "most-fractional", 3), I.Inc("hybrid", None, 1)]
    host = I.solve(oracle_lib, base, policies, trace_cap=512, heap_cap=32)
    want = I.states(host)
    assert (host.incremental["checkpoints_used"] > 0).all() and len({int(c) for c in host.incremental["checkpoints_used"]}) == 3
    copies = 1024
    pack = I.solve(hip_lib, base * copies, policies * copies, trace_cap=512, heap_cap=32)
    assert pack.launches == 1
    got = I.states(pack)
    for c in range(copies):
        for j in range(3):
            assert got[3 * c + j] == want[j], (c, j)
    pack.close()
    host.close()
    model = _with(U.fixture("Integer_Wood_Shop_Problem")["model"], useIncremental=True)
    assert Solve(model, lib=hip_lib) == Solve(model, lib=oracle_lib)  # the engine path is still right afterwards


def test_upload_and_second_call(hip_lib, oracle_lib):
    items = [I.Item(U.fixture(n)["model"]) for n in ("Knapsack_1", "Integer_Wood_Shop_Problem", "TacoParty")]
    policies = [I.Inc("depth-first"), I.Inc(), I.Inc("hybrid", "most-fractional", 1)]
    host = I.solve(oracle_lib, items, policies)
    pack = I.solve(hip_lib, items, policies)
    first = I.states(pack)
    assert first == I.states(host) and host.incremental[0]["checkpoints_used"] == 50 and host.enhanced[0]["pseudo_updates"] > 0
    with pytest.raises(_capi.EngineError, match="upload first"):
        pack.branch_and_cut(check_cycles=[it.check for it in items])
    pack.upload()
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    assert I.states(pack) == first  # (a checkpoint counter or a pseudocost table left over from the first call would change the walk)
    pack.close()
    host.close()


def test_solve_packed_with_the_keyword(hip_lib, oracle_lib):
    services, _ = I.fuzz_incremental_cases()
    default, _ = U.fuzz_default_cases()
    models = [c["model"] for c in services[::5]] + [c["model"] for c in default[:5]] + [_with(U.fixture("Knapsack_1")["model"], useIncremental=True)]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(m, lib=oracle_lib)) for m in models]
        assert [repr(r) for r in solver.solve_packed(models, lib=hip_lib, incremental=True)] == want
        assert [repr(r) for r in solver.solve_packed(models, lib=hip_lib)] == want


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import tree_inc_util as I, tree_pack_util as U
from jslpsolver_amd import _capi
items = [I.Item(U.fixture(n)["model"]) for n in ("Integer_Wood_Shop_Problem", "Knapsack_1", "TacoParty")]
pack = I.solve(_capi.load_hip(), items, [I.Inc(), I.Inc("depth-first"), I.Inc("best-first")])
print("launches", pack.launches, "status", int(pack.status.any()))
"""


def test_launch_line_from_a_child_process():
    env = dict(os.environ, JSLP_DEBUG_LAUNCH="1")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "launches 2 status 0" in out.stdout
    lines = [(int(t), kind, int(n), int(b)) for t, kind, n, b in LAUNCH.findall(out.stderr)]
    assert [(t, kind, n) for t, kind, n, _ in lines] == [(64, "inc", 2), (256, "inc", 1)], out.stderr
    lds = _capi.load_hip().jslpi_tree_lds_bytes
    assert lines[0][3] == max(lds(3, 4, 3 + 260), lds(2, 5, 2 + 264)) and lines[1][3] == lds(52, 51, 52 + 96) <= LDS_LIMIT
