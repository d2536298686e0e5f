"""jslpc_* on the MI355X: small MILPs with options.useMIRCuts in a pack, every node's MIR-cut loop run by the LP's workgroup inside the tree
kernel (the MIR builds of k_tree_packed).

The yardsticks are the reference's recorded MIR runs (fuzz records, tests/golden/mir.json.gz) and the Python host tree on the CPU oracle with
its round-by-round MIR loop (branch_and_cut.branch_and_cut + mir_loop behind TableauPack's restatement); the pack on the GPU is never
compared with itself.  The JSLP_DEBUG_LAUNCH lines say how many launches ran, with which build and how many LPs each.

A round-limit case (JSLPR_MAX_ROUNDS rounds of one node without a stop) is not here: no model that needs 64 rounds was found on the CPU --
over the fuzz records, the fixtures and the dense seeds below the most rounds one node took is 6."""
import re
import warnings

import numpy as np
import pytest

import tree_mir_util as M
import tree_pack_util as U
from jslpsolver_amd import Solve, _capi, generators
from jslpsolver_amd.engine import Tableau, TableauPack
from test_cycle_goldens import SMALL as CYCLE_GOLDENS, _instance
from test_tree_packed_gpu import BERLIN, INFEASIBLE, NO_INTEGRAL, UNBOUNDED

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[jslp\] launch k_tree_packed<(\d+)(,mir 1)?> n (\d+) lds (\d+)")
LDS_LIMIT = 65536
ROUTING_CELLS = 2048  # PACK_CELLS_WAVE (jslp_hip.hip): at most this many cells AT THE ROW CAPACITY -> the one-wave build


def _launches(capfd):
    """(threads, MIR build?, LPs, LDS bytes) per launch line"""
    return [(int(t), bool(mir), int(n), int(b)) for t, mir, n, b in LAUNCH.findall(capfd.readouterr().err)]


def _against_host(hip_lib, oracle_lib, items, **kw):
    """one pack on the GPU, one call; every LP against the Python host tree on the oracle: result struct, tree counters, MIR counters,
    evaluation, final RHS column and row map, pivot trace -- all as bytes"""
    host = M.solve(oracle_lib, items, **kw)
    pack = M.solve(hip_lib, items, **kw)
    for i, (a, b) in enumerate(zip(M.states(pack), M.states(host))):
        assert a == b, "LP %d differs from the host tree: %s" % (i, [k for k in a if a[k] != b[k]])
    return pack, host


def _cells(it):
    return (it.lp[0].shape[0] + (it.row_extra if M.is_mir(it) else it.cut_rows)) * it.lp[0].shape[1]


def test_reference_records_in_one_pack(hip_lib, oracle_lib, monkeypatch, capfd):
    cases = M.fuzz_mir_cases()
    records = M.fixture_mir_records()
    assert len(cases) >= 85 and len(records) == 10
    items = [M.MirItem(c["model"]) for c in cases] + [M.MirItem(model) for _, model, _ in records]
    plain = [U.Item(U.fixture(n)["model"]) for n in ("Integer_Wood_Shop_Problem", "Knapsack_1", "Cutting_stock")]
    items += plain
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack, host = _against_host(hip_lib, oracle_lib, items)
    lines = _launches(capfd)
    # at most one launch per build, the MIR LPs in the MIR builds and the plain LPs in the plain ones
    assert len(set((t, mir) for t, mir, _, _ in lines)) == len(lines) == pack.launches <= 4, lines
    assert sum(n for _, mir, n, _ in lines if mir) == len(items) - 3 and sum(n for _, mir, n, _ in lines if not mir) == 3, lines
    assert all(b <= LDS_LIMIT for _, _, _, b in lines)
    assert not pack.status.any()
    for i, c in enumerate(cases):
        M.check_fuzz_record(pack, i, items[i], c)
    for k, (name, _, c) in enumerate(records):
        M.check_fixture_record(pack, len(cases) + k, items[len(cases) + k], name, c)
    assert pack.mir[-3:].tobytes() == bytes(60) and (pack.mir["rounds"][:-3] > 0).all()
    assert int(pack.mir["rounds"].max()) >= 80 and int(pack.tree["iterations"].max()) >= 50
    pack.close()
    host.close()


# (height, width, first k structural variables integer, seed, row_extra): seeds searched on the CPU (tree_mir_util.round_log) for small trees
DENSE = [(70, 20, 10, 2, 30),      # one wave, rows selected and volume rows at index >= 64 (78 at most)
         (260, 20, 12, 10, 40),    # four waves, the same at index >= 256 (270 at most)
         (58, 20, 12, 9, 30),      # one wave, H crosses 64 through MIR rows
         (60, 63, 12, 25, None),   # four waves, the same
         (10, 63, 5, 40, 20), (10, 64, 5, 17, 20), (12, 65, 6, 1, 18),    # one wave, a row of 63 / 64 / 65 cells
         (20, 63, 10, 6, None), (20, 64, 10, 36, None), (20, 65, 10, 12, None),  # four waves
         (22, 64, 5, 28, 10), (22, 65, 5, 22, 10)]                         # 2048 / 2080 cells at the row capacity: both sides of the routing


def _many_eligible_item():
    """a round with more than 10 eligible rows needs more basic integer variables than the first k structural ones give: seed 5 of the
    30 x 20 tableau with every structural variable and the first 20 slacks declared integer -- 7 nodes, 13 rounds with up to 23 eligible rows"""
    m, vibr, vibc = generators.dense_resource_allocation_tableau(5, 19, 29)
    integers = [int(v) for v in vibc[1:]] + [int(v) for v in vibr[1:21]]
    return M.RawMirItem((m, vibr, vibc, []), integers, row_extra=120, cut_rows=40)


def test_lane_and_thread_edges(hip_lib, oracle_lib, monkeypatch, capfd):
    items = [M.dense_mir_item(h, w, k, seed, row_extra=extra) for h, w, k, seed, extra in DENSE] + [_many_eligible_item()]
    logs = [M.round_log(oracle_lib, it) for it in items]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack, host = _against_host(hip_lib, oracle_lib, items)
    lines = _launches(capfd)
    n_wave = sum(_cells(it) <= ROUTING_CELLS for it in items)
    assert sorted((t, mir, n) for t, mir, n, _ in lines) == [(64, True, n_wave), (256, True, len(items) - n_wave)] and 0 < n_wave < len(items), lines
    assert [_cells(it) for it in items[10:12]] == [2048, 2080]
    assert not host.status.any() and (host.tree["iterations"] >= 3).all() and (host.tree["iterations"] <= 200).all()
    # the conditions, on the oracle side: what each round saw before it appended its rows
    selected = lambda log: [r for _, eligible, _ in log for r in eligible[:10]]  # noqa: E731
    volume = lambda log: [r for _, _, rows in log for r in rows]  # noqa: E731
    assert _cells(items[0]) <= ROUTING_CELLS and max(selected(logs[0])) >= 64 and max(volume(logs[0])) >= 64
    assert _cells(items[1]) > ROUTING_CELLS and max(selected(logs[1])) >= 256 and max(volume(logs[1])) >= 256
    for i in (2, 3):
        assert items[i].lp[0].shape[0] < 64 < items[i].lp[0].shape[0] + int(host.mir[i]["rows_high_water"])
        assert any(h <= 64 < h + min(len(eligible), 10) for h, eligible, _ in logs[i]) or any(h > 64 for h, _, _ in logs[i])
    assert _cells(items[2]) <= ROUTING_CELLS < _cells(items[3])
    assert max(len(eligible) for _, eligible, _ in logs[12]) > 10 and 3 <= host.tree[12]["iterations"] <= 20
    assert sum(any(len(eligible) == 0 for _, eligible, _ in log) for log in logs) >= 5  # a round with no row still runs its simplex
    assert ((host.mir["root_rows"] > 0) & (host.tree["iterations"] > 1)).sum() >= 8      # a root that keeps MIR rows and then branches
    assert [sum(len(e[:10]) for _, e, _ in log) for log in logs] == host.mir["rows_added"].tolist()
    pack.close()
    host.close()


def _simplex_log(oracle_lib, item, monkeypatch):
    """(optimal, feasible, cycle_phase) of every simplex of the host tree on the oracle -- nodes, MIR rounds, the final re-evaluation -- in order"""
    log = []
    orig = Tableau._absorb
    monkeypatch.setattr(Tableau, "_absorb", lambda self, res: (log.append((res.optimal, res.feasible, res.cycle_phase)), orig(self, res))[1])
    M.solve(oracle_lib, [item]).close()
    monkeypatch.setattr(Tableau, "_absorb", orig)
    return log


def test_tree_edges_with_mir(hip_lib, oracle_lib, monkeypatch):
    mir = lambda model: M.MirItem(dict(model, options={"useMIRCuts": True}))  # noqa: E731
    items = [mir(BERLIN), mir(INFEASIBLE), mir(UNBOUNDED), mir(NO_INTEGRAL), mir(U.fixture("Integer_Wood_Shop_Problem")["model"])]
    g, m, vibr, vibc = _instance(CYCLE_GOLDENS[0])
    items.append(M.RawMirItem((m, vibr, vibc, g["tableau"]["unrestricted"]), [int(vibc[1])], precision=g["tableau"]["precision"], check=True))
    pack, host = _against_host(hip_lib, oracle_lib, items)
    t, r = pack.tree, pack.mir
    # integral at the root: no save, iterations == 1; the root's loop still ran
    assert (t[0]["iterations"], t[0]["is_integral"], t[0]["nodes_pushed"], r[0]["root_rows"]) == (1, 1, 1, 0) and r[0]["rounds"] >= 1
    assert U.result_of(pack, 0, items[0]) == {"feasible": True, "result": 1080000, "bounded": True, "isIntegral": True, "brit": 24, "yank": 20}
    # an infeasible root: the loop runs on it all the same (branch-and-cut.ts:38-52 has no feasibility test), and the tree ends
    assert t[1]["iterations"] == 1 and not pack.feasible[1] and not t[1]["is_integral"] and r[1]["rounds"] >= 1
    # an unbounded root: it stays unbounded through its rounds
    assert not pack.bounded[2] and pack.evaluation[2] == -np.inf and r[2]["rounds"] >= 1
    # no integral node, and a simplex inside the loop that reaches no optimum: 2 x + 2 y = 3 has a fractional root (the tree without MIR
    # branches on it and finds every leaf infeasible); its first MIR row proves that on the spot -- the round's simplex is infeasible, the
    # evaluation stays the root's, and the tree ends without a branch
    log = _simplex_log(oracle_lib, items[3], monkeypatch)
    assert [o for o, _, _ in log] == [1, 0, 0] and [f for _, f, _ in log] == [1, 0, 0]  # (the root, and two rounds: the second adds no row)
    assert (t[3]["iterations"], t[3]["is_integral"], r[3]["rounds"], r[3]["rows_added"], r[3]["simplexes"]) == (1, 0, 2, 1, 3) and not pack.feasible[3]
    assert pack.evaluation[3] == host.evaluation[3] != 0.0 and pack.results[3]["optimal"] == 0
    # a simplex inside the loop that reaches no optimum, between simplexes that do (the log holds every simplex: nodes and rounds)
    log = _simplex_log(oracle_lib, items[4], monkeypatch)
    flags = [o for o, _, _ in log]
    assert len(flags) == r[4]["simplexes"] > t[4]["iterations"] and any(not f for f in flags[1:-1]) and t[4]["is_integral"]
    # the cycling root: the root's simplex stops on a cycle in phase 2; the loop runs all the same, its round adds no row, and the round's
    # simplex -- with a history of its own -- goes on from the same tableau to the optimum, which is integral
    assert _simplex_log(oracle_lib, items[5], monkeypatch) == [(0, 0, 2), (1, 1, 0)]
    assert (t[5]["iterations"], t[5]["is_integral"], r[5]["rounds"], r[5]["rows_added"]) == (1, 1, 1, 0)
    assert pack.results[5]["cycle_phase"] == 0 and pack.feasible[5] and pack.results[5]["pivots_phase2"] > 0
    # the arena holds saved roots (with the roots' MIR rows): a second call asks for an upload, and gets on after it
    with pytest.raises(_capi.EngineError, match=r"\(-4\).*saved roots"):
        pack.branch_and_cut()
    pack.upload()
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    assert M.states(pack) == M.states(host)
    pack.close()
    host.close()


def test_per_lp_status(hip_lib, oracle_lib):
    """Knapsack_1's row_extra set exactly to its measure succeeds; set one lower, the LP between two neighbours gets JSLP_ERR_CAPACITY naming
    the LP and row_extra, its out / tree_out / MIR sentinels are untouched, and both neighbours are right"""
    records = {n: m for n, m, _ in M.fixture_mir_records()}
    wood = M.MirItem(records["Integer_Wood_Shop_Problem"])
    host = M.solve(oracle_lib, [wood, M.MirItem(records["Knapsack_1"]), wood])
    want = M.states(host)
    hw, cuts = int(host.mir[1]["rows_high_water"]), int(host.tree[1]["cuts_high_water"])
    assert hw >= 22 and 0 < cuts <= hw

    def run(row_extra):
        its = [wood, M.MirItem(records["Knapsack_1"], row_extra=row_extra, cut_rows=cuts), wood]
        pack = M.make_pack(hip_lib, its)
        out = np.zeros(3, dtype=_capi.RESULT_DTYPE)
        out["pivots_phase1"] = 777  # sentinels
        tree = np.full(3, 55, dtype=np.int32).repeat(6).view(_capi.TREE_DTYPE)
        mir = np.full(3, 66, dtype=np.int32).repeat(5).view(_capi.MIR_TREE_DTYPE)
        status = np.full(3, 7, dtype=np.int32)
        rc = hip_lib.jslpt_pack_branch_and_cut(pack._h, None, out.ctypes.data, tree.ctypes.data, _capi.ptr_i32(status), None)
        msg = hip_lib.jslp_last_error().decode()
        assert hip_lib.jslpc_pack_read_mir(pack._h, mir.ctypes.data) == _capi.JSLP_OK
        return pack, rc, out, tree, mir, status, msg

    pack, rc, out, tree, mir, status, _ = run(hw)
    assert rc == _capi.JSLP_OK and status.tolist() == [0, 0, 0]
    assert out[1].tobytes() == host.results[1].tobytes() and tree[1].tobytes() == host.tree[1].tobytes() and mir[1].tobytes() == host.mir[1].tobytes()
    pack.close()
    pack, rc, out, tree, mir, status, msg = run(hw - 1)
    assert rc == _capi.JSLP_ERR_CAPACITY and status.tolist() == [0, _capi.JSLP_ERR_CAPACITY, 0], status
    assert "LP 1" in msg and "row_extra" in msg, msg
    assert out[1]["pivots_phase1"] == 777 and out[1]["evaluation"] == 0 and tree[1].tobytes() == np.full(6, 55, dtype=np.int32).tobytes()
    assert mir[1].tobytes() == np.full(5, 66, dtype=np.int32).tobytes()
    for i in (0, 2):
        assert out[i].tobytes() == host.results[i].tobytes() and tree[i].tobytes() == host.tree[i].tobytes() and mir[i].tobytes() == host.mir[i].tobytes()
        pack.results[i], pack.tree[i] = out[i], tree[i]
        assert U.state(pack, i)["rhs"] == want[i]["rhs"] and U.state(pack, i)["trace"] == want[i]["trace"]
    pack.close()
    host.close()


def test_oversubscribed_mir_trees(hip_lib, oracle_lib, monkeypatch, capfd):
    records = [(n, m) for n, m, _ in M.fixture_mir_records() if n != "Knapsack_1"][:8]
    base = [M.MirItem(m, row_extra=40) for _, m in records]
    host = M.solve(oracle_lib, base, trace_cap=128, heap_cap=16)
    want = M.states(host)
    copies = 2048
    items = [base[i % 8] for i in range(copies * 8)]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = M.solve(hip_lib, items, trace_cap=128, heap_cap=16)
    lines = _launches(capfd)
    assert len(lines) == 1 and lines[0][:3] == (64, True, copies * 8), lines
    assert not pack.status.any()
    for j in range(8):  # the result structs and the counters of a fixture's copies, all at once
        assert pack.results[j::8].tobytes() == host.results[j].tobytes() * copies, records[j][0]
        assert pack.tree[j::8].tobytes() == host.tree[j].tobytes() * copies, records[j][0]
        assert pack.mir[j::8].tobytes() == host.mir[j].tobytes() * copies, records[j][0]
    for i in range(copies * 8):  # and every copy's RHS column, row map and trace
        assert M.state(pack, i) == want[i % 8], i
    pack.close()
    host.close()
    # isolation: a plain pack, a plain tree pack and a Solve on the same library are still right
    lps = TableauPack([it.lp for it in base], precision=[it.precision for it in base], lib=hip_lib, trace_cap=128)
    ref = TableauPack([it.lp for it in base], precision=[it.precision for it in base], lib=oracle_lib, trace_cap=128)
    assert lps.simplex().tobytes() == ref.simplex().tobytes()
    assert all(lps.read_rhs(i)[0].tobytes() == ref.read_rhs(i)[0].tobytes() for i in range(8))
    lps.close()
    ref.close()
    plain = [U.Item(U.fixture(n)["model"]) for n, _ in records]
    a, b = U.solve(hip_lib, plain), U.solve(oracle_lib, plain)
    assert U.states(a) == U.states(b)
    a.close()
    b.close()
    model = dict(U.fixture("Knapsack_1")["model"], options={"useMIRCuts": True})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (Solve's note on the presolve pre-pass)
        assert repr(Solve(model, lib=hip_lib)) == repr(Solve(model, lib=oracle_lib))


def test_create_time_refusals(hip_lib):
    it = M.MirItem(M.fixture_mir_records()[0][1])
    knapsack = M.fixture_mir_records()[U.TREE_FIXTURES.index("Knapsack_1")][1]
    with pytest.raises(_capi.EngineError, match=r"\(%d\).*LP 1.*row_extra" % _capi.JSLP_ERR_ARG):
        M.make_pack(hip_lib, [it, M.MirItem(knapsack, row_extra=19, cut_rows=20)])
    fits = M.MirItem(knapsack)
    assert hip_lib.jslpc_tree_lds_bytes(52, 51, 52 + fits.row_extra) <= LDS_LIMIT < hip_lib.jslpc_tree_lds_bytes(52, 51, 52 + fits.row_extra + 1)
    M.make_pack(hip_lib, [it, fits]).close()
    with pytest.raises(_capi.EngineError, match=r"\(%d\).*LP 1.*64 KiB" % _capi.JSLP_ERR_UNSUPPORTED):
        M.make_pack(hip_lib, [it, M.MirItem(knapsack, row_extra=fits.row_extra + 1)])
