"""include/jslpb_big_lds.h on the MI355X: LPs and trees whose LDS image lies between 64 KiB and 156 KiB, in the large builds of
k_simplex_packed and k_tree_packed (one workgroup of jslpb_pack_big_threads() threads with a compute unit's LDS to itself).

The yardsticks are the reference's goldens, the CPU oracle (an engine per LP; the Python host tree for the trees) and a twin `Tableau` on the
HIP engine.  A large pack is never compared with another pack -- the one place where two packs meet (Knapsack_1 in the large and in the
256-thread build) holds both to the golden first.  The JSLP_DEBUG_LAUNCH lines say which builds ran, with how many LPs and how much LDS.
Every pack has an explicit max_pivots (and a tree pack max_nodes): a wrong build ends at a cap, not in a long loop."""
import re

import pytest

import golden_util as G
import soft_pack_util as S
import tree_pack_util as U
from jslpsolver_amd import _capi, generators, solver
from jslpsolver_amd.engine import Tableau, TableauPack, pack_lds_bytes, tree_lds_bytes
from test_many_gpu import _check_golden
from test_packed_gpu import _Lp, _engine_state, _golden_lp, _pack_state, _state_of

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[jslp\] launch (k_simplex_packed|k_tree_packed)<(\d+)(,opt 1)?> n (\d+) lds (\d+)")
SMALL, LIMIT = 65536, 159744
MAX_PIVOTS, MAX_NODES = 20000, 4096


def _launches(capfd):
    return [(k, int(t), bool(o), int(n), int(b)) for k, t, o, n, b in LAUNCH.findall(capfd.readouterr().err)]


def _dense(h, w, seed=4242):
    m, vibr, vibc = generators.dense_resource_allocation_tableau(seed + 131 * h + w, w - 1, h - 1)
    assert m.shape == (h, w)
    return (m, vibr, vibc, []), 1e-8, True


def _big_pack(hip_lib, items, max_pivots=MAX_PIVOTS, **kw):
    return TableauPack([lp for lp, _, _ in items], precision=[p for _, p, _ in items], lib=hip_lib, trace_cap=4096, max_pivots=max_pivots, big_lds=True, **kw)


@pytest.fixture(scope="module")
def T(hip_lib):
    return int(hip_lib.jslpb_pack_big_threads())


def test_sudoku_root_in_the_large_build(hip_lib, T, monkeypatch, capfd):
    g = U.fixture("Sudoku4x4")
    lp, p, c = _golden_lp(g)
    assert lp[0].shape == (193, 65) and pack_lds_bytes(193, 65) == 107072
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = _big_pack(hip_lib, [(lp, p, c)])
    pack.simplex(check_cycles=c)
    assert _launches(capfd) == [("k_simplex_packed", T, False, 1, 107072)] and pack.launches == 1 and pack.is_big.all()
    assert g["nPivots"] == 164 and len(g["simplexCalls"]) == 1
    _check_golden(_Lp(pack, 0), pack.result(0), g)  # 164 pivots, the digest, the final tableau
    assert _pack_state(pack, 0) == _engine_state(hip_lib, lp, p, c)
    pack.close()


def test_the_three_classes_in_one_pack(hip_lib, oracle_lib, T, monkeypatch, capfd):
    berlin = _golden_lp(U.fixture("Berlin_Air_Lift_Problem"))
    items = [_dense(138, 138), berlin, _dense(88, 88), _dense(87, 87)]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = _big_pack(hip_lib, items)
    pack.simplex(check_cycles=[c for _, _, c in items])
    lines = _launches(capfd)
    assert lines == [("k_simplex_packed", 64, False, 1, pack_lds_bytes(*berlin[0][0].shape)), ("k_simplex_packed", 256, False, 1, 64336),
                     ("k_simplex_packed", T, False, 2, 159424)] and pack.launches == 3, lines
    assert pack.is_big.tolist() == [True, False, True, False]
    for i, (lp, p, c) in enumerate(items):  # (in input order, whatever the launch order)
        assert _pack_state(pack, i) == _engine_state(oracle_lib, lp, p, c), "LP %d differs from the oracle" % i
        assert _pack_state(pack, i) == _engine_state(hip_lib, lp, p, c), "LP %d differs from its twin engine" % i
    pack.close()


def _edge_items(oracle_lib):
    un = generators.unrestricted_resource_allocation_tableau(77, 110, 90, 12)
    infeasible = _dense(100, 120, seed=7)
    infeasible[0][0][37, 0] = -5.0  # a row of positive coefficients with a negative right-hand side: phase 1 finds no entering column
    unbounded = _dense(100, 120, seed=8)
    unbounded[0][0][1:, 50] *= -1.0  # a profitable column that no row limits
    items = {"138 x 138": _dense(138, 138, seed=11), "tall 1563 x 8": _dense(1563, 8), "wide 7 x 2001": _dense(7, 2001),
             "unrestricted": ((un[0], un[1], un[2], list(un[3])), 1e-8, True), "infeasible": infeasible, "unbounded": unbounded}
    for name, (lp, _, _) in items.items():
        assert SMALL < pack_lds_bytes(*lp[0].shape) <= LIMIT, name
    assert pack_lds_bytes(1563, 8) == 159552 and pack_lds_bytes(7, 2001) == 138352
    return items


def test_edges_of_the_template_at_the_large_thread_count(hip_lib, oracle_lib, T, monkeypatch, capfd):
    """the largest image (static plus dynamic LDS at the compute unit's limit), fewer columns than one wave (RP at its largest), more columns
    than the workgroup, unrestricted variables, and the two outcomes that are not an optimum; each with a second simplex() without upload and
    the whole matrix read back"""
    items = _edge_items(oracle_lib)
    names = list(items)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = _big_pack(hip_lib, [items[n] for n in names])
    pack.simplex(check_cycles=True)
    assert _launches(capfd) == [("k_simplex_packed", T, False, len(names), 159552)] and pack.is_big.all()
    first = {n: _engine_state(oracle_lib, *items[n]) for n in names}
    for i, n in enumerate(names):
        got = _pack_state(pack, i)
        assert got == first[n], "%s differs from the oracle in %s" % (n, [k for k in got if got[k] != first[n][k]])
    res = {n: pack.result(i) for i, n in enumerate(names)}
    assert not res["infeasible"].feasible and res["unbounded"].feasible and not res["unbounded"].bounded  # (as the oracle says: the states are equal)
    assert res["138 x 138"].optimal and res["tall 1563 x 8"].optimal and res["wide 7 x 2001"].optimal and res["unrestricted"].optimal
    assert all(res[n].pivots_phase1 + res[n].pivots_phase2 > 0 for n in names if n != "infeasible")
    pack.simplex(check_cycles=True)
    for i, n in enumerate(names):
        assert _pack_state(pack, i) == _engine_state(oracle_lib, *items[n], calls=2), "%s: the second call differs from the oracle" % n
    pack.close()


def test_optional_objectives_in_the_large_build(hip_lib, oracle_lib, T, monkeypatch, capfd):
    m, vibr, vibc, oo = generators.soft_resource_allocation_tableau(5, 100, 110, 3)
    assert oo.shape == (3, m.shape[1]) and SMALL < pack_lds_bytes(m.shape[0], m.shape[1], 3) <= LIMIT
    item = S.RawSoftItem((m, vibr, vibc, []), oo)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = TableauPack([item.lp], lib=hip_lib, trace_cap=4096, max_pivots=MAX_PIVOTS, optional_objectives=[item.optional], big_lds=True)
    pack.simplex(check_cycles=True)
    assert _launches(capfd) == [("k_simplex_packed", T, True, 1, pack_lds_bytes(m.shape[0], m.shape[1], 3))]
    for lib in (oracle_lib, hip_lib):  # an engine with set_optional_objectives: the state and the optional rows
        t = Tableau(*item.lp, lib=lib, optional_objectives=item.optional)
        r = t.simplex(check_cycles=True)
        assert _pack_state(pack, 0) == _state_of(r, t.evaluation, t.read_rhs(), t.pivot_trace(), t.download())
        assert pack.optional_objectives(0).tobytes() == t.optional_objectives().tobytes()
        assert r.pivots_phase1 + r.pivots_phase2 > 0
        t.close()
    pack.close()


def _knapsack(hip_lib, cut_rows, big_lds):
    g = U.fixture("Knapsack_1")
    item = U.Item(g["model"], cut_rows=cut_rows)
    pack = TableauPack([item.lp], precision=[item.precision], lib=hip_lib, trace_cap=8192, max_pivots=MAX_PIVOTS, integers=[item.integers],
                       cut_rows=[item.cut_rows], heap_cap=256, max_nodes=MAX_NODES, big_lds=big_lds)
    pack.branch_and_cut(check_cycles=item.check)
    assert g["nPivots"] == 500 and len(g["simplexCalls"]) == 80
    U.check_record(pack, 0, item, g["nPivots"], g["pivotDigest"], g["final"]["branchAndCutIterations"], g["resultKeys"], g["result"], "Knapsack_1")
    assert pack.pivot_trace(0).reshape(-1).tolist() == g["pivots"]
    return pack, item


def test_knapsack_tree_in_the_large_build(hip_lib, T, monkeypatch, capfd):
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    big, item = _knapsack(hip_lib, 200, True)
    assert _launches(capfd) == [("k_tree_packed", T, False, 1, 111088)] and tree_lds_bytes(52, 51, 252) == 111088
    small, item0 = _knapsack(hip_lib, None, False)
    assert item0.cut_rows == 96 and _launches(capfd) == [("k_tree_packed", 256, False, 1, tree_lds_bytes(52, 51, 148))]
    # two kernels, each held to the golden above: their read-backs agree field by field
    a, b = U.state(big, 0), U.state(small, 0)
    assert a == b, [k for k in a if a[k] != b[k]]
    big.close()
    small.close()


def test_sudoku_through_solve_packed(hip_lib, T, monkeypatch, capfd):
    g = U.fixture("Sudoku4x4")
    monkeypatch.setattr(solver, "TREE_MAX_NODES", MAX_NODES)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    got = solver.solve_packed([g["model"]], lib=hip_lib, big_lds=True)[0]
    assert _launches(capfd) == [("k_tree_packed", T, False, 1, 159296)]  # 95 cut rows: row capacity 288
    assert list(got.keys()) == g["resultKeys"]
    for k, v in g["result"].items():
        assert got[k] == (v if isinstance(v, bool) else G.num(v)), k


def test_soft_trees_in_the_large_opt_build(hip_lib, oracle_lib, T, monkeypatch, capfd):
    """Fertilizer (soft constraints; its tree is its root) at a row capacity that carries its image over 64 KiB, against its golden; and a
    dense tableau with two optional rows and ten integer variables, whose tree branches, against the host tree on the oracle"""
    g = U.fixture("Fertilizer")
    fert = S.SoftItem(g["model"])
    fert.cut_rows = 1000
    dense = S.dense_soft(62, 63, 2, 2, k_int=10, cut_rows=70, zero_cost=False)
    assert tree_lds_bytes(9, 8, 1009, 2) == 103200 and tree_lds_bytes(62, 63, 132, 2) == 72368 and fert.n_optional == 2
    items = [fert, dense]
    kw = dict(trace_cap=8192, max_pivots=MAX_PIVOTS, heap_cap=256, max_nodes=MAX_NODES, big_lds=True)

    def solve(lib):
        pack = TableauPack([it.lp for it in items], precision=[it.precision for it in items], lib=lib, integers=[it.integers for it in items],
                           cut_rows=[it.cut_rows for it in items], optional_objectives=[it.optional for it in items], **kw)
        pack.branch_and_cut(check_cycles=[it.check for it in items])
        return pack
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = solve(hip_lib)
    assert _launches(capfd) == [("k_tree_packed", T, True, 2, 103200)]
    U.check_record(pack, 0, fert, g["nPivots"], g["pivotDigest"], None, g["resultKeys"], g["result"], "Fertilizer")
    host = solve(oracle_lib)
    S.assert_same(S.tree_states(pack), S.tree_states(host), "large OPT trees")
    assert int(pack.tree["iterations"][1]) > 1 and int(pack.tree["nodes_pushed"][1]) > 1  # (the dense tree branches)
    pack.close()
    host.close()


def test_a_cap_in_a_large_lp(hip_lib, oracle_lib, T):
    """a large LP with max_pivots = 3 between two neighbours that need no more: JSLP_ERR_CAPACITY is its alone, and its tableau is what
    three pivots leave on the oracle"""
    small = _golden_lp(U.fixture("Chocolate_Problem"))
    big = _dense(138, 138)
    items = [small, big, small]
    ref = _engine_state(oracle_lib, *small)
    assert len(ref["trace"]) // 8 == 2  # (int32 pairs: two pivots, and the call that finds the optimum is within the cap)
    pack = _big_pack(hip_lib, items, max_pivots=3)
    with pytest.raises(_capi.EngineError, match="LP 1"):
        pack.simplex(check_cycles=True)
    assert pack.status.tolist() == [_capi.JSLP_OK, _capi.JSLP_ERR_CAPACITY, _capi.JSLP_OK]
    for i in (0, 2):
        assert _pack_state(pack, i) == ref
    # the oracle's engine, pivoted by hand along the first three pivots of its own solve
    t = Tableau(*big[0], lib=oracle_lib)
    t.simplex(check_cycles=True)
    first3 = t.pivot_trace()[:3]
    t.upload(*big[0])
    for r, c in first3:
        t.pivot(int(r), int(c))
    want = t.download()
    t.close()
    assert pack.pivot_trace(1).tolist() == first3.tolist()
    for a, b in zip(pack.download(1), want):
        assert a.tobytes() == b.tobytes()
    pack.close()


def test_a_big_lds_pack_of_small_lps_launches_what_it_launched(hip_lib, oracle_lib, monkeypatch, capfd):
    items = [_dense(87, 87), _golden_lp(U.fixture("Wiki_1")), _dense(40, 60), _golden_lp(U.fixture("Berlin_Air_Lift_Problem"))]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    lines = []
    for big_lds in (False, True):
        capfd.readouterr()
        pack = TableauPack([lp for lp, _, _ in items], precision=[p for _, p, _ in items], lib=hip_lib, trace_cap=4096, max_pivots=MAX_PIVOTS, big_lds=big_lds)
        pack.simplex(check_cycles=[c for _, _, c in items])
        lines.append(_launches(capfd))
        assert not pack.is_big.any() and pack.launches == 2
        for i, (lp, p, c) in enumerate(items):
            assert _pack_state(pack, i) == _engine_state(oracle_lib, lp, p, c), i
        pack.close()
    assert lines[0] == lines[1] and [t for _, t, _, _, _ in lines[1]] == [64, 256] and max(b for _, _, _, _, b in lines[1]) == 64336
