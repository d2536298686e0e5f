"""The instances of tests/pack_edges.py are what their names say (CPU part of tests/test_pack_edges_gpu.py): the oracle makes the planted
first decision, the planted values are one ulp from their thresholds, every history instance has the class it is listed under, the
Klee-Minty pivot counts hold, every tree root ends at iteration 1 on the Python host tree, and the Python TableauPack restatement on the
oracle library agrees with single oracle engines on every case."""
import numpy as np
import pytest

import cycle_edges as E
import pack_edges as PE
from jslpsolver_amd import _capi
from jslpsolver_amd.engine import Tableau, TableauPack, pack_lds_bytes, tree_lds_bytes, tree_mir_lds_bytes


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
def test_shapes_sit_where_the_loops_turn():
    for s in PE.SHAPES.values():
        long_side = s.H if s.tall else s.W
        assert 0 < pack_lds_bytes(s.H, s.W) <= pack_lds_bytes(s.H, s.W, 2) <= PE.LDS_LIMIT
        assert 0 < tree_mir_lds_bytes(s.H, s.W, s.H + PE.TREE_ROWS) <= PE.LDS_LIMIT and 0 < tree_lds_bytes(s.H, s.W, s.H + PE.TREE_ROWS, 2) <= PE.LDS_LIMIT
        # the LP pack and the tree pack (2 rows more) run the shape in the same build
        assert (s.H * s.W <= PE.ROUTING_CELLS) == ((s.H + PE.TREE_ROWS) * s.W <= PE.ROUTING_CELLS) == (s.threads == 64)
        assert s.pos[0] == 1 and s.pos[-1] == long_side - 1 and all(0 < p < long_side for p in s.pos)
        e0, e1, e2 = PE.edge(s)
        # index e0 is the last thread's first turn, e1 thread 0's second, e2 thread 1's second (loops `i = 1 + tid; i += THREADS`)
        assert [(p - 1) % s.threads for p in (e0, e1, e2)] == [s.threads - 1, 0, 1] and [(p - 1) // s.threads for p in (e0, e1, e2)] == [0, 1, 1]
        assert {e0, e1, e2} <= set(s.pos)
        if not s.tall:  # partial pricing is on (simplex.ts:118-127: more than 2 x 50 columns) and a batch boundary lies inside a thread turn
            assert s.W - 1 > 100 and (e0 - 1) // 50 == (e1 - 1) // 50 == (e2 - 1) // 50
    assert set(PE.POS64) >= {1, 63, 64, 65, 66, 128, 129} and set(PE.POS256) >= {1, 64, 65, 128, 129, 192, 193, 255, 256, 257, 258}
    w = PE.SHAPES["WIDE64"]
    assert (50 - 1) % 64 < (64 - 1) % 64 and (100 - 1) // 64 == (101 - 1) // 64 == 1 and w.W > 101  # 50|51 in turn 0, 100|101 in turn 1
    grids = {(t, W): PE.update_grid(t, W) for t, _, W in PE.GATE_SHAPES}
    assert grids == {(64, 24): (32, 2), (64, 64): (64, 1), (64, 70): (64, 1), (256, 24): (32, 8), (256, 256): (256, 1), (256, 262): (256, 1)}
    for t, H, W in PE.GATE_SHAPES:
        assert (H * W <= PE.ROUTING_CELLS) == ((H + PE.TREE_ROWS) * W <= PE.ROUTING_CELLS) == (t == 64) and 0 < tree_mir_lds_bytes(H, W, H + 2) <= PE.LDS_LIMIT
        assert max(PE.C3, PE.NEGCOL + 1, max(PE._zcols(W))) < min(W, 51)  # (all in the first pricing batch)


def test_planted_values_are_what_they_say():
    P, B, A = PE.PREC, PE.BELOW, PE.ABOVE
    assert B < P < A and np.nextafter(B, 1.0) == P and np.nextafter(P, 1.0) == A
    assert A / 1.0 > P and P / 1.0 == P
    with np.errstate(over="ignore"):
        assert np.float64(1e301) / np.float64(2e-8) == PE.INF
    assert np.signbit(PE.NAN_NEG) and not np.signbit(PE.NAN_POS) and np.isnan(PE.NAN_NEG) and np.isnan(PE.NAN_POS)
    with np.errstate(divide="ignore"):
        assert -np.float64(-3.0) / np.float64(0.0) == PE.INF
    G = PE.GATE
    assert not abs(np.float64(G)) > G and not abs(np.float64(-G)) > G and abs(np.float64(PE.NEXT_UP)) > G
    assert np.nextafter(np.float64(PE.NEXT_UP), np.float64(0.0)) == G
    assert np.float64(0.5) - np.float64(1.0) * np.float64(0.5) == 0.0 and not np.signbit(np.float64(0.5) - np.float64(1.0) * np.float64(0.5))
    q = np.float64(PE.LZ_VAL) / np.float64(PE.LZ_QUOT)  # the lazily zeroed quotient: the entry passes the gate, its quotient is nonzero and does not
    assert abs(PE.LZ_VAL) > G and q != 0.0 and abs(q) <= G


# ---- first decisions ------------------------------------------------------------------------------------------------------------------
def _first(lib, case):
    t = Tableau(*case.lp, precision=case.precision, lib=lib, optional_objectives=case.optional)
    try:
        res = t.simplex(check_cycles=case.check)
        return res, t.pivot_trace().tolist(), t.download()[0]
    finally:
        t.close()


def _check_decision(case, res, trace):
    want = case.want
    if want[0] == "unbounded":
        assert trace == [] and not res.bounded and res.feasible and res.unbounded_var_index == want[1], (case.name, trace[:2])
    elif want[0] == "optimal":
        assert trace == [] and res.optimal and res.feasible and res.bounded, (case.name, trace[:2])
    elif want[0] == "infeasible":
        assert trace == [] and not res.feasible and res.pivots_phase1 == 0, (case.name, trace[:2])
    else:
        assert trace and trace[0][1] == want[1] and (want[0] is None or trace[0][0] == want[0]), (case.name, want, trace[:2])


@pytest.mark.parametrize("group", ["selection", "soft", "gate", "lazy_zero"])
def test_oracle_makes_the_planted_decision(oracle_lib, group):
    cases = {"selection": PE.selection_cases, "soft": PE.soft_cases, "gate": PE.gate_cases, "lazy_zero": PE.lazy_zero_cases}[group]()
    assert len(cases) == len({c.name for c in cases}) >= 14
    for case in cases:
        res, trace, final = _first(oracle_lib, case)
        _check_decision(case, res, trace)
        rule = case.name.split("_")[0]
        if group == "selection":
            assert (res.pivots_phase1 > 0) == (rule == "p1") or case.want[0] in ("infeasible", "optimal"), case.name
            assert case.shape.tall == (rule == "ratio" or case.name.startswith("p1_leave")), case.name
        if group == "soft":  # the cost row prices nothing: without its rows the LP is optimal at once
            bare = PE.Case(case.name, case.shape, case.lp, None)
            assert _first(oracle_lib, bare)[1] == [], case.name
        if group == "lazy_zero":  # one pivot; the quotient stays only when no row's gate is open
            cell = final[case.cell]
            assert len(trace) == 1 and (cell == case.quotient if case.kind.endswith("none") else (cell == 0.0 and not np.signbit(cell))), (case.name, cell)
            assert case.quotient != 0.0 and abs(case.quotient) <= PE.GATE


def test_selection_cases_cover_the_base_cases():
    from test_selection_edges import BASE_CASES
    names = {c.name.split("-")[0].split("@")[0] for c in PE.selection_cases()}
    assert {b for b in BASE_CASES} <= {n[:-len("+unr")] if n.endswith("+unr") else n for n in names}
    plain = [c for c in PE.selection_cases() if "+unr" not in c.name]
    for c in plain:  # every case without unrestricted variables has its "+unr" variant
        twin = c.name.replace("-" + c.shape.name, "+unr-" + c.shape.name)
        assert bool(c.lp[3]) != any(x.name == twin for x in PE.selection_cases()), c.name


def test_gate_cases_close_the_gate_they_name(oracle_lib):
    """replay of the oracle's trace with its own pivot(): per pivot the rows whose entry of the entering column fails `|k| > 1e-16`"""
    for case in PE.gate_cases():
        A, vibr, vibc, _ = case.lp
        res, trace, final = _first(oracle_lib, case)
        assert res.optimal and res.pivots_phase1 == 0 and np.isfinite(final).all(), case.name
        t = Tableau(A, vibr, vibc, [], precision=PE.PREC, lib=oracle_lib)
        closed = []
        try:
            for pr, pc in trace[:3]:
                col = t.download()[0][:, pc]
                closed.append([i for i in range(A.shape[0]) if not abs(col[i]) > PE.GATE])
                t.pivot(pr, pc)
        finally:
            t.close()
        r = case.row
        if case.kind == "closed":  # gate-free, gated (exactly row r), gate-free
            assert trace[1][1] == PE.C2 and trace[2][1] == PE.C3 and closed == [[], [r], []], (case.name, closed)
        elif case.kind == "edge_open":
            assert closed[0] == [], (case.name, closed)
        else:
            assert closed[0] == [r] and len(trace) >= 2, (case.name, closed)
    rows = {(t, H, W): PE.gate_rows(t, H, W) for t, H, W in PE.GATE_SHAPES}
    assert rows[(256, 90, 24)] == [1, 7, 8, 9, 89] and rows[(64, 20, 24)] == [1, 3, 19]  # both sides of the first boundary of the row grid


# ---- the history -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pivots", [(5, 31), (7, 127), (9, 511), (12, 4095), (13, 8191)])
def test_klee_minty_pivot_counts(oracle_lib, n, pivots):
    lp = PE.km_lp(n)
    assert lp[0].shape == (n + 1, n + 1)
    t = Tableau(*lp, precision=PE.PREC, lib=oracle_lib)
    try:
        res = t.simplex(check_cycles=False)
        assert res.optimal and (res.pivots_phase1, res.pivots_phase2) == (0, pivots)
    finally:
        t.close()


def test_history_instances_have_their_class(oracle_lib):
    cases = PE.history_cases(oracle_lib)
    seen = {}
    for c in cases:
        n, start, length, p1, p2 = PE.run_history(oracle_lib, c.lp)
        assert n is not None and p1 == 0 and p2 == n - 1, c.name
        assert E.classify(n, start, length, PE.PK_HIST) == c.spec.want, (c.name, n, start, length)
        seen.setdefault(c.spec.want, set()).add(c.threads)
        assert c.threads == c.tree_threads and pack_lds_bytes(*c.lp[0].shape, 1) <= PE.LDS_LIMIT
    classes = {"below", "n == B", "n == B + 1", "between the copies", "first copy across", "second copy across", "beyond"}
    assert seen == {k: {64, 256} for k in classes}  # each class once under and once above 2048 cells
    table = {c.spec.k: PE.run_history(oracle_lib, c.lp)[:3] for c in cases if c.spec.small == "unr_3" and c.spec.blocks == PE.SMALL_BLOCKS}
    assert [table[k] for k in range(2, 8)] == [(124 + k, 120 + k, 2) for k in range(2, 8)]
    lengths = {c.spec.small: PE.run_history(oracle_lib, c.lp)[2] for c in cases}
    assert lengths == {"unr_3": 2, "deg_178868": 6, "deg_233528": 7}


@pytest.mark.parametrize("pad", [0, PE.CAP_PAD])
def test_capacity_instances_pivot_counts(oracle_lib, pad):
    """4095, 4096, 4097 phase-2 pivots (the check off: the oracle's own check is quadratic); padded, the same pivots above 2048 cells"""
    traces = []
    for k in (0, 1, 2):
        lp = PE.capacity_lp(k, pad)
        assert lp[0].shape == (13 + k + pad, 13 + k + pad) and (lp[0].size > PE.ROUTING_CELLS) == bool(pad)
        trace, _, n = PE.truncated_replay(oracle_lib, lp, PE.HIST_CAP)
        assert n == 4095 + k and len(trace) == min(n, PE.HIST_CAP)
        traces.append(trace)
    if pad:
        assert traces[2].tobytes() == PE.truncated_replay(oracle_lib, PE.capacity_lp(2), PE.HIST_CAP)[0].tobytes()


@pytest.mark.slow
@pytest.mark.parametrize("k", [0, 1])
def test_capacity_instances_have_no_cycle(oracle_lib, k):
    """with the check on the oracle (history of 2^20 pairs) ends optimal with the state of the check-off run: what the GPU part holds the
    packs' check-on runs of k = 0 and 1 against"""
    lp = PE.capacity_lp(k)
    on = PE.engine_state(oracle_lib, lp, check=True)
    assert on == PE.engine_state(oracle_lib, lp, check=False) and on["res"]["optimal"] and on["res"]["pivots_phase2"] == 4095 + k


# ---- tree roots ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PE.TREE_KINDS)
def test_every_tree_root_ends_at_iteration_1(oracle_lib, kind):
    cases = PE.lp_cases(oracle_lib)
    items = PE.tree_items(oracle_lib, kind)
    assert PE.LP_ONLY == () and len(items) == len(cases) - (0 if kind == "opt" else len(PE.soft_cases()))  # no case is left out of any build
    assert sum(not it.case.finite for it in items) == sum(not c.finite for c in cases) >= 25
    pack = PE.tree_pack(oracle_lib, items, kind)
    try:
        pack.branch_and_cut(check_cycles=[it.check for it in items])
        assert not pack.status.any()
        assert pack.tree["iterations"].tolist() == [1] * len(items)
        for i, it in enumerate(items):  # the root is the case's own solve
            lone = PE.engine_state(oracle_lib, it.lp, it.precision, it.check, it.optional, row_capacity=it.lp[0].shape[0] + PE.TREE_ROWS)
            trace = pack.pivot_trace(i).astype(np.int32).tobytes()  # (a MIR root goes on with its rounds of cuts)
            assert trace == lone["trace"] or (kind == "mir" and trace.startswith(lone["trace"])), it.case.name
            assert it.case.tree_threads == it.case.threads, it.case.name
    finally:
        pack.close()


# ---- the restated pack against single engines --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [False, True])
def test_restated_pack_equals_single_engines(oracle_lib, opt):
    cases = [c for c in PE.lp_cases(oracle_lib) if opt or c.optional is None]
    rows = [c.with_zero_row() if opt else None for c in cases]
    pack = TableauPack([c.lp for c in cases], precision=[c.precision for c in cases], lib=oracle_lib, trace_cap=512,
                       optional_objectives=rows if opt else None)
    try:
        pack.simplex(check_cycles=[c.check for c in cases])
        assert not pack.status.any()
        for i, c in enumerate(cases):
            want = PE.engine_state(oracle_lib, c.lp, c.precision, c.check, rows[i])
            got = PE.pack_lp_state(pack, i, opt)
            assert got == want, (c.name, PE.differing(got, want))
            if opt and c.optional is None:  # the all-zero row changes nothing
                bare = PE.engine_state(oracle_lib, c.lp, c.precision, c.check)
                assert {k: v for k, v in want.items() if k != "optional"} == {k: v for k, v in bare.items() if k != "optional"}, c.name
                assert want["optional"] == bytes(8 * c.lp[0].shape[1])
    finally:
        pack.close()


def test_pivot_cap_instances(oracle_lib):
    """max_pivots 1 and 2: the LPs make more pivots than that, the phase-1 one in phase 1"""
    for c in PE.pivot_cap_cases():
        trace, _, n = PE.truncated_replay(oracle_lib, c.lp, 2, check=False)
        assert n > 2 and len(trace) == 2, c.name
        if c.name.startswith("phase1"):
            assert _first(oracle_lib, c)[0].pivots_phase1 >= 2, c.name
    assert _capi.JSLP_ERR_CAPACITY == -5
