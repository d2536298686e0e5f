"""Shared by tests/test_packed_soft_*.py: packs whose LPs carry optional objectives (include/jslps_soft.h) -- the inputs (the reference's
recorded soft-constraint runs, the same models without their main objective, dense tableaus with small-integer optional rows), the
yardsticks computed ONCE on the CPU oracle, and the state a solved pack leaves, as bytes.  Builds on tree_pack_util."""
import copy
import functools

import numpy as np

import tree_pack_util as U
from jslpsolver_amd import branch_and_cut as bc
from jslpsolver_amd import generators
from jslpsolver_amd.engine import TableauPack, tree_cut_rows
from jslpsolver_amd.model import Model
from jslpsolver_amd.solver import _tree_in_scope

SOFT_FIXTURES = ["Relaxed", "Fertilizer"]
PLAIN_LP_FIXTURES = ["Berlin_Air_Lift_Problem", "Unrestricted", "Wiki_1"]


class SoftItem(U.Item):
    """one model as a pack takes it, with its optional objectives (None: it has none)"""

    def __init__(self, model_json, keep=None):
        U.Item.__init__(self, model_json, cut_rows=0)
        _, rows = self.model.optional_objectives()
        if keep is not None:
            rows = rows[:keep]
        self.optional = np.ascontiguousarray(rows, dtype=np.float64) if rows is not None and len(rows) > 0 else None
        self.n_optional = 0 if self.optional is None else self.optional.shape[0]
        h, w = self.lp[0].shape
        self.cut_rows = tree_cut_rows(h, w, len(self.integers), n_optional=self.n_optional)


class RawSoftItem(U.RawItem):
    """a tableau with optional rows and some variables declared integer (no model behind it)"""

    def __init__(self, lp, optional, integers=(), cut_rows=None, precision=1e-8, check=True):
        U.RawItem.__init__(self, lp, integers, cut_rows=cut_rows, precision=precision, check=check)
        self.optional = None if optional is None or len(optional) == 0 else np.ascontiguousarray(optional, dtype=np.float64)
        self.n_optional = 0 if self.optional is None else self.optional.shape[0]


def without_rows(item, keep=0):
    """the same LP with only its first `keep` optional rows"""
    it = copy.copy(item)
    it.optional = item.optional[:keep] if item.optional is not None and keep > 0 else None
    it.n_optional = 0 if it.optional is None else it.optional.shape[0]
    return it


def strip_objective(model_json):
    """set B: the `optimize` attribute's coefficient deleted from every variable -- the main cost row is zero, the optional rows decide"""
    m = copy.deepcopy(model_json)
    for var in m["variables"].values():
        var.pop(m["optimize"], None)
    return m


@functools.lru_cache(maxsize=None)
def soft_records():
    """the recorded soft runs that need neither options nor presolve and have optional objectives: (plain LPs, MILPs under the default service)"""
    lps, milps = [], []
    for c in U._cases("fuzz_soft.jsonl.gz"):
        if c["model"].get("options") or c["fixed"] != 0 or c["infeasPre"]:
            continue
        m = Model(c["model"], None)
        _, oo = m.optional_objectives()
        if oo is None or len(oo) == 0:
            continue
        if len(m.integerVariables) == 0:
            lps.append(c)
        elif _tree_in_scope(m):
            milps.append(c)
    return lps, milps


@functools.lru_cache(maxsize=None)
def plain_records():
    """recorded runs WITHOUT optional objectives, as neighbours in a pack: (plain LPs, MILPs)"""
    lps, milps = [], []
    for c in U._cases("fuzz_soft.jsonl.gz"):
        if c["model"].get("options") or c["fixed"] != 0 or c["infeasPre"]:
            continue
        m = Model(c["model"], None)
        _, oo = m.optional_objectives()
        if oo is not None and len(oo) > 0:
            continue
        if len(m.integerVariables) == 0:
            lps.append(c)
        elif _tree_in_scope(m):
            milps.append(c)
    return lps[:12], milps[:12]


@functools.lru_cache(maxsize=None)
def items_a():
    lps, milps = soft_records()
    return [SoftItem(c["model"]) for c in lps], [SoftItem(c["model"]) for c in milps]


@functools.lru_cache(maxsize=None)
def items_b():
    lps, milps = soft_records()
    return [SoftItem(strip_objective(c["model"])) for c in lps], [SoftItem(strip_objective(c["model"])) for c in milps]


def lp_pack(lib, items, trace_cap=4096, max_pivots=0):
    return TableauPack([it.lp for it in items], precision=[it.precision for it in items], lib=lib, trace_cap=trace_cap, max_pivots=max_pivots,
                       optional_objectives=[it.optional for it in items])


def tree_pack(lib, items, trace_cap=8192, heap_cap=256, max_nodes=0):
    return TableauPack([it.lp for it in items], precision=[it.precision for it in items], lib=lib, trace_cap=trace_cap,
                       integers=[it.integers for it in items], cut_rows=[it.cut_rows for it in items], heap_cap=heap_cap, max_nodes=max_nodes,
                       optional_objectives=[it.optional for it in items])


def solve_lps(lib, items, **kw):
    pack = lp_pack(lib, items, **kw)
    pack.simplex(check_cycles=[it.check for it in items])
    return pack


def solve_trees(lib, items, **kw):
    pack = tree_pack(lib, items, **kw)
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    return pack


def lp_state(pack, i):
    """everything simplex() leaves of LP i, as bytes: the result struct, the final tableau, the four maps, the optional rows, the trace"""
    m, vibr, vibc, rbv, cbv = pack.download(i)
    return dict(res=pack.results[i].tobytes(), matrix=m.tobytes(), vibr=vibr.tobytes(), vibc=vibc.tobytes(), rbv=rbv.tobytes(), cbv=cbv.tobytes(),
                rhs=b"".join(a.tobytes() for a in pack.read_rhs(i)), optional=pack.optional_objectives(i).tobytes(),
                trace=np.ascontiguousarray(pack.pivot_trace(i), dtype=np.int32).tobytes())


def tree_state(pack, i):
    """U.state -- the result struct, the tree counters, the evaluation, the RHS column, the row map, the trace -- and the optional rows"""
    return dict(U.state(pack, i), optional=pack.optional_objectives(i).tobytes())


def lp_states(pack):
    return [lp_state(pack, i) for i in range(len(pack))]


def tree_states(pack):
    return [tree_state(pack, i) for i in range(len(pack))]


def traces(pack):
    return [np.ascontiguousarray(pack.pivot_trace(i), dtype=np.int32).tobytes() for i in range(len(pack))]


def assert_same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "%s: LP %d differs from the oracle in %s" % (what, i, [k for k in a if a[k] != b[k]])
    assert len(got) == len(want)


def tie_counts(lib, items):
    """per tree of the host walk on `lib`: (ties reached with optional objectives, ties won on one), from branch_and_cut.TIE_STATS"""
    out = []
    for it in items:
        bc.TIE_STATS["ties"] = bc.TIE_STATS["won"] = 0
        solve_trees(lib, [it]).close()
        out.append((bc.TIE_STATS["ties"], bc.TIE_STATS["won"]))
    return out


# ---- shape edges: dense tableaus with the cost row zeroed and small-integer optional rows with planted zeros ---------------------------------
def dense_soft(h, w, n_opt, seed, k_int=0, cut_rows=None, zero_cost=True):
    """generators.dense_resource_allocation_tableau (h x w) with its cost row zeroed and n_opt optional rows of small integers in which
    about a third of the cells are exact zeros, so that a pivot meets `coefficient == 0` and `v0 == 0` as well as their opposites"""
    m, vibr, vibc = generators.dense_resource_allocation_tableau(seed, w - 1, h - 1)
    assert m.shape == (h, w)
    m = m.copy()
    if zero_cost:
        m[0, :] = 0.0
    rng = np.random.RandomState(1000 + seed)
    rows = rng.randint(-4, 5, size=(n_opt, w)).astype(np.float64)
    rows[rng.rand(n_opt, w) < 0.33] = 0.0
    rows[:, 0] = 0.0
    return RawSoftItem((m, vibr, vibc, []), rows, integers=[int(v) for v in vibc[1:1 + k_int]], cut_rows=cut_rows)


# (height, width, optional rows, seed): a row of 63 / 64 / 65 cells in the one-wave build (H = 10) and in the four-wave build (H = 40);
# width 102, the first with partial pricing (nColumns > 2 * 50), 8 rows for one wave and 24 for four.  Seeds picked on the CPU: the trace of
# each differs from its trace without the rows (tests/test_packed_soft_cpu.py asserts it)
DENSE_LPS = [(10, 63, 1, 2), (10, 64, 2, 3), (10, 65, 3, 1), (40, 63, 3, 2), (40, 64, 1, 3), (40, 65, 2, 1), (8, 102, 2, 3), (24, 102, 3, 1)]
# (height, width, optional rows, seed, integer variables): height + cuts crosses 64 rows during the tree, one case per build
DENSE_TREES = [(62, 20, 2, 1, 10), (62, 63, 2, 2, 10)]


def dense_lp_items():
    return [dense_soft(h, w, n, seed) for h, w, n, seed in DENSE_LPS]


def dense_tree_items():
    return [dense_soft(h, w, n, seed, k_int=k, zero_cost=False) for h, w, n, seed, k in DENSE_TREES]
