"""Shared by tests/test_tree_packed_cpu.py and tests/test_tree_packed_gpu.py: building the LPs of a pack with trees (include/jslpt_tree.h)
from JSON models, the reference's recorded runs they are held against, and the state a solved pack leaves, as bytes."""
import gzip
import json
import os

import numpy as np

import golden_util as G
from jslpsolver_amd import generators, pivot_digest
from jslpsolver_amd.engine import TableauPack, tree_cut_rows
from jslpsolver_amd.model import Model
from jslpsolver_amd.solver import _PackedLp, _solve_on, _tree_in_scope

TREE_FIXTURES = ["Cutting_stock", "Integer_Berlin_Air_Lift_Problem", "Integer_Chocolate_Problem", "Integer_Clothing_Shop_Problem",
                 "Integer_Clothing_Shop_Problem_II", "Integer_Sports_Complex_Problem", "Integer_Wood_Problem", "Integer_Wood_Shop_Problem",
                 "Knapsack_1", "TacoParty"]


class Item:
    """one model as a pack takes it"""

    def __init__(self, model_json, cut_rows=None, integers=None):
        self.model = Model(model_json, None)
        matrix, vibr, vibc = self.model.build_tableau()
        self.lp = (matrix, vibr, vibc, list(self.model.unrestricted))
        self.integers = [v["index"] for v in self.model.integerVariables] if integers is None else list(integers)
        self.cut_rows = tree_cut_rows(matrix.shape[0], matrix.shape[1], len(self.integers)) if cut_rows is None else cut_rows
        self.precision = self.model.precision
        self.check = bool(self.model.checkForCycles)


class RawItem:
    """a tableau with some variables declared integer (no model behind it)"""

    def __init__(self, lp, integers, cut_rows=None, precision=1e-8, check=True):
        self.lp, self.integers, self.precision, self.check = lp, list(integers), precision, check
        self.cut_rows = 2 * len(self.integers) if cut_rows is None else cut_rows


def dense_item(h, w, k, seed, cut_rows=None):
    """generators.dense_resource_allocation_tableau with its first k structural variables declared integer"""
    m, vibr, vibc = generators.dense_resource_allocation_tableau(seed, w - 1, h - 1)
    assert m.shape == (h, w)
    return RawItem((m, vibr, vibc, []), [int(v) for v in vibc[1:1 + k]], cut_rows=cut_rows)


def make_pack(lib, items, trace_cap=8192, heap_cap=256, max_nodes=0, max_pivots=0):
    return TableauPack([it.lp for it in items], precision=[it.precision for it in items], lib=lib, trace_cap=trace_cap, max_pivots=max_pivots,
                       integers=[it.integers for it in items], cut_rows=[it.cut_rows for it in items], heap_cap=heap_cap, max_nodes=max_nodes)


def solve(lib, items, **kw):
    pack = make_pack(lib, items, **kw)
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    return pack


def state(pack, i):
    """everything the tree of LP i leaves, as bytes (NaN compares equal to itself)"""
    rhs, rows = pack.read_rhs(i)
    return dict(res=pack.results[i].tobytes(), tree=pack.tree[i].tobytes(), evaluation=np.float64(pack.evaluation[i]).tobytes(),
                rhs=rhs.tobytes(), rows=rows.tobytes(), trace=np.ascontiguousarray(pack.pivot_trace(i), dtype=np.int32).tobytes())


def states(pack):
    return [state(pack, i) for i in range(len(pack))]


def result_of(pack, i, item):
    """the result object Solve builds, from LP i of a solved pack"""
    return _solve_on(_PackedLp(pack, i), item.model, 0, False, 1, None, False, simplex_done=True, integral=bool(pack.tree[i]["is_integral"]))


def check_record(pack, i, item, n_pivots, digest, iterations, keys, result, where):
    """the comparison rule of tests/test_fuzz_services.py::replay"""
    trace = pack.pivot_trace(i)
    assert len(trace) == n_pivots, where
    assert pivot_digest(trace) == digest, where
    assert iterations is None or int(pack.tree[i]["iterations"]) == iterations, where
    res = result_of(pack, i, item)
    assert list(res.keys()) == keys, where
    for k, v in result.items():
        ref = v if isinstance(v, bool) else G.num(v)
        assert res[k] == ref or (isinstance(ref, float) and np.isnan(ref) and np.isnan(res[k])), (where, k)


def _cases(name):
    with gzip.open(os.path.join(G.GOLDEN, name), "rt") as fh:
        return [json.loads(line) for line in fh if line.startswith("{")]


def fuzz_default_cases():
    """the reference's recorded runs under the DEFAULT service that need no presolve pre-pass: every default-policy case of
    fuzz_services, and the fuzz_soft cases with integers, no soft constraints and no options"""
    out = []
    for c in _cases("fuzz_services.jsonl.gz"):
        if not c["model"].get("options") and c["fixed"] == 0 and not c["infeasPre"]:
            out.append(c)
    n_services = len(out)
    for c in _cases("fuzz_soft.jsonl.gz"):
        if c["model"].get("options") or c["fixed"] != 0 or c["infeasPre"]:
            continue
        m = Model(c["model"], None)
        _, oo = m.optional_objectives()
        if len(m.integerVariables) > 0 and (oo is None or len(oo) == 0) and _tree_in_scope(m):
            out.append(c)
    return out, n_services


def fixture(name):
    return G.load(os.path.join(G.GOLDEN, "fixtures", name + ".json.gz"))

