"""jslpp_pack_* on the MI355X: many small LPs in one object, each solved by one workgroup with its whole tableau in LDS (k_simplex_packed).

The yardsticks are the reference's goldens and the CPU oracle; a twin `Tableau.simplex()` on the HIP engine is a further check.  The pack is
never compared with itself.  The JSLP_DEBUG_LAUNCH lines say how many launches ran, with which build and how many LPs each."""
import gzip
import json
import os
import re

import numpy as np
import pytest

import golden_util as G
from jslpsolver_amd import _capi, generators
from jslpsolver_amd.engine import Tableau, TableauPack, simplex_many
from jslpsolver_amd.model import Model
from test_cycle_goldens import SMALL as CYCLE_GOLDENS, _instance, _messages
from test_many_gpu import _check_golden

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[jslp\] launch k_simplex_packed<(\d+)> n (\d+) lds (\d+)")
LDS_LIMIT = 65536
ROUTING_CELLS = 2048  # PACK_CELLS_WAVE (jslp_hip.hip): at most this many cells -> the one-wave build


class _Lp:
    """LP i of a solved pack behind the read-back surface of a Tableau (what test_many_gpu._check_golden reads)"""

    def __init__(self, pack, i):
        self.pack, self.i = pack, i
        self.evaluation = float(pack.evaluation[i])

    def read_rhs(self):
        return self.pack.read_rhs(self.i)

    def pivot_trace(self):
        return self.pack.pivot_trace(self.i)

    def download(self):
        return self.pack.download(self.i)


def _state_of(res, evaluation, rhs_rows, trace, download):
    """everything a solve leaves, as bytes (NaN compares equal to itself)"""
    fm, vibr, vibc, rbv, cbv = download
    return dict(res=bytes(res), evaluation=np.float64(evaluation).tobytes(), rhs=rhs_rows[0].tobytes(), rows=rhs_rows[1].tobytes(),
                trace=trace.tobytes(), matrix=fm.tobytes(), vibr=vibr.tobytes(), vibc=vibc.tobytes(), rbv=rbv.tobytes(), cbv=cbv.tobytes())


def _pack_state(pack, i):
    return _state_of(pack.result(i), pack.evaluation[i], pack.read_rhs(i), pack.pivot_trace(i), pack.download(i))


def _engine_state(lib, lp, precision, check, calls=1):
    """the same LP through jslp_engine_simplex on a fresh engine of `lib` (row_capacity = height)"""
    t = Tableau(*lp, precision=precision, lib=lib)
    for _ in range(calls):
        res = t.simplex(check_cycles=check)
    st = _state_of(res, t.evaluation, t.read_rhs(), t.pivot_trace(), t.download())
    t.close()
    return st


def _golden_lp(g):
    tab = g["tableau"]
    m, vibr, vibc = G.dense_tableau(tab)
    return (m, vibr, vibc, tab["unrestricted"]), tab["precision"], bool(tab["checkForCycles"])


def _fixtures():
    return {G.ident(p): g for p, g in ((p, G.load(p)) for p in G.fixture_paths()) if g["tableau"] is not None}


def _launches(capfd):
    return [(int(t), int(n), int(b)) for t, n, b in LAUNCH.findall(capfd.readouterr().err)]


def _solve_and_compare(hip_lib, oracle_lib, items, trace_cap=4096):
    """items: (lp, precision, check).  One pack, one call; every LP against the oracle engine"""
    pack = TableauPack([lp for lp, _, _ in items], precision=[p for _, p, _ in items], lib=hip_lib, trace_cap=trace_cap)
    pack.simplex(check_cycles=[c for _, _, c in items])
    for i, (lp, p, c) in enumerate(items):
        assert _pack_state(pack, i) == _engine_state(oracle_lib, lp, p, c), "LP %d (%d x %d) differs from the oracle" % ((i,) + lp[0].shape)
    return pack


def test_goldens_in_one_pack(hip_lib, oracle_lib, monkeypatch, capfd):
    fx = _fixtures()
    plain = [n for n, g in fx.items() if not g["tableau"]["optionalObjectives"]]
    names = [n for n in plain if hip_lib.jslpp_lds_bytes(fx[n]["tableau"]["height"], fx[n]["tableau"]["width"]) <= LDS_LIMIT]
    assert sorted(set(plain) - set(names)) == ["Monster_II", "Monster_Problem", "Sudoku4x4", "Vendor_Selection"]
    assert "LargeFarmMIP" in names and len(names) >= 35
    items = [_golden_lp(fx[n]) for n in names]
    cyc = [_instance(p) for p in CYCLE_GOLDENS]
    assert len(cyc) == 13
    for g, m, vibr, vibc in cyc:
        items.append(((m, vibr, vibc, g["tableau"]["unrestricted"]), g["tableau"]["precision"], bool(g["tableau"]["checkForCycles"])))
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = TableauPack([lp for lp, _, _ in items], precision=[p for _, p, _ in items], lib=hip_lib, trace_cap=4096)
    pack.simplex(check_cycles=[c for _, _, c in items])
    lines = _launches(capfd)
    assert sorted(t for t, _, _ in lines) == [64, 256] and sum(n for _, n, _ in lines) == len(items) == len(pack), lines
    assert all(b <= LDS_LIMIT for _, _, b in lines) and pack.launches == 2
    for i, n in enumerate(names):
        _check_golden(_Lp(pack, i), pack.result(i), fx[n])
    for k, (g, m, vibr, vibc) in enumerate(cyc):
        i = len(names) + k
        res = pack.result(i)
        assert g["tableau"]["checkForCycles"] and _messages(res) == g["messages"], G.ident(CYCLE_GOLDENS[k])
        _check_golden(_Lp(pack, i), res, g)
    for i, (lp, p, c) in enumerate(items):  # a twin engine on the GPU that never saw a pack
        assert _pack_state(pack, i) == _engine_state(hip_lib, lp, p, c), i
    pack.close()


def test_fuzz_roots_in_one_call(hip_lib, oracle_lib):
    items = []
    for name in ("fuzz_services.jsonl.gz", "fuzz_soft.jsonl.gz"):
        with gzip.open(os.path.join(G.GOLDEN, name), "rt") as fh:
            for line in fh:
                m = Model(json.loads(line)["model"], None)
                _, oo = m.optional_objectives()
                if oo is None or len(oo) == 0:
                    matrix, vibr, vibc = m.build_tableau()
                    items.append(((matrix, vibr, vibc, list(m.unrestricted)), m.precision, bool(m.checkForCycles)))
    assert len(items) == 720
    assert max(lp[0].size for lp, _, _ in items) == 1260
    _solve_and_compare(hip_lib, oracle_lib, items).close()


def _dense(h, w, seed=4242):
    m, vibr, vibc = generators.dense_resource_allocation_tableau(seed + 131 * h + w, w - 1, h - 1)
    assert m.shape == (h, w)
    return (m, vibr, vibc, []), 1e-8, True


def test_lane_and_thread_edges(hip_lib, oracle_lib, monkeypatch, capfd):
    """one wave plus and minus one in both directions, one 256-thread block plus one, both sides of the routing constant"""
    sizes = (2, 3, 63, 64, 65, 66)
    shapes = [(h, w) for h in sizes for w in sizes] + [(257, 20), (20, 257)]
    shapes += [(32, 64), (32, 65), (2, 1024), (2, 1025)]  # 2048 / 2080 / 2048 / 2050 cells
    assert all(hip_lib.jslpp_lds_bytes(h, w) <= LDS_LIMIT for h, w in shapes)
    items = [_dense(h, w) for h, w in shapes]
    taco = G.load(os.path.join(G.GOLDEN, "fixtures", "TacoParty.json.gz"))
    assert (taco["tableau"]["height"], taco["tableau"]["width"]) == (2, 5)  # a single constraint row
    items.append(_golden_lp(taco))
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = _solve_and_compare(hip_lib, oracle_lib, items)
    lines = _launches(capfd)
    n_wave = sum(h * w <= ROUTING_CELLS for h, w in shapes) + 1
    assert sorted((t, n) for t, n, _ in lines) == [(64, n_wave), (256, len(items) - n_wave)], lines
    assert any(pack.pivot_trace(i).size > 0 for i in range(len(items)))
    _check_golden(_Lp(pack, len(items) - 1), pack.result(len(items) - 1), taco)
    pack.close()


def test_lds_limit(hip_lib, oracle_lib):
    n = 2
    while hip_lib.jslpp_lds_bytes(n + 1, n + 1) <= LDS_LIMIT:
        n += 1
    assert hip_lib.jslpp_lds_bytes(n, n) <= LDS_LIMIT < hip_lib.jslpp_lds_bytes(n + 1, n + 1) and n > 64
    big = _dense(n, n)
    _solve_and_compare(hip_lib, oracle_lib, [big]).close()
    over = _dense(n + 1, n + 1)
    with pytest.raises(_capi.EngineError, match=r"\(-6\).*LP 1"):
        TableauPack([big[0], over[0]], lib=hip_lib)
    _solve_and_compare(hip_lib, oracle_lib, [big, _dense(5, 7)]).close()  # a pack made after the refusal works


# Residency of k_simplex_packed<64> (profiles/packed_lp_kernel_resources.md): 65 VGPRs -> allocated as 72 -> 7 waves per SIMD; a workgroup
# is one wave, so 28 workgroups per CU (a tiny LP's LDS, 1.6 KB static + 1-3 KB dynamic, does not bind: 160 KB per CU) -> 7168 on the 256
# CUs.  20480 LPs are more than twice what the chip holds at once.
OVERSUBSCRIBED = 20480


def test_oversubscribed_pack(hip_lib, monkeypatch, capfd):
    fx = _fixtures()
    names = ["Berlin_Air_Lift_Problem", "Chocolate_Problem", "Coffe_Problem", "Computer_Problem", "Wiki_1", "Degenerate_Max",
             "Infeasible_1", "Unrestricted", "Cycling_Fletcher", "Shift_Work_Problem"]
    assert all(n in fx and not fx[n]["tableau"]["optionalObjectives"] for n in names)
    lps = [_golden_lp(fx[n]) for n in names]
    assert all(lp[0].size <= ROUTING_CELLS for lp, _, _ in lps)
    twins = [_engine_state(hip_lib, lp, p, True) for lp, p, _ in lps]
    k = len(names)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = TableauPack([lps[i % k][0] for i in range(OVERSUBSCRIBED)], precision=[lps[i % k][1] for i in range(OVERSUBSCRIBED)],
                       lib=hip_lib, trace_cap=64)
    out = pack.simplex(check_cycles=True)
    lines = _launches(capfd)
    assert len(lines) == 1 and lines[0][:2] == (64, OVERSUBSCRIBED), lines
    assert not pack.status.any()
    for j in range(k):  # the result structs of a fixture's copies, all at once
        assert (out[j::k].tobytes() == bytes(pack.result(j)) * len(out[j::k])) and bytes(pack.result(j)) == twins[j]["res"], names[j]
    for i in range(OVERSUBSCRIBED):
        assert _pack_state(pack, i) == twins[i % k], i
    pack.close()


def test_per_lp_status(hip_lib):
    """a cycling LP with the check off runs into its pivot cap between two LPs that solve: its status says so, the call returns the code
    naming the LP, its result is left as it was, and both neighbours are right"""
    fx = _fixtures()
    berlin, pb, _ = _golden_lp(fx["Berlin_Air_Lift_Problem"])
    g, m, vibr, vibc = _instance(os.path.join(G.GOLDEN, "cycles", "deg_178868.json.gz"))  # (cycles for ever without the check)
    pack = TableauPack([berlin, (m, vibr, vibc, g["tableau"]["unrestricted"]), berlin], precision=[pb, g["tableau"]["precision"], pb],
                       lib=hip_lib, trace_cap=4096, max_pivots=200)
    out = np.zeros(3, dtype=_capi.RESULT_DTYPE)
    out["pivots_phase1"] = 777  # sentinel
    out["evaluation"] = -12.5
    before = out[1].tobytes()
    status = np.full(3, 7, dtype=np.int32)
    cc = np.array([1, 0, 1], dtype=np.int32)
    rc = hip_lib.jslpp_pack_simplex(pack._h, _capi.ptr_i32(cc), out.ctypes.data, _capi.ptr_i32(status), None)
    assert rc == _capi.JSLP_ERR_CAPACITY
    assert status.tolist() == [_capi.JSLP_OK, _capi.JSLP_ERR_CAPACITY, _capi.JSLP_OK]
    assert b"LP 1" in hip_lib.jslp_last_error() and b"iteration" in hip_lib.jslp_last_error()
    assert out[1].tobytes() == before
    n = _capi.C.c_int64()
    hip_lib.check(hip_lib.jslpp_pack_pivot_trace(pack._h, 1, None, 0, _capi.C.byref(n)), "jslpp_pack_pivot_trace")
    assert n.value == 200  # the cap, to the pivot
    for i in (0, 2):
        pack.results[i] = out[i]
        pack.evaluation[i] = out[i]["evaluation"]
        _check_golden(_Lp(pack, i), pack.result(i), fx["Berlin_Air_Lift_Problem"])
    pack.upload()
    with pytest.raises(_capi.EngineError, match="LP 1"):  # the Python layer: the same call raises, the neighbours' scalars are folded
        pack.simplex(check_cycles=[True, False, True])
    assert pack.status.tolist() == [0, _capi.JSLP_ERR_CAPACITY, 0] and pack.evaluation[0] == out[0]["evaluation"]
    pack.close()


def test_nonfinite_values(hip_lib, oracle_lib):
    gold = G.load(os.path.join(G.GOLDEN, "nonfinite.json.gz"))
    names = [n for n in sorted(gold) if not gold[n]["tableau"]["integerVarIndexes"]]
    assert len(names) == 4
    items = [_golden_lp(gold[n]) for n in names]
    assert all(hip_lib.jslpp_lds_bytes(*lp[0].shape) <= LDS_LIMIT for lp, _, _ in items)
    pack = _solve_and_compare(hip_lib, oracle_lib, items)
    for i, n in enumerate(names):
        _check_golden(_Lp(pack, i), pack.result(i), gold[n])
    pack.close()


def test_reuse_and_isolation(hip_lib, oracle_lib):
    fx = _fixtures()
    names = ["Berlin_Air_Lift_Problem", "Wiki_1", "Unrestricted", "Infeasible_1", "LargeFarmMIP", "Shift_Work_Problem"]
    items = [_golden_lp(fx[n]) for n in names]
    pack = _solve_and_compare(hip_lib, oracle_lib, items)
    first = [_pack_state(pack, i) for i in range(len(items))]
    # ordinary engines between two pack calls: a single simplex() and a simplex_many batch, each with its usual state
    lone = Tableau(*items[1][0], precision=items[1][1], lib=hip_lib)
    res = lone.simplex(check_cycles=items[1][2])
    assert _state_of(res, lone.evaluation, lone.read_rhs(), lone.pivot_trace(), lone.download()) == _engine_state(oracle_lib, *items[1])
    many = [Tableau(*lp, precision=p, lib=hip_lib) for lp, p, _ in items[:3]]
    rs = simplex_many(many, check_cycles=[c for _, _, c in items[:3]])
    for t, r, it in zip(many, rs, items[:3]):
        assert _state_of(r, t.evaluation, t.read_rhs(), t.pivot_trace(), t.download()) == _engine_state(oracle_lib, *it)
    # a second simplex() without an upload continues from the final tableaus: the engine called twice
    pack.simplex(check_cycles=[c for _, _, c in items])
    for i, (lp, p, c) in enumerate(items):
        assert _pack_state(pack, i) == _engine_state(oracle_lib, lp, p, c, calls=2), names[i]
    # a re-upload followed by a solve equals the first solve
    pack.upload()
    pack.simplex(check_cycles=[c for _, _, c in items])
    assert [_pack_state(pack, i) for i in range(len(items))] == first
    for t in many + [lone]:
        t.close()
    pack.close()
    _solve_and_compare(hip_lib, oracle_lib, items[:2]).close()  # close() followed by a new pack works
    hip_lib.jslp_release_pooled_resources()
    _solve_and_compare(hip_lib, oracle_lib, items[2:4]).close()
