"""The pack kernels' simplex -- k_simplex_packed's loop and its second copy pk_simplex, which k_tree_packed runs per node
(jslpsolver_amd/csrc/jslp_packed.hip.h) -- at the selection, history, gate and capacity edges of tests/pack_edges.py, in all fourteen
builds: k_simplex_packed<64 | 256> plain and OPT, k_tree_packed<64 | 256> plain, OPT, MIR, ENH and INC.

The yardstick is the CPU oracle: one engine per LP for the LP packs, the Python host tree on the oracle for the tree packs; never a pack
against a pack.  Everything is compared as bytes -- result struct, evaluation, RHS column, row map, pivot trace, download(), the tree /
MIR / enhanced / incremental records, the optional rows -- with NaN canonical (the GPU and x86 make different NaN bits) and -0.0 exact.
All cases of one kind stand in ONE pack: a test is two launches of tiny workgroups, and asserts the exact JSLP_DEBUG_LAUNCH lines.
tests/test_pack_edges.py shows on the CPU that every instance is what its name says."""
import hashlib
import re

import numpy as np
import pytest

import pack_edges as PE
from jslpsolver_amd import _capi
from jslpsolver_amd.engine import TableauPack

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[jslp\] launch (k_simplex_packed|k_tree_packed)<(\d+)(?:,(\w+) 1)?> n (\d+) lds (\d+)")


def _lines(capfd):
    found = LAUNCH.findall(capfd.readouterr().err)
    assert all(0 < int(b) <= PE.LDS_LIMIT for _, _, _, _, b in found), found
    return [(k, int(t), kind or "plain", int(n)) for k, t, kind, n, _ in found]


def _want_lines(kernel, kind, threads):
    """one launch per thread count, the one-wave build first, each with exactly its LPs"""
    return [(kernel, t, kind, threads.count(t)) for t in (64, 256) if threads.count(t)]


# ---- LP packs: k_simplex_packed<64>, <256>, <64,opt 1>, <256,opt 1> -------------------------------------------------------------------
@pytest.mark.parametrize("opt", [False, True], ids=["plain", "opt"])
def test_lp_pack_equals_oracle_engines(hip_lib, oracle_lib, monkeypatch, capfd, opt):
    """every case in one pack; in the OPT builds a case without optional rows of its own gets one all-zero row (the oracle engine too)"""
    cases = [c for c in PE.lp_cases(oracle_lib) if opt or c.optional is None]
    rows = [c.with_zero_row() if opt else None for c in cases]
    for c, oo in zip(cases, rows):
        h, w = c.lp[0].shape
        lds = hip_lib.jslps_lds_bytes(h, w, len(oo)) if opt else hip_lib.jslpp_lds_bytes(h, w)
        assert 0 < lds <= PE.LDS_LIMIT, c.name
    want = [PE.engine_state(oracle_lib, c.lp, c.precision, c.check, oo) for c, oo in zip(cases, rows)]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = TableauPack([c.lp for c in cases], precision=[c.precision for c in cases], lib=hip_lib, trace_cap=512,
                       optional_objectives=rows if opt else None)
    try:
        pack.simplex(check_cycles=[c.check for c in cases])
        lines = _lines(capfd)
        assert lines == _want_lines("k_simplex_packed", "opt" if opt else "plain", [c.threads for c in cases]), lines
        assert {t for _, t, _, _ in lines} == {64, 256} and not pack.status.any()
        bad = []
        for i, c in enumerate(cases):
            got = PE.pack_lp_state(pack, i, opt)
            if got != want[i]:
                bad.append((c.name, PE.differing(got, want[i])))
        assert not bad, bad
    finally:
        pack.close()


# ---- tree packs: k_tree_packed<64 | 256> x plain, OPT, MIR, ENH, INC -------------------------------------------------------------------
@pytest.mark.parametrize("kind", PE.TREE_KINDS)
def test_tree_roots_equal_the_host_tree(hip_lib, oracle_lib, monkeypatch, capfd, kind):
    """every case as the root of a tree with one integer variable that is non-basic at the root's end: the tree is its root (the cycles
    included: a cycle at the root ends the tree)"""
    items = PE.tree_items(oracle_lib, kind)
    count = {"mir": hip_lib.jslpc_tree_lds_bytes, "inc": hip_lib.jslpi_tree_lds_bytes}.get(kind)
    for it in items:
        h, w = it.lp[0].shape
        lds = count(h, w, h + PE.TREE_ROWS) if count else hip_lib.jslps_tree_lds_bytes(h, w, h + PE.TREE_ROWS, it.n_optional)
        assert 0 < lds <= PE.LDS_LIMIT, it.case.name
    checks = [it.check for it in items]
    host = PE.tree_pack(oracle_lib, items, kind)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = PE.tree_pack(hip_lib, items, kind)
    try:
        host.branch_and_cut(check_cycles=checks)
        assert host.tree["iterations"].tolist() == [1] * len(items) and not host.status.any()
        pack.branch_and_cut(check_cycles=checks)
        lines = _lines(capfd)
        assert lines == _want_lines("k_tree_packed", kind, [it.case.tree_threads for it in items]), lines
        assert {t for _, t, _, _ in lines} == {64, 256} and not pack.status.any()
        bad = []
        for i, it in enumerate(items):
            got, want = PE.tree_state(pack, i), PE.tree_state(host, i)
            if got != want:
                bad.append((it.case.name, PE.differing(got, want)))
        assert not bad, bad
    finally:
        pack.close()
        host.close()


# ---- capacities ------------------------------------------------------------------------------------------------------------------------
def _neighbours():
    by_name = {c.name: c for c in PE.selection_cases()}
    return [by_name["ratio_tie@all-TALL64"], by_name["price_batch_in_thread-WIDE64"]]


@pytest.mark.parametrize("pad", [0, PE.CAP_PAD], ids=["one-wave", "four-waves"])
def test_history_capacity(hip_lib, oracle_lib, monkeypatch, capfd, pad):
    """Klee-Minty n = 12 with 0, 1, 2 fillers and the check ON: 4095 and 4096 pairs fit (JSLPP_HIST_CAP is no error, and the suffix test on
    the global copy has run four thousand times without a false hit); the 4097th ends the LP with the capacity code after exactly 4096
    pivots -- the oracle's first 4096, and what its own pivot() makes of them -- between two ordinary neighbours that are right"""
    nb = _neighbours()
    lps = [nb[0].lp] + [PE.capacity_lp(k, pad) for k in (0, 1, 2)] + [nb[1].lp]
    # (no cycle: the check-on state is the check-off one, tests/test_pack_edges.py::test_capacity_instances_have_no_cycle)
    want = [PE.engine_state(oracle_lib, lps[0])] + [PE.engine_state(oracle_lib, lp, check=False) for lp in lps[1:4]] + [PE.engine_state(oracle_lib, lps[4])]
    trace, arrays, n = PE.truncated_replay(oracle_lib, lps[3], PE.HIST_CAP)
    assert n == PE.HIST_CAP + 1
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = TableauPack(lps, precision=PE.PREC, lib=hip_lib, trace_cap=PE.HIST_CAP + 8)
    try:
        with pytest.raises(_capi.EngineError, match=r"\(-5\).*LP 3.*history"):
            pack.simplex(check_cycles=True)
        threads = [64, 256, 256, 256, 64] if pad else [64] * 5
        assert _lines(capfd) == _want_lines("k_simplex_packed", "plain", threads)
        assert pack.status.tolist() == [0, 0, 0, _capi.JSLP_ERR_CAPACITY, 0]
        for i in (0, 1, 2, 4):
            got = PE.pack_lp_state(pack, i, False)
            assert got == want[i], (i, PE.differing(got, want[i]))
        assert want[1]["res"]["pivots_phase2"] == 4095 and want[2]["res"]["pivots_phase2"] == PE.HIST_CAP and want[2]["res"]["optimal"]
        assert pack.pivot_trace(3).astype(np.int32).tobytes() == trace.tobytes() and len(trace) == PE.HIST_CAP
        assert [PE.canon(x) for x in pack.download(3)] == arrays
    finally:
        pack.close()


def test_trace_capacity(hip_lib, oracle_lib, monkeypatch, capfd):
    """the check OFF, 4097 pivots: trace_cap = 4097 brings all pairs back; trace_cap = 4096 makes jslpp_pack_pivot_trace refuse (the count
    is still returned) while the result, the RHS and download() are the oracle's, and the pair beyond the cap was not written: it would
    have landed in the slice of the next LP of d_trace, whose own trace is intact"""
    nb = _neighbours()
    lps = [nb[0].lp, PE.capacity_lp(2), nb[1].lp]
    want = [PE.engine_state(oracle_lib, lp, check=False) for lp in lps]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    for cap in (PE.HIST_CAP + 1, PE.HIST_CAP):
        capfd.readouterr()
        pack = TableauPack(lps, precision=PE.PREC, lib=hip_lib, trace_cap=cap, max_pivots=PE.HIST_CAP)
        try:
            # call 1 stops the long LP at 4096 pivots (max_pivots); both neighbours end and leave their pairs in their slices of d_trace: the
            # guard pattern.  Call 2 makes the long LP's 4097th pivot, the neighbours none
            with pytest.raises(_capi.EngineError, match=r"\(-5\).*LP 1.*iteration"):
                pack.simplex(check_cycles=False)
            assert pack.status.tolist() == [0, _capi.JSLP_ERR_CAPACITY, 0]
            for i in (0, 2):
                got = PE.pack_lp_state(pack, i, False)
                assert got == want[i], (i, PE.differing(got, want[i]))
            out = pack.simplex(check_cycles=False)
            assert not pack.status.any() and out[1]["optimal"] and (out[1]["pivots_phase1"], out[1]["pivots_phase2"]) == (0, 1)
            assert out["pivots_phase2"].tolist() == [0, 1, 0]
            rhs, rows = pack.read_rhs(1)
            assert PE.canon(rhs) == want[1]["rhs"] and PE.canon(rows) == want[1]["rows"] and PE.canon(np.float64(pack.evaluation[1])) == want[1]["evaluation"]
            assert [hashlib.sha256(PE.canon(x)).hexdigest() for x in pack.download(1)] == want[1]["arrays"]
            n = _capi.C.c_int64()
            buf = np.empty(2 * (PE.HIST_CAP + 1), dtype=np.int32)
            rc = hip_lib.jslpp_pack_pivot_trace(pack._h, 1, _capi.ptr_i32(buf), PE.HIST_CAP + 1, _capi.C.byref(n))
            assert n.value == PE.HIST_CAP + 1
            if cap == PE.HIST_CAP + 1:
                assert rc == _capi.JSLP_OK and buf.tobytes() == want[1]["trace"]
            else:  # ... and so does a read of the recorded prefix alone: it is not handed out as if it were complete
                assert rc == _capi.JSLP_ERR_CAPACITY
                rc = hip_lib.jslpp_pack_pivot_trace(pack._h, 1, _capi.ptr_i32(buf), PE.HIST_CAP, _capi.C.byref(n))
                assert rc == _capi.JSLP_ERR_CAPACITY and n.value == PE.HIST_CAP + 1 and b"LP 1" in hip_lib.jslp_last_error()
            assert _lines(capfd) == 2 * _want_lines("k_simplex_packed", "plain", [64, 64, 64])  # (two calls)
            for i in (0, 2):  # the neighbours' own traces, pairs of call 1 that nothing has touched since
                assert pack.pivot_trace(i).astype(np.int32).tobytes() == want[i]["trace"] and len(want[i]["trace"]) > 0, i
        finally:
            pack.close()


@pytest.mark.parametrize("cap", [1, 2])
def test_pivot_cap_equals_the_truncated_replay(hip_lib, oracle_lib, monkeypatch, capfd, cap):
    """max_pivots of 1 and 2, a gate case and a phase-1 LP in both thread counts: the LP ends with the capacity code after exactly that
    many pivots, its tableau what the oracle's pivot() makes of the first entries of the oracle's trace"""
    cases = PE.pivot_cap_cases()
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = TableauPack([c.lp for c in cases], precision=PE.PREC, lib=hip_lib, trace_cap=16, max_pivots=cap)
    try:
        with pytest.raises(_capi.EngineError, match=r"\(-5\).*LP 0.*iteration"):
            pack.simplex(check_cycles=False)
        assert _lines(capfd) == _want_lines("k_simplex_packed", "plain", [c.threads for c in cases])
        assert sorted(c.threads for c in cases) == [64, 64, 256, 256]
        assert pack.status.tolist() == [_capi.JSLP_ERR_CAPACITY] * len(cases)
        for i, c in enumerate(cases):
            trace, arrays, n = PE.truncated_replay(oracle_lib, c.lp, cap)
            assert n > cap and pack.pivot_trace(i).astype(np.int32).tobytes() == trace.tobytes(), c.name
            assert [PE.canon(x) for x in pack.download(i)] == arrays, c.name
    finally:
        pack.close()


@pytest.mark.parametrize("kind", PE.TREE_KINDS)
def test_history_capacity_at_a_tree_root(hip_lib, oracle_lib, monkeypatch, capfd, kind):
    """the 4097-pivot LP as the root of a tree of every build, one wave and four: its tree's status is the capacity code, the neighbours'
    trees equal the host's"""
    by_name = {c.name: c for c in PE.selection_cases()}
    nb = [by_name["ratio_tie@all-TALL64"], by_name["ratio_tie@all-TALL256"]]
    long_cases = [PE.Case("km12_k2", None, PE.capacity_lp(2), None), PE.Case("km12_k2_padded", None, PE.capacity_lp(2, PE.CAP_PAD), None)]
    nb_items = PE.tree_items(oracle_lib, kind, nb)
    # (the integer variable: any structural one -- the tree never gets past the root's simplex)
    items = [nb_items[0], PE.TreeItem(long_cases[0], 0, kind), PE.TreeItem(long_cases[1], 0, kind), nb_items[1]]
    host = PE.tree_pack(oracle_lib, nb_items, kind)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = PE.tree_pack(hip_lib, items, kind)
    try:
        host.branch_and_cut(check_cycles=True)
        with pytest.raises(_capi.EngineError, match=r"\(-5\).*LP 1"):
            pack.branch_and_cut(check_cycles=True)
        assert _lines(capfd) == _want_lines("k_tree_packed", kind, [64, 64, 256, 256])
        assert pack.status.tolist() == [0, _capi.JSLP_ERR_CAPACITY, _capi.JSLP_ERR_CAPACITY, 0]
        for i, j in ((0, 0), (3, 1)):
            got, want = PE.tree_state(pack, i), PE.tree_state(host, j)
            assert got == want, (i, PE.differing(got, want))
    finally:
        pack.close()
        host.close()
