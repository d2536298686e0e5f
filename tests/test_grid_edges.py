"""Every register-resident instance of the product library at the edges of its grid and lanes, and the streaming kernels at their
tile edges, HIP against the CPU oracle bit for bit.

The suite's goldens land the 28 instances of `k_simplex_resident` in jslp_resident_table.hip.h on a few grid sizes (mostly G = 251); the
full grid (G = 256) is where ONE wave gathers all four looks per lane of the ratio-test summaries and where a cooperative launch
needs every CU.  Each case here names the geometry its shape must take, and the test reads WHICH instance ran from the engine's
`JSLP_DEBUG_LAUNCH` line (one per accepted launch: key, G, rows per workgroup; or the streaming kernels' choice), so a policy change
that sends a tableau elsewhere fails instead of passing on another kernel.

Instances: the dense all-"<=" integer LP of tools/resident_stress.py, planted so that the edges pivot --
  * the cost row is zero except 64 columns (a few hundred pivots) and column W-1;
  * row 1 (workgroup 0) is the bound 2 x_c0 <= 2 and row H-1 (the LAST workgroup) x_c0 + x_{W-1} <= 1, c0 = the first entering
    column: the first phase-2 ratio test is an exact tie between the first and the last workgroup (row 1 wins: lowest row);
  * that pivot leaves row H-1 degenerate, and column W-1 is zero in every other row: once W-1 enters, row H-1 leaves.
The CPU part proves on the oracle that every instance does pivot in the last workgroup, in column W-1 and through the tie; it also
restates the launch policy (resident_geometry / fused_eligible, jslp_hip.hip) and checks every case against the geometry it names,
and checks that the case table reaches every product instance at G = 256.
Oracle answers: one run per instance (cycle check on -- with no cycle found the trace is the check-off run's too), computed side by
side on a few threads the first time any test needs one; the final tableau is compared through its sha256."""
import hashlib
import os
import re
import sys
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np
import pytest

from jslpsolver_amd.engine import Tableau
from test_edge_cases import _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resident_stress import int_instance  # noqa: E402  (the instance builder of the stress tool and its known answers)

TU_RESIDENT = os.path.join(ROOT, "jslpsolver_amd", "csrc", "jslp_resident_table.hip.h")  # the instance table the parts of jslp_tu_resident.hip compile
SEED = 12345
PREC = 1e-8
MAXG = 256  # JSLP_F_MAXG
TW = 2048  # JSLP_F_TW: columns per tile of the streaming kernels
GEOM = {"g1": (1024, 2, 8), "g2": (512, 4, 8), "g3": (512, 4, 16), "g4": (512, 6, 12), "g5": (512, 8, 8)}
LD_MAX = {"g1": 2048, "g2": 2048, "g3": 2048, "g4": 3072, "g5": 4096}
GEOM_ENV = {"g2": {"JSLP_RES_CPT": "4"}}
KNOBS = ("JSLP_FORCE_PATH", "JSLP_RES_CPT", "JSLP_RES_LEAN", "JSLP_RES_GEOM", "JSLP_RES_RPB", "JSLP_RES_WIDE_TALL", "JSLP_XL",
         "JSLP_NO_WGLDS", "JSLP_INJECT_RESIDENT_ABORT_US")


def _ld(W):
    return (W + 15) // 16 * 16


def _rpb(H):
    return (H + MAXG - 1) // MAXG


def _grid(H):
    return (H + _rpb(H) - 1) // _rpb(H)


# ---- instances ---------------------------------------------------------------------------------------------------------------
Inst = namedtuple("Inst", "H W n_unr n_opt two_phase cap")  # (cap: row capacity -- the index maps are sized by it)


def _batch(W):
    """partial pricing's batch of columns (simplex.ts:118-127), or 0: full pricing"""
    batch = min(max(int(np.floor(np.sqrt(W - 1))), 50), 500)
    return batch if W - 1 > 2 * batch else 0


def _first_column(cost, W):
    """the first entering column of phase 2 (simplex.ts:136-219 restated: partial pricing from the first batch, first maximum)"""
    batch = _batch(W)
    if batch:
        for bs in range(1, W, batch):
            seg = cost[bs:min(bs + batch, W)]
            if (seg > PREC).any():
                return bs + int(np.argmax(seg))
    return 1 + int(np.argmax(cost[1:]))


@lru_cache(maxsize=2)
def planted(inst):
    """-> (A, vibr, vibc, unrestricted, optional objectives or None, c0); see the module docstring"""
    H, W = inst.H, inst.W
    A, vibr, vibc = int_instance(H - 1, W - 1, SEED, inst.two_phase)
    rng = np.random.default_rng(SEED + H * 7 + W)
    ge_cols = set()
    if inst.two_phase:  # the ">=" rows (negative RHS, one -1 each) keep clear of the planted rows and of column W-1
        free = [r for r in range(2, H - 1) if A[r, 0] >= 0]
        for r in (1, H - 1):
            if A[r, 0] < 0:
                s = free.pop()
                A[[r, s]] = A[[s, r]]
        ge_cols = {int(c) + 1 for r in range(1, H) if A[r, 0] < 0 for c in np.nonzero(A[r, 1:])[0]}
        if W - 1 in ge_cols:
            s = next(c for c in range(W - 2, 0, -1) if c not in ge_cols)
            A[:, [W - 1, s]] = A[:, [s, W - 1]]
            ge_cols = (ge_cols - {W - 1}) | {s}
    if inst.n_unr:  # the first n_unr variables are unrestricted: negative coefficients in half the rows bound them both ways
        A[2:H - 1, 1:1 + inst.n_unr] *= np.where(rng.random((H - 3, inst.n_unr)) < 0.5, -1.0, 1.0)
    pool = np.array([c for c in range(1 + inst.n_unr, W - 1) if c not in ge_cols])
    attractive = rng.choice(pool, min(63, len(pool)), replace=False)
    A[0, 1:] = 0.0
    A[0, attractive] = rng.integers(1, 51, len(attractive))
    A[0, W - 1] = rng.integers(1, 51) if _batch(W) else 1.0  # (under full pricing the smallest cost: never the first column)
    c0 = _first_column(A[0], W)
    assert c0 != W - 1 and c0 not in ge_cols and c0 > inst.n_unr
    A[1:, W - 1] = 0.0
    A[1, :] = 0.0
    A[1, 0] = A[1, c0] = 2.0
    A[H - 1, :] = 0.0
    A[H - 1, 0] = A[H - 1, c0] = A[H - 1, W - 1] = 1.0
    oo = None
    if inst.n_opt:  # optional objectives: a few attractive columns each (priced where the main cost row is ~0)
        oo = np.zeros((inst.n_opt, W))
        for o in range(inst.n_opt):
            cols = rng.choice(np.arange(1, W), 16, replace=False)
            oo[o, cols] = rng.integers(1, 51, 16)
    return A, vibr, vibc, list(range(inst.n_unr)), oo, c0


def _answer(t, res):
    """what tests/test_edge_cases.py:_run returns, with the downloaded arrays as sha256 (tens of MB each here)"""
    return (res.as_dict(), t.pivot_trace().tolist(), [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in t.download()],
            repr(t.evaluation))


def _tie_rows(M, col):
    """rows at the minimum quotient of the ratio test (simplex.ts:271-296) on column `col` of tableau M"""
    a, b = M[1:, col], M[1:, 0]
    live = np.abs(a) >= PREC
    assert not (live & (a > 0) & (np.abs(b) < PREC)).any(), "a degenerate row would decide this ratio test"
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(live, b / a, np.inf)
    q = np.where(q > PREC, q, np.inf)
    return set((np.nonzero(q == q.min())[0] + 1).tolist())


def _oracle_one(lib, inst):
    A, vibr, vibc, unr, oo, c0 = planted(inst)
    t = Tableau(A, vibr, vibc, unr, lib=lib, optional_objectives=oo, row_capacity=inst.cap)
    res = t.simplex(check_cycles=True)
    ans = _answer(t, res)
    t.close()
    p1 = res.pivots_phase1
    M = A
    if p1 > 0:  # the tableau at the first phase-2 pivot: phase 1 replayed pivot by pivot
        r = Tableau(A, vibr, vibc, unr, lib=lib, optional_objectives=oo)
        for row, col in ans[1][:p1]:
            r.pivot(row, col)
        M = r.download()[0]
        r.close()
    return {"answer": ans, "c0": c0, "p1": p1, "tie": _tie_rows(M, c0)}


_ORACLE = {}


def _oracle(lib, inst):
    """the oracle's answer for `inst`; the first call computes every instance of the module side by side"""
    if inst not in _ORACLE:
        todo = sorted({c.inst for c in CASES} - set(_ORACLE), key=lambda i: -i.H * i.W)
        workers = max(1, min(8, len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "8") or 8)))
        with ThreadPoolExecutor(workers) as ex:  # (the oracle's calls release the GIL; it keeps no shared state)
            for i, out in zip(todo, ex.map(lambda i: _oracle_one(lib, i), todo)):
                _ORACLE[i] = out
    return _ORACLE[inst]


# ---- the case table ----------------------------------------------------------------------------------------------------------
# geom: the geometry the shape must take (g1..g5), or the streaming kernels ("fused": k_fused_p1 + k_pivot_fused, "select+update")
Case = namedtuple("Case", "id inst geom chk env G")

# per geometry: full grid with every row of the last workgroup live, full grid with ONE row in it (the geometry's widest ld first)
FULL = {"g1": [(2048, 2048), (2041, 2033)], "g2": [(2048, 2048), (2041, 2033)], "g3": [(4096, 2048), (4081, 2000)],
        "g4": [(3072, 3072), (3061, 3000)], "g5": [(2048, 4096), (2041, 3500)]}


def _case(id, H, W, geom, n_unr=0, n_opt=0, two_phase=False, chk=False, cap=None, env=None, G=None):
    return Case(id, Inst(H, W, n_unr, n_opt, two_phase, cap), geom, chk, dict(env or {}), G)


def _cases():
    out = []
    for g, shapes in FULL.items():
        env = GEOM_ENV.get(g, {})
        for H, W in shapes:
            for unr in (0, 3):
                for chk in (False, True):
                    out.append(_case("%s-%dx%d-lean-unr%d-chk%d" % (g, H, W, unr, chk), H, W, g, n_unr=unr, chk=chk, env=env, G=256))
            out.append(_case("%s-%dx%d-spare-rows" % (g, H, W), H, W, g, cap=H + 8, env=env, G=256))  # (B&B: cap_rows > H)
        H, W = shapes[0]
        out.append(_case("%s-%dx%d-phase1" % (g, H, W), H, W, g, two_phase=True, env=env, G=256))
        if g in ("g1", "g2"):  # the general build (its instances: CHK = true)
            for unr in (0, 3):
                out.append(_case("%s-%dx%d-general-unr%d" % (g, H, W, unr), H, W, g, n_unr=unr, chk=True, env=dict(env, JSLP_RES_LEAN="0"), G=256))
        if g in ("g1", "g3"):  # the OPT builds
            for n_opt in (1, 3):
                for chk in (False, True):
                    out.append(_case("%s-%dx%d-opt%d-chk%d" % (g, H, W, n_opt, chk), H, W, g, n_opt=n_opt, chk=chk, env=env, G=256))
    # the summary gather's looks (lane + 64 q < G) and one past the one-row-per-workgroup grid: forced resident at small heights
    for g in ("g1", "g2"):
        for H in (64, 65, 128, 129, 192, 193, 256, 257):
            out.append(_case("%s-%dx2048-forced" % (g, H), H, 2048, g, env=dict(GEOM_ENV.get(g, {}), JSLP_FORCE_PATH="resident"), G=_grid(H)))
    out.append(_case("g3-2049x2048-rpb9", 2049, 2048, "g3", G=228))  # (also: one row past the headline geometry)
    out.append(_case("g4-2048x2049-ld2064", 2048, 2049, "g4", G=256))  # the narrowest ld of the 6- and 8-column geometries
    out.append(_case("g5-2048x3073-ld3088", 2048, 3073, "g5", G=256))
    # one past each geometry's last grid / lane: the next geometry or the streaming kernels
    out.append(_case("past-g3-4097x2048", 4097, 2048, "fused"))
    out.append(_case("past-g4-3073x3072", 3073, 3072, "fused"))
    out.append(_case("past-g5-2048x4097", 2048, 4097, "fused"))
    # the streaming kernels at their tile edges (ld = 2048 k, 2048 k + 16), phase 2 only and with a phase 1
    fused = {"JSLP_FORCE_PATH": "fused"}
    for W in (2048, 2049, 4096, 4097, 6144, 6145, 8192, 8193):
        for tp in (False, True):
            out.append(_case("fused-40x%d-%s" % (W, "phase1" if tp else "phase2"), 40, W, "fused" if _ld(W) <= 4 * TW else "select+update",
                             two_phase=tp, env=fused))
    out.append(_case("fused-40x4096-unr3", 40, 4096, "fused", n_unr=3, env=fused))  # unrestricted variables: two tiles at most
    out.append(_case("fused-40x4097-unr3", 40, 4097, "select+update", n_unr=3, env=fused))
    out.append(_case("fused-16384x40", 16384, 40, "fused", env=fused))  # cap_rows <= 64 row groups x 256 workgroups
    out.append(_case("fused-16385x40", 16385, 40, "select+update", env=fused))
    out.append(_case("fused-3328x40", 3328, 40, "fused", env=fused))  # 13 rows per workgroup: not a multiple of the row group (8)
    return out


CASES = _cases()
RESIDENT = [c for c in CASES if c.geom in GEOM]
INSTANCES = sorted({c.inst for c in CASES}, key=lambda i: i._replace(cap=i.cap or 0))


# ---- what the table expects --------------------------------------------------------------------------------------------------
def _lean(case):
    return case.env.get("JSLP_RES_LEAN") != "0"


def expected_key(case):
    """(T, C, R, unr, lean, opt, chk, xl) of the instance the case must run (the general build is compiled with CHK = true)"""
    lean = _lean(case)
    return GEOM[case.geom] + (int(case.inst.n_unr > 0), int(lean), int(case.inst.n_opt > 0), int(case.chk or not lean), 0)


def _resident_line(case):
    T, C, R, unr, lean, opt, chk, xl = expected_key(case)
    return "k_simplex_resident<%d,%d,%d> unr %d lean %d opt %d chk %d xl %d G %d rpb %d" % (T, C, R, unr, lean, opt, chk, xl, case.G, _rpb(case.inst.H))


def expected_lines(case):
    """the JSLP_DEBUG_LAUNCH lines of one simplex() (jslp_hip.hip run_simplex): the headline geometries run the whole solve register-resident;
    the tall / wide ones run phase 1 through k_fused_p1 first; the streaming kernels k_fused_p1 + k_pivot_fused, or select + update"""
    i = case.inst
    if case.geom in ("g1", "g2"):
        return [_resident_line(case)]
    if case.geom == "select+update":
        return ["select+update"]
    nt = (_ld(i.W) + TW - 1) // TW
    unr, opt = int(i.n_unr > 0 and nt <= 2), int(i.n_opt > 0 and nt <= 2)
    p1 = "k_fused_p1<%d,%d>" % (nt, unr)
    return [p1, _resident_line(case)] if case.geom in GEOM else [p1, "k_pivot_fused<%d,%d,%d>" % (nt, unr, opt)]


def policy(case):
    """resident_geometry / fused_eligible / use_wg_single (jslp_hip.hip) restated for these cases: dense tableaus, no XCD-local build,
    no experiment knobs -> "g1".."g5", "fused", "select+update" or "workgroup" """
    i, env = case.inst, case.env
    H, ld, cap = i.H, _ld(i.W), i.cap or i.H
    force = env.get("JSLP_FORCE_PATH")
    if force is None and cap * ld <= 64 * 1024:
        return "workgroup"
    rpb, lean = _rpb(H), _lean(case)
    g = None
    if force == "fused":
        g = None
    elif i.n_opt > 0:
        if lean and i.n_unr == 0 and i.n_opt <= 3:
            g = "g1" if ld <= 2048 and rpb <= 8 else "g3" if ld <= 2048 and rpb <= 16 else None
    elif ld <= 2048 and rpb <= 8:
        g = "g2" if env.get("JSLP_RES_CPT") == "4" else "g1"
    elif lean and (i.n_unr == 0 or i.W + H + 2 <= 8192):  # (JSLP_R_LUNR: the lean build's LDS copy of the "unrestricted" flags)
        for name, rows in (("g3", 16), ("g4", 12), ("g5", 8)):
            if ld <= LD_MAX[name] and rpb <= rows:
                g = name
                break
    if g is not None:
        return g
    tiles = 4 if i.n_unr == 0 and i.n_opt == 0 else 2
    return "fused" if ld <= tiles * TW and cap <= 64 * MAXG else "select+update"


def product_instances():
    """the (T, C, R, unr, lean, opt, chk, xl) of every k_simplex_resident instance jslp_resident_table.hip.h launches, minus the XCD-local ones"""
    src = open(TU_RESIDENT).read()
    keys = set()
    b = lambda s: int(s == "true")  # noqa: E731
    for m in re.finditer(r"\blaunch<(\d+), (\d+), (\d+), (true|false), (true|false), (true|false), (true|false), (true|false)>\(", src):
        keys.add(tuple(int(x) for x in m.groups()[:3]) + tuple(b(x) for x in m.groups()[3:]))
    for m in re.finditer(r"\blaunch_lean<(\d+), (\d+), (\d+)>\(", src):  # unrestricted variables x cycle check
        keys |= {tuple(int(x) for x in m.groups()) + (u, 1, 0, c, 0) for u in (0, 1) for c in (0, 1)}
    return {k for k in keys if not k[7]}


# ---- CPU: the table, the policy, the planting ---------------------------------------------------------------------------------
def test_the_table_reaches_every_product_instance_at_the_full_grid():
    have = product_instances()
    assert len(have) == 28, sorted(have)
    full = {expected_key(c) for c in RESIDENT if c.G == MAXG}
    assert full == have, ("not covered at G = 256: %s; not an instance: %s" % (sorted(have - full), sorted(full - have)))


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_case_takes_the_geometry_it_names(case):
    assert policy(case) == case.geom
    if case.geom in GEOM:
        assert _grid(case.inst.H) == case.G and _ld(case.inst.W) <= LD_MAX[case.geom]
        T, C, _R = GEOM[case.geom]
        assert _rpb(case.inst.H) <= GEOM[case.geom][2] and T * C == LD_MAX[case.geom]


def test_the_full_grid_cases_sit_on_the_edges():
    """every geometry at G = 256 with its last workgroup full and with ONE row in it; the headline geometry's lanes all live"""
    for g, shapes in FULL.items():
        (H0, W0), (H1, W1) = shapes
        assert _grid(H0) == _grid(H1) == MAXG and H0 % _rpb(H0) == 0 and H1 % _rpb(H1) == 1, g
        assert _ld(W0) == LD_MAX[g] and _ld(W1) <= LD_MAX[g], g
    assert [_ld(c.inst.W) for c in CASES if c.id.startswith(("g4-2048x2049", "g5-2048x3073"))] == [2064, 3088]


@pytest.mark.parametrize("inst", INSTANCES, ids=["%dx%d-unr%d-opt%d%s%s" % (i.H, i.W, i.n_unr, i.n_opt, "-p1" if i.two_phase else "", "-cap%d" % i.cap if i.cap else "") for i in INSTANCES])
def test_planted_instances_pivot_on_the_edges(oracle_lib, inst):
    """on the oracle: a pivot row in the last workgroup, a pivot in column W-1, and the first phase-2 ratio test an exact tie between
    row 1 (workgroup 0) and row H-1 (the last workgroup), won by row 1; no cycle (so the check-off run's trace is this one)"""
    o = _oracle(oracle_lib, inst)
    res, trace = o["answer"][0], np.asarray(o["answer"][1]).reshape(-1, 2)
    H, W = inst.H, inst.W
    assert res["optimal"] and res["feasible"] and res["cycle_phase"] == 0, res
    assert (o["p1"] > 0) == inst.two_phase
    assert len(trace) >= 3
    assert (trace[:, 0] >= H - _rpb(H)).any(), "no pivot row in the last workgroup"
    assert (trace[:, 1] == W - 1).any(), "no pivot in column W-1"
    assert o["tie"] == {1, H - 1} and tuple(trace[o["p1"]]) == (1, o["c0"]), (o["tie"], trace[o["p1"]])


# ---- GPU: HIP against the oracle, and which kernel ran -------------------------------------------------------------------------
LAUNCH = re.compile(r"^\[jslp\] launch (.*)$", re.M)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_hip_equals_oracle_at_the_grid_edges(hip_lib, oracle_lib, monkeypatch, capfd, case):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    want = _oracle(oracle_lib, case.inst)["answer"]
    A, vibr, vibc, unr, oo, _c0 = planted(case.inst)
    capfd.readouterr()
    t = Tableau(A, vibr, vibc, unr, lib=hip_lib, optional_objectives=oo, row_capacity=case.inst.cap)
    try:
        got = _answer(t, t.simplex(check_cycles=case.chk))
        cnt = t.get_counters()
    finally:
        t.close()
    lines = LAUNCH.findall(capfd.readouterr().err)
    assert lines == expected_lines(case), lines
    _same(got, want)
    n_res = int(case.geom in GEOM)
    assert (cnt["resident_launches"], cnt["resident_aborts"], cnt["resident_refusals"], cnt["resident_handovers"]) == (n_res, 0, 0, 0), cnt
