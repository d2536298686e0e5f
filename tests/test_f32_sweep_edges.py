"""The instances k32_simplex_lds (jslpsolver_amd/csrc/jslp_f32_lds.hip.h) adds to the fp32 twin's table, at ITS tile edges, and the CPU
facts that keep them from being vacuous (runs without a GPU; tests/test_f32_sweep_gpu.py holds the kernel to the restatement on them).

The kernel's geometry: 1024 threads = 16 waves; the row update gives one wave one gated row, 16 bytes = 4 columns per lane, so one
wave-turn covers 256 columns; the pivot-column gather takes 2048 rows per turn; the LDS state of a tableau is
sizeof(F32Smem) + 4 * (3 * ld + 4 * hc) bytes with hc = the row capacity rounded up to 4, at most 64 KiB.
  t256 / t272 / t241   ld exactly one wave-turn / one turn + 16 columns / a padded tail inside the turn
  r18                  17 rows besides the pivot row: one past a whole round of 16 waves
  (tall, of test_fp32_exact: 1029 gated rows, past the first 1024-thread turn of the gated-row list)
  fits / overflows     the tallest 16-column tableau whose LDS state still fits / one step beyond it
"""
import functools
import os
import sys

import numpy as np
import pytest

import fp32_reference as R
from test_fp32_exact import CAP, MAX_PIVOTS, PRECISIONS, expected, instance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resident_stress import int_instance  # noqa: E402

THREADS, WAVES, TURN = 1024, 16, 256
SMEM_BYTES = 8 * 2 * 4 + 8 * 128 + 16  # sizeof(F32Smem): the selections' wave slots, the history prefix, three words + padding
LDS_MAX = 64 * 1024


def lds_bytes(ld, row_capacity):
    """f32lds_bytes of jslp_f32_lds.hip.h"""
    hc = (row_capacity + 3) // 4 * 4
    return SMEM_BYTES + 4 * (3 * ld + 4 * hc)


FITS_H = max(h for h in range(4, 5000) if lds_bytes(16, h) <= LDS_MAX)


def _cols(W, seed):  # (the seed: the first whose run does what test_column_instances_sit_at_the_wave_turn asks, chosen by the CPU run)
    m, vibr, vibc = int_instance(20, W - 1, seed)
    m[0, 1:W - 72] = -m[0, 1:W - 72]  # nothing prices in before the last 72 columns: the first pivots sit at the edge
    return m, vibr, vibc, ()


def _r18():
    m, vibr, vibc = int_instance(17, 30, 14)
    m[1:, 1:][np.random.default_rng(114).random((17, 30)) < 0.45] = 0.0  # the first pivots gate fewer rows than there are waves; fill-in does the rest
    return m, vibr, vibc, ()


def _lds_edge(extra):
    H = FITS_H
    m, vibr, vibc = int_instance(H - 1, 15, 13)
    m[1:, 0] *= 4.0
    # x_j <= 3 + j in rows on both sides of the 1024-thread turns and of the gather's 2048-row turn, the last row among them
    for j, r in enumerate((H - 1, 2049, 2047, 1025, 700, 3, H - 2, 3000, 1023, 2048, 1500, 2500, 3500, 10, H - 3)):
        m[r, 1:] = 0.0
        m[r, 1 + j] = 1.0
        m[r, 0] = 3.0 + j
    if extra:  # the same LP with one more (slack) row in the middle: the rows above it move down by one, the last row stays the last
        m = np.insert(m, 1200, m[1201] + 1.0, axis=0)
        vibr = np.array([-1] + list(range(15, 15 + H)), dtype=np.int32)
    return m, vibr, vibc, ()


EDGE_BUILDERS = {"t256": functools.partial(_cols, 256, 12), "t272": functools.partial(_cols, 272, 11), "t241": functools.partial(_cols, 241, 11),
                 "r18": _r18, "fits": functools.partial(_lds_edge, False), "overflows": functools.partial(_lds_edge, True)}
EDGE_NAMES = list(EDGE_BUILDERS)


@functools.lru_cache(maxsize=None)
def edge_instance(name):
    if name not in EDGE_BUILDERS:
        return instance(name)
    m, vibr, vibc, unr = EDGE_BUILDERS[name]()
    m.setflags(write=False)
    return m, vibr, vibc, tuple(unr)


@functools.lru_cache(maxsize=None)
def edge_expected(name, precision, check):
    """the float32 restatement's outcome, computed once and shared (old names: test_fp32_exact.expected's own cache)"""
    if name not in EDGE_BUILDERS:
        return expected(name, precision, check)
    m, vibr, vibc, unr = edge_instance(name)
    return R.solve(m, vibr, vibc, unr, precision, check, dtype=np.float32, max_pivots=CAP)


def _trace(name, precision=1e-5):
    return np.array(edge_expected(name, precision, True).trace, dtype=np.int64).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def gated_rows(name, precision=1e-5):
    """rows that pass the gate (simplex.ts:370-375), per pivot of the restatement's run: the trace replayed in binary32"""
    m = edge_instance(name)[0]
    ar = R._Arith(np.float32, None)
    A = np.array(ar.narrow(np.asarray(m, dtype=np.float64)), dtype=np.float32, ndmin=2)
    counts = []
    with np.errstate(all="ignore"):
        for pr, pc in edge_expected(name, precision, True).trace:
            gate = R.nonzero16(A[:, pc])
            gate[pr] = False
            counts.append(int(gate.sum()))
            R._pivot(A, ar, pr, pc)
    return counts


@pytest.mark.parametrize("name", EDGE_NAMES)
@pytest.mark.parametrize("check", [True, False], ids=["check", "nocheck"])
def test_edge_runs_end(name, check):
    for p in PRECISIONS:
        o = edge_expected(name, p, check)  # (raises at CAP = 3000)
        assert 1 <= o.it1 + max(o.it2, 0) <= MAX_PIVOTS
        assert o.cycle_phase == 0 and o.optimal


def test_the_lds_formula_is_the_kernels():
    text = open(os.path.join(ROOT, "jslpsolver_amd", "csrc", "jslp_f32_lds.hip.h")).read()
    assert "return sizeof(F32Smem) + 4 * (3 * (size_t)ld + 4 * hc);" in text
    assert "#define F32L_HIST 128" in text and "#define F32L_SEL 256" in text and "#define F32L_TURN 256" in text
    assert "static const size_t WGLDS_MAX_BYTES = 64 * 1024;" in open(os.path.join(ROOT, "jslpsolver_amd", "csrc", "jslp_hip.hip")).read()


def test_column_instances_sit_at_the_wave_turn():
    for name, ld in (("t256", 256), ("t272", 272), ("t241", 256)):
        W = edge_instance(name)[0].shape[1]
        assert (W + 15) // 16 * 16 == ld
        pcs = _trace(name)[:, 1]
        assert len(pcs) >= 20
        assert set((pcs % 4).tolist()) == {0, 1, 2, 3}, "a pivot column on every lane position of a 16-byte quad (both lanes of every pair)"
    assert edge_instance("t256")[0].shape[1] == TURN and _trace("t256")[:, 1].max() >= TURN - 16
    assert edge_instance("t241")[0].shape[1] == TURN - 15 and _trace("t241")[:, 1].max() >= TURN - 32
    pcs = _trace("t272")[:, 1]
    assert (pcs >= TURN).any() and (pcs < TURN).any(), "pivot columns on both sides of the first wave-turn"


def test_column_instances_price_in_batches():
    for name in ("t256", "t272", "t241"):
        m, vibr, vibc, unr = edge_instance(name)
        assert R.pricing_batch(m.shape[1]) == 50
        full = R.solve(m, vibr, vibc, unr, 1e-5, True, dtype=np.float32, max_pivots=CAP, full_pricing=True)
        assert full.trace != edge_expected(name, 1e-5, True).trace, name


def test_r18_gates_one_row_more_than_a_round_of_waves():
    assert edge_instance("r18")[0].shape[0] == WAVES + 2
    g = gated_rows("r18")
    assert len(g) >= 8
    assert max(g) == WAVES + 1, "every row but the pivot row: a second round with one row in it"
    assert min(g) <= WAVES - 1, "and pivots that need one round only"
    assert any(x == WAVES for x in g), "and exactly one whole round"


def test_tall_gates_more_rows_than_one_turn_of_the_list_loop():
    assert max(gated_rows("tall")) > THREADS


def test_lds_pair_straddles_the_budget():
    for name, H, fits in (("fits", FITS_H, True), ("overflows", FITS_H + 1, False)):
        m = edge_instance(name)[0]
        assert m.shape == (H, 16)
        assert (lds_bytes(16, H) <= LDS_MAX) == fits
        assert H * 16 <= 64 * 1024, "small enough for AUTO's first bound: the LDS fit alone decides"
        prs = _trace(name)[:, 0]
        assert len(prs) >= 8
        assert (prs > 2048).any() and (prs < 2048).any(), "pivot rows on both sides of the column gather's turn"
        assert (prs > 1024).any() and (prs < 1024).any()
        assert (prs == H - 1).any(), "the last row pivots"
        assert max(gated_rows(name)) > 2 * THREADS
    assert lds_bytes(16, FITS_H) == LDS_MAX or lds_bytes(16, FITS_H + 4) > LDS_MAX
    assert FITS_H % 4 == 0, "one more row is one more step of the row capacity's rounding"
