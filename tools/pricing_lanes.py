#!/usr/bin/env python3
"""How many lanes take part in the LDS-atomic rounds of the lean resident kernels' pricing?  CPU only.

  python tools/pricing_lanes.py 3a N | 3b N   [--cpt 2]

Solves one instance with the CPU oracle, replays its pivot trace in numpy (as tools/gate_openness.py does: same operands, same two roundings per
cell; the replay's final tableau is compared with the oracle's bit for bit) and looks, in front of every pivot, at the cost row as
price_row_pipe (jslp_resident_pipe.hip.h) sees it: lane t holds columns t CPT .. t CPT + CPT - 1 and offers its best column (earliest batch, then
the larger value, then the first index); round 2 (`ds_max_u64`) is run by the lanes whose offer lies in the winning batch, round 3 (`ds_min_i32`)
by those of them that hold the maximum.  Phase-1 pivots price by quotient over the whole pivot row (step E1): their second round is run by the
lanes that hold the best quotient.  Prints mean, p99 and max of the lanes per pivot and of the lanes in the busiest WAVE of a pivot (a wave's
same-address atomics are serialised inside the LDS unit), and checks that the entering column the rounds name is the oracle's.
  3a N: generators.dense_resource_allocation_tableau(12345, N, N) (bench.py's headline at N = 2000); 3b N: dense_random_lp_tableau(12345, N, N)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jslpsolver_amd import _capi, generators  # noqa: E402
from jslpsolver_amd.engine import Tableau  # noqa: E402


def nonzero16(v):
    return ~((v >= -1e-16) & (v <= 1e-16))


def stats(x):
    x = np.asarray(x)
    return "%.2f / %d / %d" % (x.mean(), int(np.percentile(x, 99)), x.max()) if len(x) else "-"


def two_round_lanes(cost, cand, batch_of, lane_of):
    """price_row_pipe's two-round form restated on its packed keys: round 1 is a 64-bit maximum of {127 - batch : 7 | value bits >> 6 : 57} over the
    lanes' offers, round 2 a 32-bit maximum of {value bits & 63 : 6 | 65535 - column : 16} among the lanes whose first key won.  Returns the column
    the two rounds name and the lanes that go through round 1 in either form (every lane with a candidate / the lanes of their wave's earliest
    batch) and through round 2."""
    ci = np.nonzero(cand)[0]
    order = np.lexsort((ci, -cost[ci], batch_of[ci], lane_of[ci]))  # a lane's offer: earliest batch, larger value, first column
    ci = ci[order]
    ln = lane_of[ci]
    first = np.r_[True, ln[1:] != ln[:-1]]
    col, ln = ci[first], ln[first]
    bits = np.ascontiguousarray(cost[col]).view(np.uint64)
    bb = batch_of[col].astype(np.uint64)
    assert bb.max() <= 127 and col.max() <= 0xffff
    key1 = ((np.uint64(127) - bb) << np.uint64(57)) | (bits >> np.uint64(6))
    wv = ln // 64
    wave_first = np.r_[True, wv[1:] != wv[:-1]]  # (lanes ascend: a wave's first candidate lane holds its earliest batch)
    wave_b = np.zeros(wv.max() + 1, dtype=np.uint64)
    wave_b[wv[wave_first]] = bb[wave_first]
    early = bb == wave_b[wv]
    w1 = key1.max()
    assert key1[early].max() == w1
    second = key1 == w1
    key2 = ((bits & np.uint64(63)) << np.uint64(16)) | (np.uint64(0xffff) - col.astype(np.uint64))
    w2 = int(key2[second].max())
    return 0xffff - (w2 & 0xffff), ln, ln[early], ln[second]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=("3a", "3b"))
    ap.add_argument("n", type=int)
    ap.add_argument("--cpt", type=int, default=2, help="columns per lane")
    a = ap.parse_args()
    prec = 1e-8
    if a.kind == "3a":
        M, vibr, vibc = generators.dense_resource_allocation_tableau(12345, a.n, a.n)
    else:
        M, vibr, vibc, _ = generators.dense_random_lp_tableau(12345, a.n, a.n)
    M = np.ascontiguousarray(M, dtype=np.float64)
    H, W = M.shape
    oracle = _capi.Library(os.path.join(ROOT, "oracle", "libjslp_oracle.so"))
    t = Tableau(M, vibr, vibc, [], precision=prec, lib=oracle)
    res = t.simplex(check_cycles=True)
    trace = t.pivot_trace().tolist()
    final = t.download()[0]
    t.close()
    batch = min(500, max(50, int(np.floor(np.sqrt(W - 1)))))
    partial = (W - 1) > 2 * batch
    cols = np.arange(W)
    lane_of = cols // a.cpt
    wave_of = lane_of // 64
    batch_of = np.where(cols >= 1, (cols - 1) // batch, 0) if partial else np.zeros(W, dtype=np.int64)
    r2, r3, r2w, r3w, p1, p1w = [], [], [], [], [], []
    # the two-round pricing (profiles/pricing_two_rounds.md): who goes through its FIRST round -- "all": every lane that holds a candidate;
    # "earliest": the lanes whose offer lies in their own wave's earliest batch -- and who goes through its second (top 57 bits equal to the winner's)
    t1 = {"all": ([], []), "earliest": ([], [])}
    t2, t2w = [], []
    wrong = wrong2 = 0
    buf = np.empty_like(M)
    for it, (pr, pc) in enumerate(trace):
        if it >= res.pivots_phase1:
            cost = M[0]
            cand = (cols >= 1) & (cost > prec)
            wb = batch_of[cand].min()
            inb = cand & (batch_of == wb)
            # a lane's offer lies in the winning batch iff its EARLIEST candidate does: batches ascend with the column
            first_b = np.full(lane_of.max() + 1, 1 << 30)
            np.minimum.at(first_b, lane_of[cand], batch_of[cand])
            lanes2 = np.nonzero(first_b == wb)[0]
            best = np.full(lane_of.max() + 1, -np.inf)
            np.maximum.at(best, lane_of[inb], cost[inb])
            top = best[lanes2].max()
            lanes3 = lanes2[best[lanes2] == top]
            pick = int(np.nonzero(inb & (cost == top))[0][0])
            wrong += pick != pc
            r2.append(len(lanes2)); r3.append(len(lanes3))
            r2w.append(np.bincount(lanes2 // 64).max()); r3w.append(np.bincount(lanes3 // 64).max())
            pick2, lanes_all, lanes_early, lanes_second = two_round_lanes(cost, cand, batch_of, lane_of)
            wrong2 += pick2 != pc
            for form, lanes in (("all", lanes_all), ("earliest", lanes_early)):
                t1[form][0].append(len(lanes)); t1[form][1].append(np.bincount(lanes // 64).max())
            t2.append(len(lanes_second)); t2w.append(np.bincount(lanes_second // 64).max())
        else:
            coef = M[pr]
            cand = (cols >= 1) & (coef < -prec)
            with np.errstate(all="ignore"):
                quo = np.where(cand, -M[0] / np.where(cand, coef, 1.0), -np.inf)
            top = quo.max()
            lanes = np.unique(lane_of[cand & (quo == top)])
            wrong += int(np.nonzero(cand & (quo == top))[0][0]) != pc
            p1.append(len(lanes)); p1w.append(np.bincount(lanes // 64).max())
        # the pivot (tools/gate_openness.py)
        quot = M[pr, pc]
        row = M[pr]
        nz = nonzero16(row)
        with np.errstate(all="ignore"):
            p = np.where(nz, row / quot, 0.0)
        p[pc] = 1.0 / quot
        k = M[:, pc].copy()
        gate = nonzero16(k)
        gate[pr] = False
        live = nz & nonzero16(p)
        if gate.any():
            p[nz & ~live] = 0.0
        with np.errstate(all="ignore"):
            rows_, cols_ = np.nonzero(gate)[0], np.nonzero(live)[0]
            if len(rows_) == H - 1 and len(cols_) == W:
                k[pr] = 0.0
                np.multiply.outer(k, p, out=buf)
                np.subtract(M, buf, out=M)
                k[pr] = quot
            else:
                M[np.ix_(rows_, cols_)] = M[np.ix_(rows_, cols_)] - np.multiply.outer(k[rows_], p[cols_])
            M[gate, pc] = -k[gate] / quot
        M[pr] = p
    same = M.view(np.int64).tobytes() == np.ascontiguousarray(final).view(np.int64).tobytes()
    print("| instance | columns per lane | pivots (phase 1 + 2) | round 2 lanes per pivot: mean / p99 / max | ... in the busiest wave | round 3 lanes | ... in the busiest wave | phase-1 second round lanes | ... in the busiest wave | entering column = oracle's | replay = oracle |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    print("| %s n = %d | %d | %d (%d + %d) | %s | %s | %s | %s | %s | %s | %s | %s |" % (
        a.kind, a.n, a.cpt, len(trace), res.pivots_phase1, max(res.pivots_phase2, 0), stats(r2), stats(r2w), stats(r3), stats(r3w), stats(p1), stats(p1w),
        "every pivot" if wrong == 0 else "%d DIFFER" % wrong, "bit for bit" if same else "DIFFERS"))
    if t2:
        print()
        print("| instance | columns per lane | two-round pricing: round 1 lanes per workgroup, every candidate lane: mean / p99 / max | ... in the busiest wave | round 1 lanes per workgroup, the waves' earliest batches | ... in the busiest wave | round 2 lanes per workgroup | ... in the busiest wave | entering column = oracle's |")
        print("|---|---|---|---|---|---|---|---|---|")
        print("| %s n = %d | %d | %s | %s | %s | %s | %s | %s | %s |" % (
            a.kind, a.n, a.cpt, stats(t1["all"][0]), stats(t1["all"][1]), stats(t1["earliest"][0]), stats(t1["earliest"][1]), stats(t2), stats(t2w),
            "every pivot" if wrong2 == 0 else "%d DIFFER" % wrong2))
    return 0 if same and wrong == 0 and wrong2 == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
