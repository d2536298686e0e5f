#!/usr/bin/env python3
"""How often is every row gate of the resident update pass open?  CPU only.

  python tools/gate_openness.py 3a N | 3b N | fixture NAME   [--rows 8]

Solves one instance with the CPU oracle (oracle/libjslp_oracle.so), replays its pivot trace in numpy (the oracle's pivot(), simplex.ts:330-392,
restated: same operands, same two roundings per cell; the replay's final tableau is compared with the oracle's bit for bit) and looks, in front
of every pivot, at what the update pass of the register-resident kernels will see (JSLP_XL_UPDATE_PASS, jslp_resident_pipe.hip.h):
  * the pivot column's entries k of all rows but the pivot row: the row gate is `|k| > 1e-16`;
  * the normalised pivot row's entries: the column gate (the EXEC mask) is the same test.
Prints the share of (workgroup of --rows rows, pivot) pairs in which every live row's gate is open -- the pairs that take the gate-free arm --
and the failing entries per pivot column and per pivot row.
  3a N: generators.dense_resource_allocation_tableau(12345, N, N) (bench.py's headline at N = 2000); 3b N: dense_random_lp_tableau(12345, N, N);
  fixture NAME: the root tableau of tests/golden/fixtures/NAME.json.gz (Monster_Problem: a sparse model, for contrast)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from jslpsolver_amd import _capi, generators  # noqa: E402
from jslpsolver_amd.engine import Tableau  # noqa: E402


def nonzero16(v):
    return ~((v >= -1e-16) & (v <= 1e-16))  # (NaN counts as non-zero, as in the reference)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=("3a", "3b", "fixture"))
    ap.add_argument("what")
    ap.add_argument("--rows", type=int, default=8, help="rows per workgroup")
    a = ap.parse_args()
    unr, prec = [], 1e-8
    if a.kind == "3a":
        n = int(a.what)
        M, vibr, vibc = generators.dense_resource_allocation_tableau(12345, n, n)
        label = "3a n = %d" % n
    elif a.kind == "3b":
        n = int(a.what)
        M, vibr, vibc, _ = generators.dense_random_lp_tableau(12345, n, n)
        label = "3b n = %d" % n
    else:
        import golden_util as G
        g = G.load(os.path.join(G.GOLDEN, "fixtures", a.what + ".json.gz"))
        M, vibr, vibc = G.dense_tableau(g["tableau"])
        unr, prec = g["tableau"]["unrestricted"], g["tableau"]["precision"]
        label = "%s (root relaxation)" % a.what
    M = np.ascontiguousarray(M, dtype=np.float64)
    H, W = M.shape
    oracle = _capi.Library(os.path.join(ROOT, "oracle", "libjslp_oracle.so"))
    t0 = time.perf_counter()
    t = Tableau(M, vibr, vibc, unr, precision=prec, lib=oracle)
    res = t.simplex(check_cycles=True)
    trace = t.pivot_trace().tolist()
    final = t.download()[0]
    t.close()
    t_solve = time.perf_counter() - t0
    G_ = (H + a.rows - 1) // a.rows
    wg_of = np.arange(H) // a.rows
    pairs_open = 0
    col_fail = np.zeros(len(trace), dtype=np.int64)
    row_fail = np.zeros(len(trace), dtype=np.int64)
    buf = np.empty_like(M)
    t0 = time.perf_counter()
    for it, (pr, pc) in enumerate(trace):
        quot = M[pr, pc]
        row = M[pr]
        nz = nonzero16(row)
        with np.errstate(all="ignore"):
            p = np.where(nz, row / quot, 0.0)
        p[pc] = 1.0 / quot
        k = M[:, pc].copy()
        gate = nonzero16(k)
        gate[pr] = False
        shut = ~gate
        shut[pr] = False
        col_fail[it] = int(shut.sum())
        pairs_open += G_ - len(set(wg_of[shut].tolist()))
        live = nz & nonzero16(p)
        row_fail[it] = W - int(live.sum())
        if gate.any():
            p[nz & ~live] = 0.0  # (a normalised entry under the gate is zeroed by the first row that meets it, :388-390)
        with np.errstate(all="ignore"):
            if col_fail[it] == 0 and row_fail[it] == 0:
                k[pr] = 0.0
                np.multiply.outer(k, p, out=buf)
                keep = M[pr].copy()
                np.subtract(M, buf, out=M)
                M[pr] = keep
                k[pr] = quot
            else:
                rows_, cols_ = np.nonzero(gate)[0], np.nonzero(live)[0]
                M[np.ix_(rows_, cols_)] = M[np.ix_(rows_, cols_)] - np.multiply.outer(k[rows_], p[cols_])
            M[gate, pc] = -k[gate] / quot
        M[pr] = p
    t_replay = time.perf_counter() - t0
    same = M.view(np.int64).tobytes() == np.ascontiguousarray(final).view(np.int64).tobytes()
    n = len(trace)
    print("| instance | tableau | pivots (phase 1 + 2) | (workgroup of %d rows, pivot) pairs with every gate open | failing entries per pivot column: mean, max | pivots with any | failing entries per pivot row: mean, max | replay = oracle |"
          % a.rows)
    print("|---|---|---|---|---|---|---|---|")
    print("| %s | %d x %d | %d (%d + %d) | %d of %d = %.4f %% | %.4f, %d | %d | %.3f, %d | %s |" % (
        label, H, W, n, res.pivots_phase1, max(res.pivots_phase2, 0), pairs_open, G_ * n, 100.0 * pairs_open / max(G_ * n, 1),
        col_fail.mean() if n else 0.0, col_fail.max() if n else 0, int((col_fail > 0).sum()), row_fail.mean() if n else 0.0,
        row_fail.max() if n else 0, "bit for bit" if same else "DIFFERS"))
    print("(oracle solve %.1f s, replay %.1f s)" % (t_solve, t_replay), file=sys.stderr)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
