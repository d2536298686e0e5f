"""Helpers of tests/test_cycle_edges.py (not a test module): instances whose detected cycle ends where an implementation of
checkForCycles (simplex.ts:415-440) changes code paths -- a history of 128 pairs (WGL_HIST, jslp_wglds.hip.h) or of 4096 pairs
(JSLP_PIPE_LHIST, jslp_resident_pipe.hip.h) --, the replay of a pivot trace into the history the check saw, and the check itself
restated.

Builders.  `with_fillers(model, k)` puts k constraints fc_i: {max: 1 + i % 3} and k variables f_i: {fc_i: 1, <objective>: -+1e6}
FIRST in the model: each filler is the most attractive column once, enters with one pivot and never again, and its row is zero in
every other column -- the rest of the run is the base model's own pivot sequence k rows, k columns and k pivots later (as long as
the base model's columns keep their place relative to the pricing batches, simplex.ts:118-127).  `late_model(small, n, seed, k)`
is the dense block of test_cycle_goldens._late_model (thousands of pivots) with k fillers in front and a small cycling LP behind.
`build(inst)` adds, for the tall / wide geometries, test_cycle_goldens._embed's zero-cost variables and constraints LAST."""
import os
from collections import namedtuple

import golden_util as G
from jslpsolver_amd import Model
from test_cycle_goldens import CYCLES, _embed, _late_model

EDGES = os.path.join(G.GOLDEN, "cycle_edges")
WGL_HIST = 128     # jslp_wglds.hip.h: histories shorter than this are wave 0's, on the LDS copy
PIPE_LHIST = 4096  # jslp_resident_pipe.hip.h: pairs 0..4095 in LDS, the rest in the workgroup's global slice only
FILLER_COST = 1e6


# ---- builders ----------------------------------------------------------------------------------------------------------------
def small_model(name):
    return G.load(os.path.join(CYCLES, "%s.json.gz" % name))["model"]


def with_fillers(model, k):
    """k filler constraints and variables in front of everything else (see the module docstring)"""
    cost = -FILLER_COST if model["opType"] != "max" else FILLER_COST  # attractive either way
    big = {"optimize": model["optimize"], "opType": model["opType"], "constraints": {}, "variables": {}}
    for i in range(k):
        big["constraints"]["fc_%d" % i] = {"max": 1 + i % 3}
        big["variables"]["f_%d" % i] = {"fc_%d" % i: 1, model["optimize"]: cost}
    big["constraints"].update(model["constraints"])
    big["variables"].update({name: dict(v) for name, v in model["variables"].items()})
    if "unrestricted" in model:
        big["unrestricted"] = dict(model["unrestricted"])
    big["options"] = {"presolve": False}
    return big


def late_model(small, n, seed, k):
    """resource allocation (seed, n x n, dense) as a minimisation + the small cycling LP, k fillers in front"""
    return with_fillers(_late_model(small, n, seed), k)


# kind "fill": with_fillers(small, k); "late": late_model(small, n, seed, k); extra = (variables, constraints) of _embed, or None
Inst = namedtuple("Inst", "name kind small k n seed extra B")


def _fill(small, k):
    return Inst("%s_k%d" % (small, k), "fill", small, k, 0, 0, None, WGL_HIST)


def _late(small, k, extra=None, tag=""):
    return Inst("late_%s_k%d%s" % (small, k, tag), "late", small, k, 1000, 3, extra, PIPE_LHIST)


TALL = (40, 500)   # _embed(extra variables, extra constraints): 2161+ rows, at most 1712 columns -> <512,4,16>
WIDE = (500, 8)    # 2161+ columns (ld 2176..2192), 1669+ rows -> <512,6,12>; fewer than 2601 columns: the batch stays 50

EDGE_128 = ([_fill("deg_35358", k) for k in (84, 85, 86, 87, 100, 110)] +   # history 127, 128, 129, 130 (second copy across), 143 (first copy across), 153 (beyond)
            [_fill("unr_3", k) for k in (122, 123, 124, 125)] +             # 127..130, length 2, unrestricted variables
            [_fill("deg_233528", k) for k in (103, 104)] +                  # length 7 at 128 and 129
            [_fill("deg_178868", k) for k in (102, 103)])                   # length 6 at 128 and 129
EDGE_4096 = ([_late(s, 650) for s in ("deg_292715", "deg_347708", "deg_233528", "deg_178868", "deg_398167", "deg_137788", "deg_35358")] +
             [_late("deg_35358", 600), _late("deg_35358", 700)])
TALL_WIDE = ([_late(s, 650, TALL, "_tall") for s in ("deg_233528", "deg_178868", "deg_35358")] +
             [_late(s, 650, WIDE, "_wide") for s in ("deg_233528", "deg_178868", "deg_35358")])
INSTANCES = EDGE_128 + EDGE_4096 + TALL_WIDE
BY_NAME = {i.name: i for i in INSTANCES}


def json_model(inst):
    small = small_model(inst.small)
    m = with_fillers(small, inst.k) if inst.kind == "fill" else late_model(small, inst.n, inst.seed, inst.k)
    return _embed(m, *inst.extra) if inst.extra else m


def build(inst):
    """-> (matrix, var_index_by_row, var_index_by_col, unrestricted variable indexes)"""
    model = Model(json_model(inst))
    return model.build_tableau() + (list(model.unrestricted),)


def base_of(inst):
    """the same instance without its fillers and without the embedding: what the filler shift is measured against"""
    return inst._replace(name="%s_%s_base" % (inst.kind, inst.small), k=0, extra=None)


# ---- the history of a run ----------------------------------------------------------------------------------------------------
def replay(trace, vibr, vibc, p1=0):
    """pivot trace [(row, col)] + the uploaded index maps -> ([(leaving variable, entering variable)] of phase 1, of phase 2, the maps
    after the last pivot): what simplex.ts:79-82 / 306-309 pushed before each pivot; pivot() swaps the two map entries (:339-343)"""
    vibr, vibc = [int(x) for x in vibr], [int(x) for x in vibc]
    pairs = []
    for r, c in trace:
        r, c = int(r), int(c)
        pairs.append((vibr[r], vibc[c]))
        vibr[r], vibc[c] = vibc[c], vibr[r]
    return pairs[:p1], pairs[p1:], vibr, vibc


def with_stop(pairs, start, length):
    """the history at a reported hit [start, length]: the pivoted pairs plus the selected-but-unpivoted pair that completed the square
    (the last element of the second copy, hence equal to the last element of the first)"""
    assert len(pairs) == start + 2 * length - 1, (len(pairs), start, length)
    return pairs + [pairs[start + length - 1]]


# ---- checkForCycles ----------------------------------------------------------------------------------------------------------
def check_for_cycles(var_indexes):
    """simplex.ts:415-440, loop for loop"""
    n = len(var_indexes)
    for e1 in range(0, n - 1):
        for e2 in range(e1 + 1, n):
            elt1 = var_indexes[e1]
            elt2 = var_indexes[e2]
            if elt1[0] == elt2[0] and elt1[1] == elt2[1]:
                if e2 - e1 > n - e2:
                    break
                cycle_found = True
                for i in range(1, e2 - e1):
                    tmp1 = var_indexes[e1 + i]
                    tmp2 = var_indexes[e2 + i]
                    if tmp1[0] != tmp2[0] or tmp1[1] != tmp2[1]:
                        cycle_found = False
                        break
                if cycle_found:
                    return [e1, e2 - e1]
    return []


def first_hit(pairs):
    """the check after every push, as the solve runs it: -> (history length at the first hit, [start, length]) or (None, []).
    A history whose prefixes had no hit can only hold a square that ENDS at its newest pair, so per push only the earlier occurrences
    of the newest pair are candidates for the last element of the first copy; the literal scan returns the smallest e1: the longest
    such square."""
    seen = {}
    for n1, p in enumerate(pairs, start=1):
        p = (p[0], p[1])
        for j in seen.get(p, ()):  # ascending: the longest block first
            L = n1 - 1 - j
            if 2 * L <= n1 and all(pairs[n1 - 2 * L + i][0] == pairs[n1 - L + i][0] and pairs[n1 - 2 * L + i][1] == pairs[n1 - L + i][1]
                                   for i in range(L - 1)):
                return n1, [n1 - 2 * L, L]
        seen.setdefault(p, []).append(n1 - 1)
    return None, []


def seen_without_square(pairs):
    """history lengths at which the newest pair had been selected before in the phase and no square was completed: where a pair filter
    says "seen" and the suffix test says "no" """
    seen, out = set(), []
    stop, _ = first_hit(pairs)
    for n1, p in enumerate(pairs, start=1):
        p = (p[0], p[1])
        if p in seen and n1 != stop:
            out.append(n1)
        seen.add(p)
    return out


def classify(n, start, length, B):
    """where a hit at history length n = start + 2 length sits relative to the boundary B (pairs 0..B-1 on one side)"""
    assert n == start + 2 * length
    if n < B:
        return "below"
    if n == B:
        return "n == B"
    if n == B + 1:
        return "n == B + 1"
    if start >= B:
        return "beyond"
    if start < B < start + length:
        return "first copy across"
    if n - length < B < n:
        return "second copy across"
    return "between the copies"
