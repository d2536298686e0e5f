"""What a branch-and-bound call LEAVES BEHIND in the engine's live tableau (slot 0), which the sequential services read after every node
(mir_loop, createCheckpoint / jslp_engine_relax_from, save(), download(), read_rhs(), optional_objectives()): HIP against the CPU oracle,
byte for byte, NaN canonicalised (GPU and x86 make different NaN payloads), -0.0 kept.  No tolerance, no skip.

1. WALKS.  A walk is a list of ABI calls on ONE engine (build_walk), chosen on the oracle from what the calls before it left and recorded
with the oracle's observation after every step: the result struct(s), evaluation / feasible / height, read_rhs(), the five arrays of
download() and, on a "+opt" root, optional_objectives().  tests/live_tableau_worker.py replays the recorded steps on the GPU, one
subprocess per setting of the JSLP_* knobs, compares every observation and, under JSLP_DEBUG_LAUNCH=1, the launch lines of every relax
call with the dispatcher's bookkeeping restated (LiveDispatch there).  After a call whose live tableau the ABI leaves unspecified
(relax_batch with several nodes, any refused call) only the outcomes / the error code are compared and the next step is one that is
defined whatever the slot holds.  A walk covers, per root: single nodes after save() (several launches), again (the one-launch kernel),
after batches of 2, 16, 17 and a batch larger than the queue kernel's resident workgroups (roots whose slots fit LDS and the 4 M cell
limit), every batch twice so that its second run is the one-launch kernel; refused cut lists and the node and checkpoint after them; applyCuts -> mirRound x 3 -> applyCuts, applyMIRCuts alone -> applyCuts;
createCheckpoint after a one-launch node, a several-launch node, a mirRound, a grandchild, restore(), add_cuts, simplex() and pivot(),
each restored after a deeper node and a batch and compared with what was observed when it was taken; 1, 2, 3 and 17 children of a
checkpoint taller than the root (into a slot that last held the tallest node there is; the spare rows used up exactly; one cut too many);
an infeasible node straight after a three-child call, which reports the ENGINE's evaluation: the last child's;
the root again after a checkpoint call; restoreCheckpoint -> save() and nodes, batches, checkpoints of the new root, ids recycled.

An infeasible or refused node of a BATCH reports the evaluation its call started from (fill_result), the oracle's sequential batch the
one the node before it left: as in test_node_edges the expectation is the oracle's outcome with that one field restated, and every batch
of a walk ends on a node with an optimum so that the engine's own evaluation is the same on both sides afterwards.

Multi-child jslp_engine_relax_from is absent from the "+opt" roots: a checkpoint carries no optional objectives and the other slots'
objective rows are whatever an earlier batch left, which the sequential reference has no equivalent of (include/jslp_engine.h).
The large roots (2049 x 15, 2590 x 15 without an LDS fit, 15 x 1040 with 4.26 M cells) run under the first three settings only;
JSLP_FORCE_PATH=sp (every node through the chip-wide kernels, one after the other) runs the tiny, the 41 x 15 and the 258 x 15 roots.

2. k_mir_cuts ALONE on crafted uploads (mir_cases): which rows get a cut against the kernel's 256-row chunks, its four-wave ballot and
the limit of 10; widths against the 256-thread column loop; non-finite and signed-zero cells; right-hand sides at the precision
threshold; row capacity exact and one short (the code only: the oracle appends rows until it runs out, the kernel none) and the same
engine after upload() again.

CPU: the whole oracle plan (13 walks of 94 to 119 steps, 52 MIR cases) takes 5 s, 1.5 s of it the 2049 x 15 walk with its three 1100-node batches.
GPU time of this module on an MI355X: 19 s (7 tests, the slowest 4.2 s) inside a full `-m gpu` run of 673 s, which leaves 654 s for the
parent's suite on that box; tests/test_node_edges.py took 199 s in the same run (the bound is half of that).
"""
import hashlib
import math
import os
import pickle
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

import golden_util as G
import test_node_edges as N
from node_edges_worker import WG_CELLS_BATCH
from jslpsolver_amd import _capi
from jslpsolver_amd.engine import Tableau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "live_tableau_worker.py")
RAW_LIMIT = 32 * 1024  # observations up to this many bytes are kept whole (a mismatch then names the first differing cell), larger ones as a digest
LIVE = ("evaluation", "feasible", "height", "rhs", "rows", "A", "vibr", "vibc", "rbv", "cbv", "oo")


# ---- roots: test_node_edges' own, by name, and 258 x 15 (the first row of the second MIR chunk) -------------------------------------
ROOT_NAMES = ("tiny 2x2", "tiny 7x6+opt", "stride 41x15 cap 44", "stride 41x15 cap 45", "stride 41x15 cap 46", "stride 41x15 cap 47",
              "ld 15x129+unr", "ld 15x1040", "H 258x15", "H 513x15+opt", "H 2049x15", "fit 2590x15 cap 2610", "cells 15x1040 cap 4100")
LARGE_ROOTS = ("H 2049x15", "fit 2590x15 cap 2610", "cells 15x1040 cap 4100")
SP_ROOTS = tuple(n for n in ROOT_NAMES if n.startswith(("tiny", "stride", "H 258")))
SETTINGS = {
    "defaults": {},
    "cow0": {"JSLP_NODE_COW": "0"},
    "cowsingle0": {"JSLP_NODE_COW_SINGLE": "0"},
    "nowglds": {"JSLP_NO_WGLDS": "1"},
    "nonodekernel": {"JSLP_NO_NODE_KERNEL": "1"},
    "sp": {"JSLP_FORCE_PATH": "sp"},
}


def roots_of(setting):
    if setting == "sp":
        return list(SP_ROOTS)
    if setting in ("nowglds", "nonodekernel"):
        return [n for n in ROOT_NAMES if n not in LARGE_ROOTS]
    return list(ROOT_NAMES)


def root_spec(name):
    if name == "H 258x15":
        return dict(name=name, rows=258, cols=15, cap=258 + N.SPARE, seed=1000 + 7 * 258 + 15, unr=False, opt=False)
    return next(s for s in N.root_specs() + N.root_specs(large=True) if s["name"] == name)


def queue_sized(root):
    """a batch larger than the queue kernel's resident workgroups makes sense where the defaults would send it to that kernel"""
    ld = (root["cols"] + 15) // 16 * 16
    return N.wglds_bytes(ld, root["cap"]) <= N.WGLDS_MAX_BYTES and root["cap"] * ld <= WG_CELLS_BATCH


# ---- observations --------------------------------------------------------------------------------------------------------------------
def canon(x):
    """bytes of an array or a float with every NaN made the same NaN (-0.0 kept): test_selection_edges._canon"""
    a = np.asarray(x)
    if a.dtype.kind == "f":
        a = G.canon_nan(a)
    return np.ascontiguousarray(a).tobytes()


def pack(x):
    b = canon(x)
    return ("raw", str(np.asarray(x).dtype), zlib.compress(b, 1)) if len(b) <= RAW_LIMIT else ("sha1", len(b), hashlib.sha1(b).hexdigest())


def first_difference(want, got):
    """where two packed observations differ, in words"""
    if want[0] != "raw" or got[0] != "raw":
        return "digests differ (%s bytes / %s bytes)" % (want[1], got[1])
    a, b = np.frombuffer(zlib.decompress(want[2]), dtype=want[1]), np.frombuffer(zlib.decompress(got[2]), dtype=got[1])
    if a.shape != b.shape:
        return "%d entries expected, %d found" % (a.size, b.size)
    at = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(axis=1))
    return "%d entries differ, the first at %d: expected %r, found %r" % (at.size, at[0], a[at[0]], b[at[0]]) if at.size else "equal"


def result_dict(res):
    return {k: (canon(v) if isinstance(v, float) else int(v)) for k, v in res.as_dict().items()}


def node_digest(res, rhs, rows, evaluation=None):
    """one node of a batch: the result struct (evaluation restated where the node has no optimum), RHS column and row map up to the height"""
    d = result_dict(res)
    if evaluation is not None:
        d["evaluation"] = canon(float(evaluation))
    h = res.height
    blob = repr(sorted(d.items())).encode() + canon(np.asarray(rhs[:h], dtype=np.float64)) + canon(np.asarray(rows[:h], dtype=np.int32))
    return hashlib.sha1(blob).digest()[:10]


REFUSALS = (_capi.JSLP_ERR_ARG, _capi.JSLP_ERR_STATE, _capi.JSLP_ERR_CAPACITY)


def error_code(exc):
    """the code of a call the engine REFUSED.  Any other failure (JSLP_ERR_DEVICE: a fault the runtime reported, out of memory) is no
    observation to compare: it is raised as it is, no assertion, and ends the process that met it -- nothing more is started on that GPU"""
    code = N.error_code(exc)
    if code not in REFUSALS:
        raise RuntimeError("the engine failed, it did not refuse: %s" % exc) from exc
    return code


class Runner:
    """one engine and the steps of a walk on it; do(step) returns the observation of the step.  Used with the oracle to record a walk and
    by the worker to replay it on the GPU: the same code looks at both."""

    def __init__(self, lib, root):
        self.lib, self.root = lib, root
        self.t = Tableau(root["A"], root["vibr"], root["vibc"], root["unr_list"], lib=lib, row_capacity=root["cap"], optional_objectives=root["oo"])
        self.cks = {}
        self.raw = None  # arrays of the last live observation (the recorder chooses cuts from them)
        self.call_eval = 0.0  # the engine's evaluation, tracked as fill_result does

    def close(self):
        self.t.close()

    def live(self):
        t = self.t
        rhs, rows = t.read_rhs()
        A, vibr, vibc, rbv, cbv = t.download()
        self.raw = dict(rhs=rhs, rows=rows, A=A, vibr=vibr, vibc=vibc, rbv=rbv, cbv=cbv)
        out = dict(evaluation=canon(float(t.evaluation)), feasible=bool(t.feasible), height=int(t.height), rhs=pack(rhs), rows=pack(rows),
                   A=pack(A), vibr=pack(vibr), vibc=pack(vibc), rbv=pack(rbv), cbv=pack(cbv))
        if self.root["oo"] is not None:
            out["oo"] = pack(t.optional_objectives())
        return out

    def _track(self, res, prev):
        self.call_eval = res.evaluation if res.optimal else (float("-inf") if not res.bounded else prev)

    def do(self, step):
        op, t = step[0], self.t
        try:
            if op == "simplex":
                res = t.simplex(check_cycles=self.root["check"])
                self._track(res, self.call_eval)
                return dict(res=result_dict(res), live=self.live())
            if op in ("save", "restore"):
                getattr(t, op)()
                return dict(live=self.live())
            if op == "cuts":
                res, rhs, rows = t.applyCuts(step[1], check_cycles=True)
                self._track(res, self.call_eval)
                return dict(res=result_dict(res), out=(pack(rhs), pack(rows)), live=self.live())
            if op == "batch":  # the live tableau is unspecified afterwards: the outcomes only
                res, rhs, rows = t.applyCutsBatch(step[1], check_cycles=True)
                prev = self.call_eval
                # (the oracle's sequential batch hands a node without an optimum the evaluation the node before it left: restated, on the oracle only)
                restate = self.lib.backend == "oracle-c"
                nodes = [node_digest(r, rhs[j], rows[j], prev if restate and not r.optimal and r.bounded else None) for j, r in enumerate(res)]
                self._track(res[-1], prev)
                return dict(nodes=nodes, last_optimal=bool(res[-1].optimal))
            if op == "ints":
                iv = _capi.as_i32(list(step[1]))
                t.lib.check(t.lib.jslp_engine_set_integer_variables(t._h, _capi.ptr_i32(iv), int(iv.shape[0])), "jslp_engine_set_integer_variables")
                return {}
            if op == "mir":
                n, res, rhs, rows = t.mirRound(check_cycles=True)
                self._track(res, self.call_eval)
                return dict(added=int(n), res=result_dict(res), out=(pack(rhs), pack(rows)), live=self.live())
            if op == "mircuts":
                return dict(added=int(t.applyMIRCuts()), live=self.live())
            if op == "addcuts":
                t.addCutConstraints(step[1])
                return dict(live=self.live())
            if op == "pivot":
                t.pivot(step[1], step[2])
                return dict(live=self.live())
            if op == "ck":
                ck = t.createCheckpoint()
                self.cks[step[1]] = (ck, self.call_eval)
                return dict(id=int(ck["id"]), live=self.live())
            if op == "rck":
                ck, ev = self.cks[step[1]]
                t.restoreCheckpoint(ck)
                self.call_eval = ev
                return dict(live=self.live())
            if op == "rel":
                t.releaseCheckpoint(self.cks.pop(step[1])[0])
                return {}
            if op == "from":  # (checkpoint name, cut lists, observe the live tableau afterwards)
                ck, ev = self.cks[step[1]]
                outs = t.applyCutsFrom(ck, step[2], check_cycles=True)
                for res, _, _ in outs:
                    t.absorb_from(ck, res)
                self._track(outs[-1][0], ev)
                obs = dict(nodes=[node_digest(*o) for o in outs], res=result_dict(outs[-1][0]))
                if step[3]:
                    obs["live"] = self.live()
                return obs
            raise ValueError(op)
        except _capi.EngineError as e:  # a refused call: the code, and nothing about the tableau
            return dict(error=error_code(e))


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
def cut(kind, var, value):
    return {"type": kind, "varIndex": int(var), "value": float(value)}


def fractional_basics(raw):
    rhs, rows = raw["rhs"], raw["rows"]
    return [(int(rows[r]), float(rhs[r])) for r in range(1, len(rows)) if math.isfinite(rhs[r]) and abs(rhs[r] - round(rhs[r])) > 1e-6]


def child_cuts(raw, n):
    """n single-cut lists on the tableau `raw` was read from: floor / ceil on its fractional basic variables, then bounds further out;
    a tableau without a fractional basic value is cut on its first basic variables instead"""
    basics = fractional_basics(raw) or [(int(raw["rows"][r]), float(raw["rhs"][r])) for r in range(1, len(raw["rows"]))]
    out, k = [], 0
    while len(out) < n:
        v, x = basics[k % len(basics)]
        away = k // len(basics)
        out.append([cut("max", v, math.floor(x) - away)])
        out.append([cut("min", v, math.ceil(x) + away)])
        k += 1
    return out[:n]


class Recorder:
    def __init__(self, oracle_lib, root):
        self.run, self.root, self.steps, self.obs = Runner(oracle_lib, root), root, [], []

    def __call__(self, *step):
        o = self.run.do(step)
        self.steps.append(step)
        self.obs.append(o)
        return o


def build_walk(rec, root):
    fam, want, n = root["family"], root["want"], len(root["family"])
    single = [k for k in range(n) if len(fam[k]) == 1]
    piv = [k for k in single if want[k]["optimal"] and want[k]["p1"] + max(want[k]["p2"], 0) > 0] or [k for k in range(n) if want[k]["optimal"]]
    inf = [k for k in single if not want[k]["feasible"]] or piv
    opt = root["oo"] is not None
    spare = root["cap"] - root["H"]

    def node(i):
        return fam[piv[i % len(piv)]]

    def batch(size, start):  # a window of the family that ends on a node with an optimum
        return [fam[(start + i) % n] for i in range(size - 1)] + [node(start)]

    big = [fam[k] for _ in range(max(30, -(-1100 // n))) for k in range(n)] + [node(0)] if queue_sized(root) else None

    def settle():
        """a checkpoint carries no optional objectives: restoreCheckpoint after a batch would show the rows of whichever node the batch
        left in slot 0, so on a "+opt" root restore() brings the saved root's back first"""
        if opt:
            rec("restore")

    # ---- the root, and nodes of it in every state of the slots
    rec("simplex")
    rec("save")
    rec("cuts", node(0))  # slot 0 not yet in sync: several launches
    rec("cuts", fam[inf[0]])  # the one-launch kernel; an infeasible node
    rec("cuts", node(1))
    for size in (2, 16, 17):  # each batch twice: the first brings its slots in sync (several launches), the second is one launch
        rec("batch", batch(size, size))
        rec("batch", batch(size, size + 1))
        rec("cuts", node(size))
    if big:  # (twice for the same reason: the second goes through the queue kernel)
        rec("batch", big)
        rec("batch", big)
        rec("cuts", node(3))
    # ---- refused lists, the node and the checkpoint after them
    taken = []
    for label, cuts, code in (root["bad"][0], root["bad"][3]):
        assert rec("cuts", cuts) == dict(error=code), (root["name"], label)
        rec("cuts", node(len(taken)))
        rec("ck", "after " + label)
        taken.append("after " + label)
    # ---- MIR after a node, as mir_loop runs it; the node after it must not see the MIR rows or their slack indexes
    rec("cuts", node(0))
    frac = fractional_basics(rec.run.raw)
    # (room for ten rows a round where there is any; one candidate where the spare rows are a handful)
    rec("ints", list(range(root["rows"] + root["cols"] - 2)) if spare >= 40 else [v for v, _ in frac[:1]])
    tall = None
    for i in range(3):
        o = rec("mir")
        if "error" in o or o["added"] == 0:
            break
        if tall is None:
            rec("ck", "mir")
            tall = "mir"
            taken.append("mir")
    rec("cuts", node(1))
    rec("mircuts")
    rec("cuts", node(2))
    # ---- a checkpoint after each kind of call
    rec("cuts", node(0))  # one launch (copy-on-write under the defaults)
    rec("ck", "one-launch")
    rec("rck", "one-launch")
    rec("cuts", node(1))  # slot 0 holds a checkpoint: several launches, an eager restore
    rec("ck", "several-launch")
    base = tall or "one-launch"
    rec("rck", base)
    grand = child_cuts(rec.run.raw, 1)[0]
    rec("from", base, [grand], True)
    rec("ck", "grandchild")
    # (a root whose spare rows the grandchild used up gets a deeper node without a cut: the call is made, not refused)
    deeper = child_cuts(rec.run.raw, 2)[1] if len(rec.run.raw["rows"]) < root["cap"] else []
    rec("restore")
    rec("ck", "restore")
    rec("addcuts", node(2))
    rec("ck", "add_cuts")
    rec("simplex")
    rec("ck", "simplex")
    A = rec.run.raw["A"]
    r, c = next((r, c) for r in range(1, A.shape[0]) for c in range(1, A.shape[1]) if abs(A[r, c]) > 0.5)
    rec("pivot", r, c)
    rec("ck", "pivot")
    taken += ["one-launch", "several-launch", "grandchild", "restore", "add_cuts", "simplex", "pivot"]
    rec("from", "grandchild", [deeper], True)  # an unrelated deeper node, then a batch, then every checkpoint back
    rec("batch", batch(16, 5))
    settle()
    for name in taken:
        rec("rck", name)
    tall = tall or "grandchild"
    # ---- children of a checkpoint that is taller than the root
    rec("rck", tall)
    h_tall = len(rec.run.raw["rows"])
    kids = child_cuts(rec.run.raw, 17)
    room = root["cap"] - h_tall
    rec("restore")
    rec("cuts", fam[-1] if len(fam[-1]) <= spare else node(0))  # the slot last held the tallest node of the family
    rec("from", tall, [kids[0]] if room >= 1 else [[]], True)
    if not opt and room >= 1:
        for count in (2, 3, 17):
            rec("from", tall, kids[:count], True)
            for k in range(count):  # every child against its single-call twin
                rec("from", tall, [kids[k]], count == 2)
        # the ENGINE's evaluation after several children is the last child's: an infeasible node reports the evaluation its call started from
        rec("from", tall, kids[:3], True)
        rec("cuts", fam[inf[0]])
    exact = [kids[i % len(kids)][0] for i in range(room)]
    rec("from", tall, [exact], True)  # the spare rows used up exactly
    assert rec("from", tall, [exact + [kids[0][0]]], True) == dict(error=_capi.JSLP_ERR_CAPACITY), root["name"]
    rec("from", tall, [kids[0]] if room >= 1 else [[]], True)
    # ---- back to the root after a checkpoint call
    rec("cuts", node(0))  # several launches once
    rec("cuts", node(1))  # the one-launch kernel again
    rec("batch", batch(16, 9))
    if big:
        rec("batch", big)
    settle()
    # ---- re-rooting: the checkpoint becomes the root; batches and checkpoints of the old root stay behind
    rec("rck", tall)
    rec("save")
    news = child_cuts(rec.run.raw, 6)
    outcomes = [rec("cuts", c) for c in news[:4]]
    good = [c for c, o in zip(news, outcomes) if "error" not in o and o["res"]["optimal"]]
    if good:
        rec("batch", [news[i % len(news)] for i in range(16)] + [good[0]])
        rec("cuts", good[0])
    rec("ck", "new root")
    for name in taken[:3]:
        rec("rel", name)
    for name in ("recycled 1", "recycled 2"):
        rec("ck", name)
    rec("from", "recycled 2", [child_cuts(rec.run.raw, 1)[0] if len(rec.run.raw["rows"]) < root["cap"] else []], True)
    rec("rck", "pivot")  # taken under the old root
    rec("cuts", news[0])
    rec("restore")
    rec("rck", "new root")
    rec("restore")
    rec("save")


def plan_walk(oracle_lib, name):
    t0 = time.time()
    root = N.plan_root(oracle_lib, root_spec(name))
    rec = Recorder(oracle_lib, root)
    try:
        build_walk(rec, root)
    finally:
        rec.run.close()
    keep = ("name", "rows", "cols", "cap", "A", "vibr", "vibc", "unr_list", "oo", "check", "H")
    return dict(root={k: root[k] for k in keep}, steps=rec.steps, obs=rec.obs, oracle_s=time.time() - t0)


# ---- k_mir_cuts on crafted uploads ---------------------------------------------------------------------------------------------------
PRECISION = 1e-8


def mir_case(name, H, W, cand, spare=None, seed=0, first_int=True, last_int=False, cells=None, rhs=None, near_n_idx=False, short=False):
    """an upload on which applyMIRCuts() cuts the rows `cand` (the first ten of them): integral column 0 with 0.25 / 0.75 planted on the
    candidates, whose basic variables are the integer ones; decoys have one of the two properties.  cells: {(row, col): value};
    rhs: {row: value}.  spare: rows beyond H (default: exactly the cuts); short: one row less than that"""
    rng = np.random.default_rng(7000 + seed)
    cuts = min(len(cand), 10)
    cap = H + (cuts if spare is None else spare) - (1 if short else 0)
    A = np.zeros((H, W))
    A[:, 1:] = rng.integers(-8, 9, (H, W - 1)) + rng.integers(0, 4, (H, W - 1)) * 0.25
    A[:, 0] = rng.integers(-40, 100, H)
    n_idx = W + 2 * cap + 2
    vibr = np.concatenate(([-1], np.arange(H - 1))).astype(np.int32)
    vibc = np.concatenate(([-1], H - 1 + np.arange(W - 1))).astype(np.int32)
    ints = set()
    for k, r in enumerate(cand):
        A[r, 0] += 0.25 if k % 2 == 0 else 0.75
        if near_n_idx:  # a slack index at the end of the index range as its basic variable
            vibr[r] = n_idx - 1 - k
        ints.add(int(vibr[r]))
    others = [r for r in range(1, H) if r not in set(cand)]
    for k, r in enumerate(others[:40]):
        if k % 2 == 0:
            ints.add(int(vibr[r]))  # integer variable, integral value
        else:
            A[r, 0] += 0.5  # fractional value, no integer variable
    for c in range(1, W):  # every third column an integer variable; the first and the last as the case says
        if {1: first_int, W - 1: last_int}.get(c, c % 3 == 0):
            ints.add(int(vibc[c]))
    for (r, c), v in (cells or {}).items():
        A[r, c] = v
    for r, v in (rhs or {}).items():
        A[r, 0] = v
    return dict(name=name, H=H, W=W, cap=cap, A=A, vibr=vibr, vibc=vibc, ints=sorted(ints), cand=list(cand), short=short)


def mir_cases():
    out = []
    add = out.append
    add(mir_case("no candidate", 300, 9, []))
    add(mir_case("row 1", 300, 9, [1]))
    add(mir_case("row H-1", 300, 9, [299]))
    add(mir_case("rows 255 256 257 258", 300, 9, [255, 256, 257, 258]))
    add(mir_case("exactly 10", 300, 9, list(range(20, 300, 28))[:10]))
    add(mir_case("11, the 10th at 256, the 11th at 257", 300, 9, [3, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257]))
    add(mir_case("9 in the first chunk, 3 in the second", 600, 9, [2, 30, 63, 64, 100, 128, 192, 250, 256, 257, 400, 513]))
    add(mir_case("12 inside one wave", 300, 9, list(range(70, 82))))
    add(mir_case("one per wave and chunk, H 1100", 1100, 9, sorted(1 + 256 * (k % 5) + 64 * (k % 4) + k for k in range(10))))
    add(mir_case("slack indexes near n_idx", 300, 9, [5, 256, 299], near_n_idx=True))
    add(mir_case("H 2", 2, 9, [1]))
    add(mir_case("H 2, no candidate", 2, 2, []))
    for W in (2, 9, 129, 256, 257, 1040):
        for first_int, last_int in ((True, False), (False, True)):
            add(mir_case("W %d first %d last %d" % (W, first_int, last_int), 40, W, [1, 17, 39], seed=W, first_int=first_int, last_int=last_int))
    # cell values on one source row (f = 0.25 on row 4): every kind in an integer and in a non-integer column (c % 3 == 0: integer)
    kinds = {"-0.0": -0.0, "NaN": float("nan"), "+Inf": float("inf"), "-Inf": float("-inf"), "negative non-integer": -2.6, "a - floor(a) == f": 3.25,
             "just under f": float(np.nextafter(3.25, 0.0)), "just over f": float(np.nextafter(3.25, 9.0))}
    for k, (label, v) in enumerate(kinds.items()):
        add(mir_case("cell " + label, 12, 9, [4], seed=50 + k, cells={(4, 3): v, (4, 4): v, (4, 1): v, (4, 8): v}))
    add(mir_case("cells of every kind on one row", 12, 33, [4, 9], seed=70, cells={(4, 1 + i): v for i, v in enumerate(list(kinds.values()) * 4)}))
    # right-hand sides: the variable of every listed row is an integer one, the value decides
    p = PRECISION
    # (f = rhs - floor(rhs) is exactly the value for 0 <= rhs < 1; 5 + precision and 6 - precision round on the way)
    edge = {"negative fractional": -7.25, "2^53": 2.0 ** 53, "precision": p, "below precision": float(np.nextafter(p, 0.0)),
            "above precision": float(np.nextafter(p, 1.0)), "1 - precision": 1.0 - p, "below 1 - precision": float(np.nextafter(1.0 - p, 0.0)),
            "above 1 - precision": float(np.nextafter(1.0 - p, 2.0)), "5 + precision": 5.0 + p, "6 - precision": 6.0 - p, "NaN": float("nan"),
            "+Inf": float("inf"), "-Inf": float("-inf"), "-0.0": -0.0, "-precision": -p}
    for k, (label, v) in enumerate(edge.items()):
        add(mir_case("rhs " + label, 12, 9, [6], seed=80 + k, rhs={6: v}, spare=2))
    add(mir_case("every rhs edge in one upload", 40, 17, list(range(2, 2 + len(edge))), seed=99, rhs={2 + i: v for i, v in enumerate(edge.values())}, spare=12))
    # capacity: exact passes (every case above with spare=None); one row short is refused, and the engine works after upload() again
    add(mir_case("one row short, 1 cut", 300, 9, [258], short=True))
    add(mir_case("one row short, 10 cuts", 300, 9, list(range(250, 262)), short=True))
    add(mir_case("no spare row, no candidate", 30, 9, [], spare=0))
    return out


def run_mir_case(lib, case):
    """-> observation: rows appended and the five arrays, or the error code; after an error the same engine once more after upload()"""
    t = Tableau(case["A"], case["vibr"], case["vibc"], precision=PRECISION, row_capacity=case["cap"], lib=lib, integer_variables=case["ints"])
    try:
        try:
            obs = dict(added=int(t.applyMIRCuts()), arrays=[pack(a) for a in t.download()], rhs=[pack(a) for a in t.read_rhs()])
        except _capi.EngineError as e:
            obs = dict(error=error_code(e))
            # the same engine after upload() again: the candidates that fit (the upload forgets the integer variables: said again)
            A = case["A"].copy()
            for r in case["cand"][max(min(len(case["cand"]), 10) - 1, 0):]:
                A[r, 0] = np.floor(A[r, 0])
            t.upload(A, case["vibr"], case["vibc"])
            iv = _capi.as_i32(case["ints"])
            lib.check(lib.jslp_engine_set_integer_variables(t._h, _capi.ptr_i32(iv), int(iv.shape[0])), "jslp_engine_set_integer_variables")
            obs["again"] = dict(added=int(t.applyMIRCuts()), arrays=[pack(a) for a in t.download()])
        return obs
    finally:
        t.close()


# ---- the plan: computed once on the oracle, shared by every test, never changed ---------------------------------------------------------
_PLAN = {}


def plan(oracle_lib):
    if not _PLAN:
        t0 = time.time()
        walks = {name: plan_walk(oracle_lib, name) for name in ROOT_NAMES}
        cases = mir_cases()
        _PLAN.update(walks=walks, mir=[dict(case, want=run_mir_case(oracle_lib, case)) for case in cases], seconds=time.time() - t0)
    return _PLAN


def test_roots_and_settings_are_what_the_docstring_says():
    assert set(LARGE_ROOTS) <= set(ROOT_NAMES) and set(SP_ROOTS) == {n for n in ROOT_NAMES if "2x2" in n or "7x6" in n or "41x15" in n or "258x15" in n}
    for name in ROOT_NAMES:
        s = root_spec(name)
        assert s["name"] == name
    assert [queue_sized(root_spec(n)) for n in ("H 2049x15", "fit 2590x15 cap 2610", "cells 15x1040 cap 4100")] == [True, False, False]
    names = [c["name"] for c in mir_cases()]
    assert len(set(names)) == len(names)
    for c in mir_cases():
        assert c["cap"] >= c["H"] and all(0 <= v < c["W"] + 2 * c["cap"] + 2 for v in c["ints"]), c["name"]


def _steps(walk, op):
    return [(s, o) for s, o in zip(walk["steps"], walk["obs"]) if s[0] == op]


def test_walks_on_the_oracle(oracle_lib):
    """the vacuity guards of every walk, and what must hold on the reference itself: a restored checkpoint is the tableau it was taken
    from, the children of a multi-child call are their single-call twins, and its live tableau is the LAST child's"""
    p = plan(oracle_lib)
    for name, walk in p["walks"].items():
        steps, obs, root = walk["steps"], walk["obs"], walk["root"]
        cuts = [o for s, o in _steps(walk, "cuts") if "error" not in o]
        assert any(o["res"]["optimal"] and o["res"]["pivots_phase1"] + max(o["res"]["pivots_phase2"], 0) > 0 for o in cuts), (name, "no node pivots")
        assert any(not o["res"]["feasible"] for o in cuts), (name, "no node is infeasible")
        assert sum(1 for s, o in _steps(walk, "cuts") if "error" in o) == 2, name
        mir = [o for s, o in _steps(walk, "mir") if "error" not in o]
        assert any(o["added"] >= 1 and o["res"]["pivots_phase1"] + max(o["res"]["pivots_phase2"], 0) > 0 for o in mir), (name, "no MIR round adds a row and pivots")
        taken = {s[1]: o for s, o in _steps(walk, "ck")}
        assert any(o["live"]["height"] > root["H"] for o in taken.values()), (name, "no checkpoint is taller than the root")
        assert {"mir", "one-launch", "several-launch", "grandchild", "restore", "add_cuts", "simplex", "pivot", "new root"} <= set(taken), (name, sorted(taken))
        for s, o in _steps(walk, "batch"):
            assert "error" not in o and o["last_optimal"], (name, "a batch must end on a node with an optimum")
        # every checkpoint that is restored gives back what was observed when it was taken (the optional objectives are not part of it)
        latest, restored = {}, 0
        for s, o in zip(steps, obs):
            if s[0] == "ck":
                latest[s[1]] = o["live"]
            elif s[0] == "rck":
                restored += 1
                for key in LIVE[2:-1]:
                    assert o["live"][key] == latest[s[1]][key], (name, "restoreCheckpoint", s[1], key)
        assert restored >= len(taken) - 3, name
        # multi-child calls: outcomes of the twins, the live tableau of the last, and children that differ
        froms = [(i, s, o) for i, (s, o) in enumerate(zip(steps, obs)) if s[0] == "from" and "error" not in o]
        multi = [(i, s, o) for i, s, o in froms if len(s[2]) > 1]
        # one call from a checkpoint is refused (one cut too many), no other: the deeper node and the child of the recycled checkpoint are evaluated
        assert [o for s, o in zip(steps, obs) if s[0] == "from" and "error" in o] == [dict(error=_capi.JSLP_ERR_CAPACITY)], name
        assert any(s[:2] == ("from", "grandchild") for s in steps) and any(s[:2] == ("from", "recycled 2") for s in steps), name
        for i, o in enumerate(obs[:-1]):  # a refused call leaves the live tableau unspecified: the next step is defined whatever it holds
            assert "error" not in o or steps[i + 1][0] in ("cuts", "batch", "restore", "rck", "from"), (name, i, steps[i + 1][0])
        if root["oo"] is not None:
            assert not multi, name
            for i, s in enumerate(steps[:-1]):  # the optional objectives after a batch are those of an unspecified node
                assert s[0] != "batch" or steps[i + 1][0] in ("cuts", "restore", "batch"), (name, i, steps[i + 1][0])
            continue
        assert [len(s[2]) for _, s, _ in multi] == [2, 3, 17, 3], name
        after = obs[multi[3][0] + 1]  # the node that reports the engine's evaluation after a multi-child call
        assert steps[multi[3][0] + 1][0] == "cuts" and not after["res"]["feasible"] and after["res"]["bounded"] and not after["res"]["optimal"], name
        for i, s, o in multi[:3]:
            twins = obs[i + 1:i + 1 + len(s[2])]
            assert [t["nodes"][0] for t in twins] == o["nodes"], (name, "children and their single-call twins")
            assert o["res"] == twins[-1]["res"]
            if len(s[2]) == 2:
                assert twins[0]["live"]["A"] != twins[1]["live"]["A"], (name, "the two children leave the same tableau")
                assert o["live"] == twins[1]["live"], (name, "the oracle's live tableau is not the LAST child's")
    slow = {n: round(w["oracle_s"], 2) for n, w in p["walks"].items() if w["oracle_s"] > 0.3}
    print("oracle plan: %.2f s; walks over 0.3 s: %s; steps %s" % (p["seconds"], slow, {n: len(w["steps"]) for n, w in p["walks"].items()}))
    assert p["seconds"] < 30, p["seconds"]


def test_mir_cases_on_the_oracle(oracle_lib):
    """the crafted uploads do what their names say on the reference: the rows that get a cut, the limit of ten, the capacity codes"""
    cases = {c["name"]: c for c in plan(oracle_lib)["mir"]}
    for name, c in cases.items():
        want = c["want"]
        if c["short"]:
            assert want["error"] == _capi.JSLP_ERR_CAPACITY and want["again"]["added"] == min(len(c["cand"]), 10) - 1, name
        elif name.startswith(("rhs ", "every rhs")):
            assert "error" not in want, name
        else:
            assert want.get("added") == min(len(c["cand"]), 10), (name, want.get("added"), want.get("error"))
    added = {n: c["want"]["added"] for n, c in cases.items() if n.startswith("rhs ")}
    # f < precision and f > 1 - precision give no cut, the thresholds themselves and what lies between do (cutting-strategies.ts:88-90)
    assert (added["rhs below precision"], added["rhs precision"], added["rhs above precision"]) == (0, 1, 1), added
    assert (added["rhs below 1 - precision"], added["rhs 1 - precision"], added["rhs above 1 - precision"]) == (1, 1, 0), added
    assert added["rhs negative fractional"] == 1 and added["rhs 2^53"] == 0 and added["rhs -0.0"] == 0, added
    assert cases["every rhs edge in one upload"]["want"]["added"] == min(10, sum(added.values())), added


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_file(oracle_lib, tmp_path_factory):
    path = tmp_path_factory.mktemp("live_tableau") / "plan.pkl"
    with open(path, "wb") as fh:
        pickle.dump(plan(oracle_lib), fh, protocol=pickle.HIGHEST_PROTOCOL)
    return str(path)


def _worker(plan_file, mode, extra, names, timeout):
    env = {k: v for k, v in os.environ.items() if k not in N.KNOBS}
    env.update(extra)
    env["JSLP_DEBUG_LAUNCH"] = "1"
    try:
        out = subprocess.run([sys.executable, WORKER, mode, plan_file, "\n".join(names)], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        pytest.exit("the live-tableau worker hung (%s): nothing more is started on this GPU" % extra, returncode=3)
    print(out.stdout[-8000:])
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):  # killed by a signal: a fault, not a wrong answer
        pytest.exit("the live-tableau worker died with %d (%s): nothing more is started on this GPU\n%s" % (out.returncode, extra, out.stdout[-3000:]), returncode=3)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-6000:] + out.stderr[-3000:]
    return out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_walks_on_the_gpu(hip_lib, plan_file, setting):
    """every step of every walk of the setting's roots: outcomes, the whole live state and the launch lines.  The live tableau after
    jslp_engine_relax_from with several children is the LAST child's (the `from` steps with 2, 3 and 17 cut lists): with the final child
    evaluated in whatever slot its position in the group gives it, this test fails at the first two-child call of the first root."""
    names = roots_of(setting)
    out = _worker(plan_file, "walks", SETTINGS[setting], names, 300)
    assert out.count("walk ok") == len(names)
    if setting == "defaults":
        assert "k_node_lds<1024,opt 0,cow 1>" in out and "k_node_queue<512,cow 1,opt 0>" in out and "k_node_wg<1024,4096>" in out and "chip-wide" in out
    if setting == "sp":
        assert "k_node_" not in out and "k_simplex_" not in out


@pytest.mark.gpu
def test_mir_cuts_kernel_on_crafted_uploads(hip_lib, plan_file):
    out = _worker(plan_file, "mir", {}, [], 300)
    assert out.count("mir ok") == len(mir_cases())
