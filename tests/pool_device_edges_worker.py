"""Body of tests/test_pool_device_edges.py: the device pool (run_pool) and the `_device` entry points (run_device) at the node edges,
every outcome held to the plan the parent computed on the CPU oracle.  As a subprocess (main) it drives the HIP library, "device"
memory being a torch.uint8 tensor on the GPU; imported by the parent it drives the oracle library with numpy memory (the CPU twin):
the allocator is the only thing that differs.  share_bounds() and pool_stride() restate how the pool splits a batch and lays out its
shared buffer; the parent swaps each for a wrong one to prove that the comparisons notice."""
import os
import pickle
import re
import sys
import traceback
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jslpsolver_amd import _capi  # noqa: E402
from jslpsolver_amd.engine import DevicePool, branch_record_from_watched  # noqa: E402
import test_node_edges as N  # noqa: E402

RESULT_DTYPE = np.dtype([(name, np.int32 if ctype is _capi.C.c_int32 else np.float64) for name, ctype in _capi.SimplexResult._fields_])
assert RESULT_DTYPE.itemsize == _capi.C.sizeof(_capi.SimplexResult)
FIELDS = ("feasible", "bounded", "optimal", "height", "pivots_phase1", "pivots_phase2", "cycle_phase")
FLAVOURS = ("full copy", "full pinned", "watched copy", "watched pinned")
FILL, GUARD, ALIGN = 0xA5, 4096, 256
FILL64, FILL32 = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint32(0xA5A5A5A5)
LINE = re.compile(r"^\[jslp\] launch (.+?) g (\d+)", re.M)
BIG_WATCHED = "H 2049x15"  # the root whose `_device` calls watch more than 1024 variables


def share_bounds(n, M):
    """[first, last) of every member's share of n nodes (pool_relax: first = n * mi / M)"""
    return [(n * mi // M, n * (mi + 1) // M) for mi in range(M)]


def pool_stride(cap):
    """entries per node in the pool's shared pinned buffer: the plain row capacity"""
    return cap


def window(n, start, size):
    return [(start + i) % n for i in range(size)]


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compact_of(w, watched):
    """the compact read-back of an outcome: per watched variable its row (-1: not basic) and its RHS cell"""
    rows = np.frombuffer(w["rows"], dtype=np.int32)
    rhs = np.frombuffer(w["rhs"], dtype=np.float64)
    row_of = {int(v): r for r, v in enumerate(rows) if r > 0}
    r = np.array([row_of.get(v, -1) for v in watched], dtype=np.int32)
    return r, np.where(r > 0, rhs[np.maximum(r, 0)], 0.0)


def node_slices(a, n, stride, width):
    """[n, width]: the first `width` entries of n node slices that lie `stride` entries apart in the buffer behind `a`"""
    if a.ndim == 2 and a.shape[1] == stride:
        return a[:n, :width]
    flat = a.reshape(-1)
    idx = np.arange(n, dtype=np.int64)[:, None] * stride + np.arange(width, dtype=np.int64)[None, :]
    return flat[np.minimum(idx, flat.size - 1)]


def as_results(res, n):
    arr = res if isinstance(res, _capi.C.Array) else res[0]._b_base_
    return np.frombuffer(arr, dtype=RESULT_DTYPE, count=n)


class Want:
    """the oracle's outcome of every node of a list, as arrays a whole batch is compared with at once"""

    def __init__(self, name, want, cap, watched, precision):
        n, nw = len(want), len(watched)
        self.name, self.cap, self.watched, self.precision, self.want = name, cap, list(watched), precision, want
        self.res = np.zeros(n, dtype=RESULT_DTYPE)
        self.rhs = np.zeros((n, cap), dtype=np.uint64)
        self.rows = np.zeros((n, cap), dtype=np.int32)
        self.valid = np.zeros((n, cap), dtype=bool)
        self.wrows = np.zeros((n, nw), dtype=np.int32)
        self.wvals = np.zeros((n, nw), dtype=np.uint64)
        for k, w in enumerate(want):
            h = w["height"]
            self.res[k] = (w["feasible"], w["bounded"], w["optimal"], w["unbounded_var"], w["p1"], w["p2"], w["cycle"], 0, 0, h, w["obj_cell"], w["evaluation"])
            self.rhs[k, :h] = np.frombuffer(w["rhs"], dtype=np.uint64)
            self.rows[k, :h] = np.frombuffer(w["rows"], dtype=np.int32)
            self.valid[k, :h] = True
            r, v = compact_of(w, self.watched)
            self.wrows[k], self.wvals[k] = r, bits64(v)
        self.pivots = self.res["pivots_phase1"].astype(np.int64) + np.maximum(self.res["pivots_phase2"], 0)
        self._records = None

    def expected_eval(self, ks, prev):
        """optimal: the node's own; unbounded: -Infinity; else what its engine had when the call began (`prev`, per node)"""
        w = self.res[ks]
        return np.where(w["optimal"] != 0, w["evaluation"], np.where(w["bounded"] == 0, -np.inf, prev))

    def check_results(self, got, ks, prev, what, pivots=True):
        w = self.res[ks]
        for f in FIELDS:
            if not pivots and f.startswith(("pivots", "cycle")):
                continue
            bad = np.nonzero(got[f] != w[f])[0]
            assert bad.size == 0, (self.name, what, f, "node", int(bad[0]), "of", len(ks), int(got[f][bad[0]]), int(w[f][bad[0]]))
        bad = np.nonzero(bits64(got["obj_cell"]) != bits64(w["obj_cell"]))[0]
        assert bad.size == 0, (self.name, what, "objective cell", "node", int(bad[0]))
        exp = self.expected_eval(ks, prev)
        bad = np.nonzero(bits64(got["evaluation"]) != bits64(exp))[0]
        assert bad.size == 0, (self.name, what, "evaluation", "node", int(bad[0]), "of", len(ks), float(got["evaluation"][bad[0]]), float(exp[bad[0]]))
        return exp

    def check_full(self, rhs, rows, ks, stride, what):
        n, valid = len(ks), self.valid[ks]
        for got, exp, label in ((node_slices(rhs, n, stride, self.cap).view(np.uint64), self.rhs[ks], "RHS column"),
                                (node_slices(rows, n, stride, self.cap), self.rows[ks], "row map")):
            bad = np.nonzero(((got != exp) & valid).any(axis=1))[0]
            assert bad.size == 0, (self.name, what, label, "node", int(bad[0]), "of", n, "stride", stride)

    def check_compact(self, wrows, wvals, ks, what):
        n = len(ks)
        bad = np.nonzero((np.asarray(wrows)[:n] != self.wrows[ks]).any(axis=1))[0]
        assert bad.size == 0, (self.name, what, "watched rows", "node", int(bad[0]), "of", n)
        bad = np.nonzero((np.asarray(wvals)[:n].view(np.uint64) != self.wvals[ks]).any(axis=1))[0]
        assert bad.size == 0, (self.name, what, "watched values", "node", int(bad[0]), "of", n)

    def records(self):
        """the branch record of every node, restated from its compact read-back (engine.branch_record_from_watched)"""
        if self._records is None:
            fakes = [types.SimpleNamespace(feasible=w["feasible"], bounded=w["bounded"], optimal=w["optimal"], height=w["height"],
                                           unbounded_var_index=w["unbounded_var"], obj_cell=w["obj_cell"]) for w in self.want]
            self._records = branch_record_from_watched(fakes, self.wrows, self.wvals.view(np.float64), self.watched, self.precision)
        return self._records


class Stderr:
    """this process's stderr (the engine's fprintf included) in a file; kernels() names the node launches since the last look"""

    def __init__(self, path):
        self.out = open(path, "wb")
        os.dup2(self.out.fileno(), 2)
        self.inp = open(path, "rb")
        self.path = path

    def kernels(self):
        sys.stderr.flush()
        text = self.inp.read().decode(errors="replace")
        return {m.group(1) for m in LINE.finditer(text) if m.group(1).startswith(("k_node_", "restore+"))}


def solved_root(lib, root):
    t = N.tableau(lib, root)
    res = t.simplex(check_cycles=root["check"])
    assert res.feasible and res.bounded and res.optimal, root["name"]
    rhs, rows = t.read_rhs()
    assert rhs.tobytes() == root["root_rhs"] and rows.tobytes() == root["root_rows"], (root["name"], "the root itself differs")
    assert bits64(t.evaluation) == bits64(root["root_eval"]), root["name"]
    t.save()
    return t


def watched_with_dup(root):
    """the root's watched list (every variable a family cuts on and the structural ones: non-basic in some nodes), two of them twice"""
    w = list(root["watched"])
    return w + [w[len(w) // 2], w[0]]


def error_text(exc):
    return str(exc).split("): ", 1)[1]


# ---- part 1: the pool -------------------------------------------------------------------------------------------------------------
class PoolRun:
    def __init__(self, lib, root, M, cov):
        self.root, self.M, self.cov, self.name = root, M, cov, root["name"]
        self.t = solved_root(lib, root)
        self.pool = DevicePool(self.t, [0] * M)
        assert self.pool.size == M
        self.watched = watched_with_dup(root)
        self.pool.set_watched_variables(self.watched)  # (fans the root out: every member starts from the primary's evaluation)
        self.ev = [root["root_eval"]] * M  # per member: what a node without an optimum reports
        self.fam = root["family"]
        self.W = Want(self.name, root["want"], root["cap"], self.watched, self.t.precision)
        self.packed = {}
        self.calls = 0

    def close(self):
        self.pool.close()
        self.t.close()

    def pack(self, nodes, key):
        if key not in self.packed:
            self.packed[key] = self.t.pack_cut_lists(nodes)
        return self.packed[key]

    def launch(self, pk, flavour):
        full, copy = flavour.startswith("full"), flavour.endswith("copy")
        self.calls += 1
        if full:
            return self.pool.applyCutsBatch(None, check_cycles=True, packed=pk, copy=copy)
        return self.pool.applyCutsBatchWatched(None, check_cycles=True, packed=pk, copy=copy)

    def prev_of(self, n):
        prev = np.empty(n, dtype=np.float64)
        for mi, (a, b) in enumerate(share_bounds(n, self.M)):
            prev[a:min(b, n)] = self.ev[mi]
        return prev

    def move(self, n, exp, failed=()):
        for mi, (a, b) in enumerate(share_bounds(n, self.M)):
            if min(b, n) > a and mi not in failed:
                self.ev[mi] = float(exp[min(b, n) - 1])

    def call(self, ks, flavour, W=None, fam=None, tag="family"):
        W, fam = W or self.W, fam or self.fam
        n, what = len(ks), "pool of %d, %s, %d nodes (%s)" % (self.M, flavour, len(ks), tag)
        res, a, b = self.launch(self.pack([fam[k] for k in ks], (tag, tuple(ks) if n <= len(fam) else (ks[0], n))), flavour)
        if n == 0:
            return
        ks = np.asarray(ks)
        exp = W.check_results(as_results(res, n), ks, self.prev_of(n), what)
        cap = self.root["cap"]
        if flavour.startswith("full"):
            stride = pool_stride(cap) if flavour == "full pinned" else a.shape[1]
            W.check_full(a, b, ks, stride, what)
            assert a.shape[1] == b.shape[1] == cap, (self.name, what, "out_stride", a.shape)
        else:
            W.check_compact(a, b, ks, what)
        self.move(n, exp)
        self.cov |= {(cap % 4, int(h), flavour) for h in np.unique(W.res["height"][ks] % 2)}

    def refused(self, ks, plants, flavour, code, text, texts):
        """plants: {position in the batch: (label, cuts, code)}; the call fails with `code` and the text the list `text` is refused with"""
        nodes = [self.fam[k] for k in ks]
        for at, (label, cuts, _) in plants.items():
            nodes[at] = cuts
        n, what = len(ks), "pool of %d, %s, refused %s" % (self.M, flavour, sorted((at, p[0]) for at, p in plants.items()))
        shares = share_bounds(n, self.M)
        failed = {mi for mi, (a, b) in enumerate(shares) for at in plants if a <= at < b}
        try:
            self.launch(self.t.pack_cut_lists(nodes), flavour)
        except _capi.EngineError as e:
            assert N.error_code(e) == code, (self.name, what, str(e), code)
            got = error_text(e)
            assert texts.setdefault(text, got) == got, (self.name, what, "the text of the lowest failing member", got, texts[text])
        else:
            raise AssertionError((self.name, what, "no error"))
        self.move(n, self.W.expected_eval(np.asarray(ks), self.prev_of(n)), failed)  # a refused share leaves its member's evaluation alone


def run_pool(lib, root, M, cov, sizes=None):
    """one pool of M members on one root: every batch size in every read-back flavour, twice; counters; refused lists; new roots"""
    r = PoolRun(lib, root, M, cov)
    try:
        nf = len(r.fam)
        big = nf * (256 * M // nf + 1)  # one member's share passes 256 nodes
        start = 0
        for n in sizes if sizes is not None else sorted({0, 1, M - 1, M, M + 1, 2 * M + 1, nf, big}):
            ks = window(nf, start, n) if n <= nf else list(range(nf)) * (n // nf)
            start += 3
            for flavour in FLAVOURS:
                r.call(ks, flavour)
                r.call(ks, flavour)  # (the one-launch shape in every member)
        if sizes is not None:
            return r.calls
        # counters
        ks = window(nf, 1, nf)
        r.pool.set_counting(True)
        r.call(ks, "full copy")
        c = r.pool.get_counters()
        r.pool.set_counting(False)
        assert c["relaxations"] == nf and c["pivots"] == int(r.W.pivots.sum()), (r.name, M, c["relaxations"], c["pivots"], nf, int(r.W.pivots.sum()))
        # refused cut lists: in member 0's share, in the last member's, in two members' at once (the lower one decides)
        if r.name in N.ERROR_ROOTS:
            n = 2 * M + 1
            shares = share_bounds(n, M)
            mid = [(a + b) // 2 for a, b in shares]
            bad = {b[0]: b for b in root["bad"]}
            texts, count = {}, 0
            for label, b in bad.items():
                other = bad["negative index" if label == "spare + 1 cuts" else "spare + 1 cuts"]  # (another code and another text)
                plans = [{mid[0]: b}] + ([{mid[-1]: b}, {mid[0]: b, mid[-1]: other}] if M > 1 else []) + ([{mid[1]: b, mid[-1]: other}] if M > 2 else [])
                for plants in plans:
                    flavour = FLAVOURS[count % 4]
                    ks = window(nf, count, n)
                    r.call(ks, flavour)
                    r.call(ks, flavour)
                    r.refused(ks, plants, flavour, b[2], label, texts)
                    r.call(ks, flavour)  # one launch in the members whose share was clean, the eager sequence in the others
                    r.call(ks, flavour)  # one launch in every member
                    count += 1
        # a new root: the primary saves after a relaxation grew its tableau and it was handed other optional objectives; the next
        # call fans both out by itself, and every member starts from the primary's evaluation again
        nr = root["new_root"]
        r.t.applyCuts(r.fam[nr["k"]], check_cycles=True)
        oo = np.ascontiguousarray(nr["oo"], dtype=np.float64)
        lib.check(lib.jslp_engine_set_optional_objectives(r.t._h, int(oo.shape[0]), _capi.ptr_f64(oo)), "jslp_engine_set_optional_objectives")
        r.t.save()
        r.ev = [nr["eval"]] * M
        W2 = Want(r.name + " (new root)", nr["want"], root["cap"], r.watched, r.t.precision)
        n2 = len(nr["family"])
        for n in sorted({1, M + 1, n2, 3 * n2}):
            ks = window(n2, n, n)
            for flavour in FLAVOURS:
                r.call(ks, flavour, W2, nr["family"], "new root")
                r.call(ks, flavour, W2, nr["family"], "new root")
        return r.calls
    finally:
        r.close()


# ---- part 2: the _device entry points ---------------------------------------------------------------------------------------------
class NumpyMemory:
    """"device" memory of the oracle library: host memory, its base on a 256-byte boundary"""

    def __init__(self, nbytes):
        self.raw = np.empty(nbytes + ALIGN, dtype=np.uint8)
        o = (-self.raw.ctypes.data) % ALIGN
        self.a = self.raw[o:o + nbytes]
        self.ptr = self.a.ctypes.data

    def fill(self):
        self.a.fill(FILL)

    def host(self):
        return self.a.copy()


class TorchMemory:
    """memory of the engine's device: one torch.uint8 tensor"""

    def __init__(self, nbytes):
        import torch
        self.torch = torch
        self.a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.ptr = self.a.data_ptr()

    def fill(self):
        self.a.fill_(FILL)
        self.torch.cuda.current_stream().synchronize()  # the fill runs on torch's stream, the engine's kernels on the engine's own

    def host(self):
        return self.a.cpu().numpy()


class Regions:
    """one buffer: a 4 KiB guard, then per region its bytes (from a multiple of 256) and another guard; all of it pre-filled"""

    def __init__(self, memory, sizes):
        self.sizes, self.offs, off = list(sizes), [], GUARD
        for s in sizes:
            self.offs.append(off)
            off += (s + ALIGN - 1) // ALIGN * ALIGN + GUARD
        self.total = off
        self.mem = memory(off)
        assert self.mem.ptr % ALIGN == 0
        self.mem.fill()

    def ptr(self, i):
        return self.mem.ptr + self.offs[i]

    def read(self, what):
        """the regions' bytes; every byte outside them must still hold the fill"""
        h = self.mem.host()
        outside = np.ones(self.total, dtype=bool)
        for o, s in zip(self.offs, self.sizes):
            outside[o:o + s] = False
        assert (h[outside] == FILL).all(), (what, "a guard zone was written", int(np.nonzero(outside & (h != FILL))[0][0]), self.offs, self.sizes)
        return [h[o:o + s] for o, s in zip(self.offs, self.sizes)]


class DeviceRun:
    def __init__(self, lib, root, memory, strides_seen):
        self.lib, self.root, self.memory, self.name, self.seen = lib, root, memory, root["name"], strides_seen
        self.t = solved_root(lib, root)
        self.watched = watched_with_dup(root)
        if self.name == BIG_WATCHED:  # more watched variables than the widest block has threads
            self.watched += list(range(1100))
        self.t.set_watched_variables(self.watched)
        self.nw = len(self.watched)
        self.eval = root["root_eval"]
        self.fam, self.cap = root["family"], root["cap"]
        self.W = Want(self.name, root["want"], self.cap, self.watched, self.t.precision)
        self.rec = self.t.state_record_bytes()
        self.calls = 0

    def close(self):
        self.t.close()

    def sizes(self, n, kind, stride):
        if kind == "full":
            return [n * self.rec, n * stride * 8, n * stride * 4]
        if kind == "watched":
            return [n * self.rec, n * self.nw * 4, n * self.nw * 8]
        return [n * _capi.BRANCH_RECORD_DTYPE.itemsize]

    def launch(self, nodes, kind, stride):
        pk = self.t.pack_cut_lists(nodes)
        buf = Regions(self.memory, self.sizes(len(nodes), kind, stride))
        self.calls += 1
        if kind == "full":
            self.t.applyCutsBatchDevice(pk, True, buf.ptr(0), buf.ptr(1), buf.ptr(2), stride)
        elif kind == "watched":
            self.t.applyCutsBatchWatchedDevice(pk, True, buf.ptr(0), buf.ptr(1), buf.ptr(2))
        else:
            self.t.applyCutsBatchBranchDevice(pk, True, buf.ptr(0))
        return buf

    def call(self, ks, kind, stride=0):
        """kind: full (at row_stride `stride`) | watched | branch"""
        n, what = len(ks), "%s_device, %d nodes%s" % (kind, len(ks), ", row_stride %d" % stride if kind == "full" else "")
        buf = self.launch([self.fam[k] for k in ks], kind, stride)
        parts = buf.read((self.name, what))
        ks, prev, W = np.asarray(ks), np.full(n, self.eval), self.W
        if kind == "branch":
            recs = parts[0].view(_capi.BRANCH_RECORD_DTYPE)
            exp = W.check_results(as_results(self.t.results_from_branch_records(recs, n), n), ks, prev, what, pivots=False)
            bad = np.nonzero((recs.view(np.int64).reshape(n, -1) != W.records()[ks].view(np.int64).reshape(n, -1)).any(axis=1))[0]
            assert bad.size == 0, (self.name, what, "branch record", "node", int(bad[0]), recs[bad[0]], W.records()[ks][bad[0]])
        else:
            exp = W.check_results(as_results(self.t.results_from_states(parts[0], n), n), ks, prev, what)
        if kind == "watched":
            W.check_compact(parts[1].view(np.int32).reshape(n, self.nw), parts[2].view(np.float64).reshape(n, self.nw), ks, what)
        if kind == "full":
            rhs, rows = parts[1].view(np.float64).reshape(n, stride), parts[2].view(np.int32).reshape(n, stride)
            W.check_full(rhs, rows, ks, stride, what)
            # beyond height + (height & 1) entries a node's slice still holds the fill: the 16-byte stores may pad an odd height by one
            h = W.res["height"][ks].astype(np.int64)
            beyond = np.arange(stride)[None, :] >= (h + (h & 1))[:, None]
            assert (rhs.view(np.uint64)[beyond] == FILL64).all(), (self.name, what, "RHS column written beyond the padded height")
            assert (rows.view(np.uint32)[beyond] == FILL32).all(), (self.name, what, "row map written beyond the padded height")
            self.seen.add((self.name, "vector" if stride % 4 == 0 else "scalar"))
        self.eval = float(exp[-1])

    def host(self, ks):
        """a host call between `_device` calls on the same engine"""
        n, what = len(ks), "host batch of %d between _device calls" % len(ks)
        self.calls += 1
        res, rhs, rows = self.t.applyCutsBatch([self.fam[k] for k in ks], check_cycles=True, copy=False)
        ks = np.asarray(ks)
        exp = self.W.check_results(as_results(res, n), ks, np.full(n, self.eval), what)
        self.W.check_full(rhs, rows, ks, rhs.shape[1], what)
        self.eval = float(exp[-1])

    def refused(self, ks, at, bad, kind, stride):
        nodes = [self.fam[k] for k in ks]
        nodes[at] = bad[1]
        try:
            self.launch(nodes, kind, stride)
        except _capi.EngineError as e:
            assert N.error_code(e) == bad[2], (self.name, kind, bad[0], str(e))
        else:
            raise AssertionError((self.name, kind, bad[0], "no error"))


def run_device(lib, root, memory, seen, batches_only=False):
    r = DeviceRun(lib, root, memory, seen)
    try:
        nf, cap = len(r.fam), r.cap
        sizes = [2, nf] if batches_only else [1, 2, nf]
        start = 0
        for stride in sorted({cap, cap + 1, cap + 2, cap + 3, (cap + 3) & ~3}):
            for n in sizes:
                ks = window(nf, start, n)
                start += 5
                r.call(ks, "full", stride)
                r.call(ks, "full", stride)  # (the one-launch shape)
        for kind in ("watched", "branch"):
            for n in sizes:
                ks = window(nf, start, n)
                start += 5
                r.call(ks, kind)
                r.call(ks, kind)
        # _device and host calls on one engine, turn by turn: each starts from the evaluation the last one left
        n = min(nf, 8)
        for i, stride in enumerate((cap, cap + 1, (cap + 3) & ~3)):
            r.call(window(nf, i, n), "full", stride)
            r.host(window(nf, i + 2, n))
            r.call(window(nf, i + 4, n), "watched")
            r.host(window(nf, i + 1, n))
            r.call(window(nf, i + 3, n), "branch")
        if r.name in N.ERROR_ROOTS:  # a refused list in a `_device` call, then the batch that would be one launch had the slots stayed in sync
            count = 0
            for bad in root["bad"]:
                for kind, stride in (("full", cap), ("full", cap + 1), ("watched", 0), ("branch", 0)):
                    ks = window(nf, count, n)
                    r.call(ks, kind, stride)
                    r.call(ks, kind, stride)
                    r.refused(ks, (count * 3) % n, bad, kind, stride)
                    r.call(ks, kind, stride)
                    r.call(ks, kind, stride)
                    count += 1
        return r.calls
    finally:
        r.close()


def run(lib, plan, pool_names, device_names, Ms, memory, err=None, log=print):
    """both parts on the named roots -> (the (cap % 4, height % 2, flavour) the pool part compared, the (root, gather branch) of part 2)"""
    cov, seen = set(), set()
    for name in pool_names:
        calls = sum(run_pool(lib, plan[name], M, cov) for M in Ms)
        log("root ok | pool | %s | %d calls | %s" % (name, calls, " ; ".join(sorted(err.kernels())) if err else ""))
    for name in device_names:
        calls = run_device(lib, plan[name], memory, seen, batches_only=name not in pool_names)
        log("root ok | device | %s | %d calls | %s" % (name, calls, " ; ".join(sorted(err.kernels())) if err else ""))
    log("compared | pool | %r" % sorted(cov))
    log("compared | device | %r" % sorted(seen))
    return cov, seen


def main():
    plan_file, pool_names, device_names, Ms = sys.argv[1], sys.argv[2].split("\n"), sys.argv[3].split("\n"), [int(m) for m in sys.argv[4].split(",")]
    err = Stderr(plan_file + ".stderr.%d" % os.getpid())
    try:
        with open(plan_file, "rb") as fh:
            plan = pickle.load(fh)
        import torch
        torch.cuda.init()  # (before the engine's library: torch initialises HIP itself)
        hip = _capi.load_hip()
        run(hip, plan, [n for n in pool_names if n], [n for n in device_names if n], Ms, TorchMemory, err, lambda s: print(s, flush=True))
        print("ok", flush=True)
    except BaseException:
        print(traceback.format_exc(), flush=True)
        err.out.flush()
        with open(err.path, "rb") as fh:
            print("---- stderr ----\n" + fh.read().decode(errors="replace")[-3000:], flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
