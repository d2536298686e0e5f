"""The pack's host logic on the CPU: engine.TableauPack and solver.solve_packed through the RESTATED pack (one oracle engine per LP behind
the pack's interface), against Solve and against single engines that never saw a pack."""
import gzip
import json
import os

import numpy as np
import pytest

import golden_util as G
from jslpsolver_amd import Solve, UnsupportedModel, _capi, solve_packed
from jslpsolver_amd.engine import Tableau, TableauPack, pack_fits
from jslpsolver_amd.model import Model
from test_cycle_goldens import _instance, _messages


def _models():
    out = []
    for path in G.fixture_paths():
        g = G.load(path)
        if g["model"] is not None:
            out.append((G.ident(path), g["model"]))
    return out


def _packs(model):
    m = Model(model, None)
    matrix, _, _ = m.build_tableau()
    _, oo = m.optional_objectives()
    return len(m.integerVariables) == 0 and (oo is None or len(oo) == 0) and pack_fits(*matrix.shape)


def test_solve_packed_equals_solve_on_every_fixture(oracle_lib):
    """all 47 fixtures in one call, with duplicates: models that pack next to models that do not -- integer variables, optional
    objectives, and Sudoku4x4, whose tableau is beyond the LDS limit -- in their order"""
    named = _models()
    assert len(named) == 47
    named = named + named[:3]
    kinds = {name: _packs(mdl) for name, mdl in named}
    assert kinds["Berlin_Air_Lift_Problem"] and not kinds["Sudoku4x4"] and not kinds["Fertilizer"] and not kinds["Monster_II"]
    assert 15 <= sum(kinds.values()) < len(kinds)
    got = solve_packed([mdl for _, mdl in named], lib=oracle_lib)
    assert len(got) == len(named)
    for (name, mdl), g in zip(named, got):
        assert repr(g) == repr(Solve(mdl, lib=oracle_lib)), name
    assert solve_packed([], lib=oracle_lib) == []


@pytest.mark.parametrize("name", ["fuzz_services.jsonl.gz", "fuzz_soft.jsonl.gz"])
def test_solve_packed_equals_solve_on_the_fuzz_models(oracle_lib, name):
    with gzip.open(os.path.join(G.GOLDEN, name), "rt") as fh:
        models = [json.loads(line)["model"] for _, line in zip(range(200), fh)]
    assert len(models) == 200
    n_packed = sum(_packs(m) for m in models)
    # (the service fuzz is all MILPs: every model takes Solve's route; the soft-constraint fuzz takes both routes)
    assert n_packed == 0 if name == "fuzz_services.jsonl.gz" else 0 < n_packed < 200
    got = solve_packed(models, lib=oracle_lib)
    for k, (mdl, g) in enumerate(zip(models, got)):
        assert repr(g) == repr(Solve(mdl, lib=oracle_lib)), k


def test_solve_packed_rejects_before_solving(oracle_lib, monkeypatch):
    berlin = G.load(os.path.join(G.GOLDEN, "fixtures", "Berlin_Air_Lift_Problem.json.gz"))["model"]
    made = []
    real = TableauPack.__init__
    monkeypatch.setattr(TableauPack, "__init__", lambda self, *a, **k: (made.append(1), real(self, *a, **k))[1])
    with pytest.raises(ValueError, match="requires a model"):
        solve_packed([berlin, None], lib=oracle_lib)
    bad = dict(berlin, options={"keep_solutions": True})
    with pytest.raises(UnsupportedModel):
        solve_packed([berlin, bad], lib=oracle_lib)
    assert not made  # no pack was built, let alone solved
    assert solve_packed([berlin], lib=oracle_lib) == [Solve(berlin, lib=oracle_lib)] and made


def _lp(g):
    tab = g["tableau"]
    m, vibr, vibc = G.dense_tableau(tab)
    return (m, vibr, vibc, tab["unrestricted"]), tab["precision"], bool(tab["checkForCycles"])


def _single(lib, lp, precision, check):
    t = Tableau(*lp, precision=precision, lib=lib)
    res = t.simplex(check_cycles=check)
    return t, res


def test_tableau_pack_against_single_engines(oracle_lib):
    """per-LP check_cycles, read_rhs, download and pivot_trace; a cycling LP with the check on between LPs with it off"""
    fx = {G.ident(p): G.load(p) for p in G.fixture_paths()}
    names = ["Berlin_Air_Lift_Problem", "Unrestricted", "Infeasible_1", "Wiki_1", "TacoParty"]
    lps, precs, checks = [], [], []
    for n in names:
        lp, p, c = _lp(fx[n])
        lps.append(lp); precs.append(p); checks.append(False)
    g, m, vibr, vibc = _instance(os.path.join(G.GOLDEN, "cycles", "deg_178868.json.gz"))
    lps.insert(2, (m, vibr, vibc, g["tableau"]["unrestricted"])); precs.insert(2, g["tableau"]["precision"]); checks.insert(2, True)
    pack = TableauPack(lps, precision=precs, lib=oracle_lib, trace_cap=4096)
    assert len(pack) == 6 and pack.launches == 0
    out = pack.simplex(check_cycles=checks)
    assert out.dtype == _capi.RESULT_DTYPE and out.shape == (6,) and not pack.status.any()
    for i, (lp, p, c) in enumerate(zip(lps, precs, checks)):
        t, res = _single(oracle_lib, lp, p, c)
        assert pack.result(i).as_dict() == res.as_dict(), i
        assert {k: out[i][k].item() for k in out.dtype.names} == res.as_dict() or np.isnan(res.evaluation)
        assert pack.evaluation[i] == t.evaluation and pack.feasible[i] == t.feasible and pack.bounded[i] == t.bounded
        for a, b in zip(pack.read_rhs(i), t.read_rhs()):
            assert a.tobytes() == b.tobytes()
        for a, b in zip(pack.download(i), t.download()):
            assert a.tobytes() == b.tobytes()
        assert pack.pivot_trace(i).tobytes() == t.pivot_trace().tobytes()
        t.close()
    assert _messages(pack.result(2)) == g["messages"] and pack.result(0).cycle_phase == 0
    # one flag for all, and a list of the wrong length
    pack.upload()
    again = pack.simplex(check_cycles=True)
    assert again["pivots_phase1"].tolist() == out["pivots_phase1"].tolist()
    with pytest.raises(ValueError):
        pack.simplex(check_cycles=[True])
    pack.close()
    pack.close()  # (idempotent)


def test_tableau_pack_refuses_what_does_not_fit(oracle_lib):
    big = np.zeros((193, 65))
    with pytest.raises(_capi.EngineError, match="64 KiB"):
        TableauPack([(big, [-1] * 193, [-1] * 65, [])], lib=oracle_lib)
    with pytest.raises(ValueError):
        TableauPack([(np.zeros((3, 3)), [-1] * 4, [-1] * 3, [])], lib=oracle_lib)
    with pytest.raises(ValueError):
        TableauPack([(np.zeros((3, 3)), [-1, 1, 2], [-1, 3, 4], [])], precision=[1e-8, 1e-8], lib=oracle_lib)
    assert len(TableauPack([], lib=oracle_lib).simplex()) == 0
