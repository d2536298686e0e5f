"""The many-LP extension's boundary (runs without a GPU): include/jslpm_many.h, the ctypes table MANY_SYMBOLS and the jslpm_ exports of
the product and test libraries agree; the extension stays out of jslp_engine.h, out of the oracle and apart from the other tables; the
argument checks of jslpm_simplex_many refuse bad calls before touching a device; and on the CPU solve_many equals Solve model by model."""
import ctypes
import os
import re
import subprocess

import pytest

import golden_util as G
from jslpsolver_amd import Solve, UnsupportedModel, _capi, solve_many
from jslpsolver_amd.engine import simplex_many

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslpm_many.h")
CHAOS = os.path.join(ROOT, "jslpsolver_amd", "csrc", "libjslp_hip_chaos.so")


def declared_in_header(path=HEADER, prefix="jslpm_"):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, text))


def exported(path, prefix="jslpm_"):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith(prefix)}


def built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def test_header_and_binding_declare_the_same_extension():
    assert declared_in_header() == set(_capi.MANY_SYMBOLS) == {"jslpm_simplex_many"}
    assert not declared_in_header(os.path.join(ROOT, "include", "jslp_engine.h"))  # the drop-in boundary stays as it is
    assert not set(_capi.MANY_SYMBOLS) & set(_capi.SYMBOLS)
    assert not set(_capi.MANY_SYMBOLS) & set(_capi.BRANCH_SYMBOLS)


def test_product_and_test_libraries_export_the_extension():
    assert exported(built(_capi.HIP_LIB_PATH)) == declared_in_header()
    assert exported(built(CHAOS)) == declared_in_header()
    assert _capi.Library(_capi.HIP_LIB_PATH).has_many


def test_oracle_does_not_export_the_extension(oracle_lib):
    assert exported(oracle_lib.path) == set()
    assert not oracle_lib.has_many


def test_argument_errors_without_a_device():
    """refused with JSLP_ERR_ARG before any engine is looked at or any device touched"""
    lib = _capi.Library(built(_capi.HIP_LIB_PATH))
    out = (_capi.SimplexResult * 2)()
    handles = (ctypes.c_void_p * 2)(None, None)
    assert lib.jslpm_simplex_many(None, 2, None, out, None) == _capi.JSLP_ERR_ARG
    assert lib.jslpm_simplex_many(handles, -1, None, out, None) == _capi.JSLP_ERR_ARG
    assert lib.jslpm_simplex_many(handles, 2, None, None, None) == _capi.JSLP_ERR_ARG
    assert lib.jslpm_simplex_many(None, 0, None, None, None) == _capi.JSLP_OK  # nothing to do
    # a null engine in the list: the engine state is wrong, not the arguments
    assert lib.jslpm_simplex_many(handles, 2, None, out, None) == _capi.JSLP_ERR_STATE
    assert b"engine 0" in lib.jslp_last_error()


def test_simplex_many_on_the_oracle_is_a_loop(oracle_lib):
    from jslpsolver_amd.engine import Tableau
    assert simplex_many([]) == []
    g = G.load(os.path.join(G.GOLDEN, "fixtures", "Berlin_Air_Lift_Problem.json.gz"))
    m, vibr, vibc = G.dense_tableau(g["tableau"])
    a, b = (Tableau(m, vibr, vibc, lib=oracle_lib) for _ in range(2))
    res = simplex_many([a], check_cycles=[True])
    ref = b.simplex(check_cycles=True)
    assert res[0].as_dict() == ref.as_dict() and a.evaluation == b.evaluation
    with pytest.raises(ValueError):
        simplex_many([a, b], check_cycles=[True])
    a.close(); b.close()


def _models():
    out = []
    for path in G.fixture_paths():
        g = G.load(path)
        if g["model"] is not None:
            out.append((G.ident(path), g["model"]))
    return out


def test_solve_many_equals_solve_on_every_fixture(oracle_lib):
    """all 47 fixtures, LP and MILP, in one call with duplicates: the same list as Solve model by model"""
    named = _models()
    assert len(named) == 47
    models = [mdl for _, mdl in named] + [named[0][1], named[1][1]]
    got = solve_many(models, lib=oracle_lib)
    want = [Solve(mdl, lib=oracle_lib) for mdl in models]
    assert len(got) == len(want)
    for (name, _), g, w in zip(named + named[:2], got, want):
        assert repr(g) == repr(w), name
    assert solve_many([], lib=oracle_lib) == []


def test_solve_many_rejects_before_solving(oracle_lib):
    berlin = G.load(os.path.join(G.GOLDEN, "fixtures", "Berlin_Air_Lift_Problem.json.gz"))["model"]
    with pytest.raises(ValueError, match="requires a model"):
        solve_many([berlin, None], lib=oracle_lib)
    bad = dict(berlin, options={"keep_solutions": True})
    with pytest.raises(UnsupportedModel):
        solve_many([berlin, bad], lib=oracle_lib)
