"""The MIR extension's boundary (runs without a GPU): include/jslpr_mir.h, the ctypes table MIR_SYMBOLS and the jslpr_ exports of the
product library agree; the oracle goes without; the outcome record is 32 bytes on both sides."""
import os

from jslpsolver_amd import _capi
from test_many_abi import built, declared_in_header, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslpr_mir.h")


def test_header_binding_and_library_agree():
    declared = declared_in_header(HEADER, "jslpr_")
    assert declared == set(_capi.MIR_SYMBOLS) == {"jslpr_mir_outcome_bytes", "jslpr_engine_relax_mir"}
    assert exported(built(_capi.HIP_LIB_PATH), "jslpr_") == declared
    assert not declared_in_header(os.path.join(ROOT, "include", "jslp_engine.h"), "jslpr_")
    for other in (_capi.SYMBOLS, _capi.BRANCH_SYMBOLS, _capi.MANY_SYMBOLS, _capi.F32_SYMBOLS):
        assert not set(_capi.MIR_SYMBOLS) & set(other)


def test_outcome_record_is_32_bytes():
    lib = _capi.Library(built(_capi.HIP_LIB_PATH))
    assert lib.has_mir
    assert lib.jslpr_mir_outcome_bytes() == 32 == _capi.C.sizeof(_capi.MirOutcome) == _capi.MIR_OUTCOME_DTYPE.itemsize
    assert "JSLPR_MAX_ROUNDS %d" % _capi.JSLPR_MAX_ROUNDS in open(HEADER).read()


def test_oracle_does_not_export_the_extension(oracle_lib):
    assert exported(oracle_lib.path, "jslpr_") == set() and not oracle_lib.has_mir
