"""Worker of tests/test_measure_modes.py for the one launch shape whose knob is latched per process: phase 1 through k_select + k_update
(JSLP_FUSED_P1=0, set by the parent) in front of the fused phase 2.  argv[1]: a pickle of {instance name: what the oracle and the independent
count say} (test_measure_modes.want); every instance runs measure_modes.run_case on the product library.  Prints "ok" at the end."""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import measure_modes as M  # noqa: E402
from jslpsolver_amd import _capi  # noqa: E402


def main():
    assert os.environ.get("JSLP_FUSED_P1") == "0" and os.environ.get("JSLP_DEBUG_LAUNCH")
    with open(sys.argv[1], "rb") as fh:
        wants = pickle.load(fh)
    lib = _capi.load_hip()
    for name, w in wants.items():
        M.run_case(lib, name, "fused-p1off", w)
    print("ok")


if __name__ == "__main__":
    main()
