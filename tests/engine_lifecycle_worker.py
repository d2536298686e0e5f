"""Subprocess body of tests/test_engine_lifecycle.py (JSLP_NO_POOL is read once per process): runs the module's script of calls on the
product library and leaves the observations in a file.  The first failure of any kind ends the process."""
import os
import pickle
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jslpsolver_amd import _capi  # noqa: E402
import test_engine_lifecycle as L  # noqa: E402


def main():
    plan_file, obs_file = sys.argv[1], sys.argv[2]
    try:
        with open(plan_file, "rb") as fh:
            plan = pickle.load(fh)
        obs = L.run_script(_capi.load_hip(), plan, True)
        with open(obs_file, "wb") as fh:
            pickle.dump(obs, fh)
        print("ok", flush=True)
    except BaseException:
        print(traceback.format_exc(), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
