"""The failure paths of the engine's memory owners (jslpsolver_amd/csrc/jslp_host_mem.h: DevBuf / PinBuf, the staging pair, the carve
helper, the parked bundle) where they can be walked: on a host WITHOUT a GPU every HIP allocation is refused.  tests/host_mem_check.cpp
includes that header alone, is built here with the host's address and undefined-behaviour sanitizers and run as a process of its own;
it is never loaded into Python.  With a device visible the allocations would succeed and the program's premise is gone: skipped there."""
import os
import shutil
import subprocess

import pytest

from jslpsolver_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_failure_paths_of_the_memory_owners_under_the_host_sanitizers(tmp_path):
    if _capi.load_hip().jslp_device_count() > 0:
        pytest.skip("a GPU is visible: the refused allocations this program walks are for GPU-less hosts")
    assert shutil.which(HIPCC), "hipcc not found"
    exe = str(tmp_path / "host_mem_check")
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "host_mem_check.cpp")], check=True, timeout=300)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, text=True)
    assert run.returncode == 0 and "host_mem_check ok" in run.stdout and "runtime error" not in run.stdout, run.stdout[-4000:]
