"""The stream layout (indexed_bzip2_amd/csrc/bz2_lanes.hpp) on the CPU, under AddressSanitizer + UBSan:
tests/native/lanes_cases.cpp pins the lanes of a batch for queue budgets 1 to 32 and 1 to 8 live contexts, with and
without an expensive group and side-by-side k_mtf instances, and checks the invariants the launcher relies on."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "native", "lanes_cases.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lane_layout_under_sanitizers(tmp_path):
    exe = tmp_path / "lanes_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "lanes ok" in run.stdout
