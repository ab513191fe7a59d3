"""The scratch layout of a decoder context (indexed_bzip2_amd/csrc/bz2_scratch.hpp) on the CPU, under AddressSanitizer +
UBSan: tests/native/scratch_cases.cpp checks alignment, bounds and that only the two declared pairs of regions share
memory, for the capacities of 1 to MI355X_BZ2_MAX_BATCH_BLOCKS blocks with and without KEEP_STAGES, and pins the bytes
of the two allocations."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "native", "scratch_cases.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_scratch_layout_under_sanitizers(tmp_path):
    exe = tmp_path / "scratch_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "scratch ok" in run.stdout
