"""The range planner of read_ranges (indexed_bzip2_amd/csrc/bz2_ranges.hpp) on the CPU, under AddressSanitizer + UBSan:
tests/native/ranges_cases.cpp checks launches, gather pieces, per-range counts and the packed bounded-residency input
against a byte-by-byte restatement, on hand-written maps with end-of-stream entries and two streams and on seeded ones."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "native", "ranges_cases.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_range_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "ranges_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "ranges ok" in run.stdout
