"""The arithmetic of the query launchers (indexed_bzip2_amd/csrc/bz2_query_layout.hpp) on the CPU, under AddressSanitizer
+ UBSan: tests/native/query_layout_cases.cpp checks that the tiler's tiles are in order, disjoint, at most a tile long and
cover exactly the start positions of every span -- around every boundary, beyond 2^32, with empty and repeated spans --
and that every staging layout has the offsets, alignments and totals of the hand-written arithmetic it replaced."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "native", "query_layout_cases.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_query_layout_under_sanitizers(tmp_path):
    exe = tmp_path / "query_layout_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "query layout ok" in run.stdout
