"""k_mtf's data-parallel pass B on the CPU: the per-symbol rule, the fast-path predicate and the digit-sequence flag of
indexed_bzip2_amd/csrc/bz2_mtf_expand.hpp under AddressSanitizer + UBSan -- tests/native/mtf_expand_cases.cpp expands seeded
and hand-made symbol chunks symbol by symbol and compares with a byte-by-byte restatement of the serial pass, 32-bit wraps
included; wherever the two could differ the predicate must choose the serial pass."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "native", "mtf_expand_cases.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_mtf_expand_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "mtf_expand_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "mtf expand ok" in run.stdout
