"""Search on the CPU: the planner and the seam matches of the reader's search (indexed_bzip2_amd/csrc/bz2_search.hpp) under
AddressSanitizer + UBSan -- tests/native/search_cases.cpp checks the extents and seamMatches against a byte-by-byte
restatement --, the bindings, the argument checks that need no GPU, and the tool's help."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES

HARNESS = os.path.join(ROOT, "tests", "native", "search_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_search_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "search_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "search ok" in run.stdout


def test_every_search_symbol_is_bound(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in ("count_bytes", "find_bytes", "reader_search", "reader_take_matches"):
        assert "mi355x_bz2_" + name in names
        assert callable(getattr(native.lib(), "mi355x_bz2_" + name))
    for method in ("count_bytes", "find_bytes"):
        assert callable(getattr(native.Decoder, method))
    for method in ("count_matches", "find_all", "find"):
        assert callable(getattr(native.reader._IndexedBzip2FileParallel, method))
        assert callable(getattr(native.IndexedBzip2File, method))
    assert native.lib().mi355x_bz2_abi_version() == 2


def test_help_lists_count_matches(native):
    assert os.path.exists(CLI)
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --count-matches arg" in run.stdout       # long only, with its argument
    assert b"--count-lines" in run.stdout


def test_pattern_size_is_checked_without_a_gpu(native):
    """m == 0 and m > 256 are refused by the Python layer and, behind it, by the reader itself before anything is
    launched."""
    import ctypes
    path = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
    with native.open(path, parallelization=0) as f:
        for bad in (b"", b"x" * 257, bytearray(300), memoryview(b"")):
            with pytest.raises(ValueError):
                f.count_matches(bad)
            with pytest.raises(ValueError):
                f.find_all(bad)
            with pytest.raises(ValueError):
                f.find(bad, 3, 9)
            with pytest.raises(ValueError):
                f.find_all(bad, limit=0)
        for bad in ("text", None, 7):
            with pytest.raises(TypeError):
                f.count_matches(bad)
        with pytest.raises(ValueError):
            f.find_all(b"a", -1)
        with pytest.raises(ValueError):
            f.find_all(b"a", 0, -5)
        with pytest.raises(ValueError):
            f.find_all(b"a", limit=-1)
        reader = f.bz2reader
        n = ctypes.c_uint64(99)
        search = native.lib().mi355x_bz2_reader_search
        for pattern in (b"", b"y" * 257):
            assert search(reader._h, pattern, len(pattern), 0, 2**64 - 1, 0, ctypes.byref(n)) == 103
            assert b"1 to 256" in native.lib().mi355x_bz2_reader_last_error(reader._h)
            with pytest.raises(ValueError):
                reader._check(103)
        assert search(reader._h, None, 3, 0, 10, 0, ctypes.byref(n)) == 103
        # nothing is held by a search that was refused
        assert native.lib().mi355x_bz2_reader_take_matches(reader._h, None, 0) == 103
