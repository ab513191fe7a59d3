"""Grep and line numbers on the CPU: the planner of the reader's line_numbers (planLineNumbers in
indexed_bzip2_amd/csrc/bz2_lines.hpp) under AddressSanitizer + UBSan -- tests/native/linenum_cases.cpp checks launches,
queries and answers against a byte-by-byte restatement --, the bindings, the argument checks that need no GPU, and the
tool's help."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES

HARNESS = os.path.join(ROOT, "tests", "native", "linenum_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_line_number_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "linenum_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "linenum ok" in run.stdout


def test_every_grep_symbol_is_bound(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in ("rank_byte", "reader_line_numbers", "reader_grep", "reader_take_grep"):
        assert "mi355x_bz2_" + name in names
        assert callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert callable(native.Decoder.rank_byte)
    for method in ("line_numbers", "grep", "count_matching_lines", "grep_to_tensor"):
        assert callable(getattr(native.reader._IndexedBzip2FileParallel, method))
        assert callable(getattr(native.IndexedBzip2File, method))
    assert native.lib().mi355x_bz2_abi_version() == 2


def test_help_lists_grep(native):
    assert os.path.exists(CLI)
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --grep arg" in run.stdout                # long only, with its argument
    assert b"      --line-number " in run.stdout
    assert b"exit status is 0 whether or not a line matched" in run.stdout
    assert b"      --count-matches arg" in run.stdout and b"--count-lines" in run.stdout      # the lines that were there


def test_option_combinations_are_refused(native):
    """--grep and --count-matches share the pattern, --line-number means nothing without --grep: status 1 and a message,
    before the input is looked at."""
    path = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
    for args in (["--grep", "a", "--count-matches", "b", path], ["--count-matches", "b", "--grep=a", path],
                 ["--line-number", path], ["--line-number", "--count-matches", "b", path], ["--line-number", "--count-lines", path]):
        run = subprocess.run([CLI] + args, capture_output=True, timeout=300)
        assert run.returncode == 1 and run.stdout == b"", args
        assert b"--grep" in run.stderr


def test_grep_arguments_are_checked_without_a_gpu(native):
    """Pattern, range, limit, newline and offsets are refused by the Python layer and, behind it, by the reader itself
    before anything is launched."""
    path = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
    with native.open(path, parallelization=0) as f:
        for call in (f.grep, f.count_matching_lines, f.grep_to_tensor):
            for bad in (b"", b"x" * 257, bytearray(300), memoryview(b"")):
                with pytest.raises(ValueError):
                    call(bad)
            for bad in ("text", None, 7):
                with pytest.raises(TypeError):
                    call(bad)
            with pytest.raises(ValueError):
                call(b"a", -1)
            with pytest.raises(ValueError):
                call(b"a", 0, -5)
            for newline in (b"", b"\r\n", "\n", None, 10):
                with pytest.raises(ValueError):
                    call(b"a", newline=newline)
        for call in (f.grep, f.grep_to_tensor):
            with pytest.raises(ValueError):
                call(b"a", limit=-1)
            with pytest.raises(ValueError):
                call(b"", limit=0)
        for bad in ([-1], [3, -7], [2**64]):
            with pytest.raises(ValueError):
                f.line_numbers(bad)
        for newline in (b"", b"ab", "\n"):
            with pytest.raises(ValueError):
                f.line_numbers([0], newline=newline)
        with pytest.raises(ValueError):
            f.grep(b"a", -1, limit=0)
        with pytest.raises(ValueError):
            f.grep(b"a", 0, -5, limit=0)
        numbers, lines = f.grep(b"a", limit=0)             # nothing is asked for, nothing is launched
        assert numbers.dtype.name == "uint64" and len(numbers) == 0 and lines == []

        reader = f.bz2reader
        lib = native.lib()
        n, total = ctypes.c_uint64(99), ctypes.c_uint64(99)
        for pattern in (b"", b"y" * 257):
            for max_lines in (0, 5):
                assert lib.mi355x_bz2_reader_grep(reader._h, pattern, len(pattern), 10, 0, 2**64 - 1, max_lines, 0,
                                                  ctypes.byref(n), ctypes.byref(total)) == 103
                assert b"1 to 256" in lib.mi355x_bz2_reader_last_error(reader._h)
        assert lib.mi355x_bz2_reader_grep(reader._h, None, 3, 10, 0, 10, 0, 0, ctypes.byref(n), ctypes.byref(total)) == 103
        assert lib.mi355x_bz2_reader_grep(reader._h, b"abc", 3, 10, 0, 10, 0, 0, None, ctypes.byref(total)) == 103
        # nothing is held by a grep that was refused, or before any grep
        numbers, sizes = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
        assert lib.mi355x_bz2_reader_take_grep(reader._h, numbers, sizes, 4) == 103
        assert lib.mi355x_bz2_reader_take_grep(reader._h, None, None, 0) == 103
        assert lib.mi355x_bz2_reader_take_grep(reader._h, None, sizes, 4) == 103
        assert lib.mi355x_bz2_reader_line_numbers(reader._h, 10, None, 3, numbers) == 103
        assert lib.mi355x_bz2_reader_line_numbers(reader._h, 10, numbers, 3, None) == 103
    # a closed reader answers nothing, also where nothing is asked for
    for call in (f.grep, f.grep_to_tensor):
        with pytest.raises(ValueError):
            call(b"a", limit=0)
    with pytest.raises(ValueError):
        f.count_matching_lines(b"a")
    # the decoder's rank_byte refuses null lists before it touches the device
    assert native.lib().mi355x_bz2_rank_byte(None, None, 0, 10, None) == 103
