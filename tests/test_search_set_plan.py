"""Search for a set of patterns on the CPU: the planner, the seam pairs and the limit rule of the reader's search_set
(indexed_bzip2_amd/csrc/bz2_search.hpp) under AddressSanitizer + UBSan -- tests/native/search_set_cases.cpp checks them
against a byte-by-byte restatement --, the bindings, the argument checks that need no GPU (every limit of a set, through
Python and through the raw C calls), and the tool's help."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES

HARNESS = os.path.join(ROOT, "tests", "native", "search_set_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_search_set_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "search_set_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "search set ok" in run.stdout


def test_every_set_symbol_is_bound(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in ("count_bytes_set", "find_bytes_set", "reader_search_set", "reader_take_set_matches", "reader_grep_set"):
        assert "mi355x_bz2_" + name in names
        assert callable(getattr(native.lib(), "mi355x_bz2_" + name))
    for method in ("count_bytes_set", "find_bytes_set"):
        assert callable(getattr(native.Decoder, method))
    for method in ("count_matches_each", "find_all_any", "find_any", "grep_any", "count_matching_lines_any",
                   "grep_any_to_tensor"):
        assert callable(getattr(native.reader._IndexedBzip2FileParallel, method))
        assert callable(getattr(native.IndexedBzip2File, method))
    assert native.lib().mi355x_bz2_abi_version() == 2


def test_help_lists_the_file_options(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --grep-file arg" in run.stdout
    assert b"      --count-matches-file arg" in run.stdout
    assert b"      --count-matches arg" in run.stdout and b"      --grep arg" in run.stdout


def test_refused_combinations_of_the_tool(native, tmp_path):
    """Refused before the input is opened: no GPU is needed."""
    patterns = tmp_path / "patterns.txt"
    patterns.write_bytes(b"dolor\nipsum\n")
    path = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
    for options in (["--grep-file", str(patterns), "--grep", "x"], ["--grep-file", str(patterns), "--count-matches", "x"],
                    ["--count-matches-file", str(patterns), "--grep", "x"],
                    ["--count-matches-file", str(patterns), "--count-matches", "x"],
                    ["--grep-file", str(patterns), "--count-matches-file", str(patterns)],
                    ["--count-matches-file", str(patterns), "--line-number"]):
        run = subprocess.run([CLI] + options + [path], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", options
        assert b"cannot be combined" in run.stderr or b"needs" in run.stderr, options
    # an empty line that is not the final one, and a file that does not exist
    patterns.write_bytes(b"dolor\n\nipsum\n")
    run = subprocess.run([CLI, "--grep-file", str(patterns), path], capture_output=True, timeout=300)
    assert run.returncode != 0 and b"empty line (line 2)" in run.stderr
    run = subprocess.run([CLI, "--count-matches-file", str(tmp_path / "none"), path], capture_output=True, timeout=300)
    assert run.returncode != 0 and b"pattern file" in run.stderr


BAD_SETS = [([], "1 to 1024 patterns"), ([b"a"] * 1025, "1 to 1024 patterns"), ([b"ab", b""], "1 to 256 bytes"),
            ([b"ab", b"x" * 257], "1 to 256 bytes"), ([b"x" * 256] * 64 + [b"y"], "at most 16384 bytes")]


def test_sets_are_checked_without_a_gpu(native):
    """Every limit of a set is refused by the Python layer and, behind it, by the reader itself before anything is
    launched; the message names the limit."""
    path = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
    with native.open(path, parallelization=0) as f:
        calls = (f.count_matches_each, f.find_all_any, f.find_any, f.grep_any, f.count_matching_lines_any,
                 f.grep_any_to_tensor, lambda patterns: f.find_all_any(patterns, limit=0),
                 lambda patterns: f.grep_any(patterns, limit=0))
        for bad, words in BAD_SETS:
            for call in calls:
                with pytest.raises(ValueError) as failure:
                    call(bad)
                assert words in str(failure.value), (words, str(failure.value))
        for bad in (["text"], [b"ab", "cd"], b"ab", bytearray(b"ab"), memoryview(b"ab"), "ab", None, 7, [None], [7]):
            for call in calls:
                with pytest.raises(TypeError):
                    call(bad)
        for call in (f.count_matches_each, f.find_all_any, f.find_any):
            with pytest.raises(ValueError):
                call([b"a"], -1)
            with pytest.raises(ValueError):
                call([b"a"], 0, -5)
        with pytest.raises(ValueError):
            f.find_all_any([b"a"], limit=-1)
        # the limits themselves are accepted by the check (a tuple and a generator are sequences enough)
        assert native._native.pattern_set((b"x" * 16 for _ in range(1024)))[2] == 1024
        assert native._native.pattern_set((bytearray(b"a"), memoryview(b"x" * 256)))[2] == 2

        reader, lib = f.bz2reader, native.lib()
        n = ctypes.c_uint64(99)
        each = (ctypes.c_uint64 * 1100)()
        lines, total = ctypes.c_uint64(), ctypes.c_uint64()
        for bad, words in BAD_SETS:
            data = b"".join(bad)
            sizes = (ctypes.c_uint32 * max(1, len(bad)))(*map(len, bad))
            for limit in (0, 5):
                assert lib.mi355x_bz2_reader_search_set(reader._h, data, sizes, len(bad), 0, 2**64 - 1, limit,
                                                        ctypes.byref(n), each) == 103
                assert words.encode() in lib.mi355x_bz2_reader_last_error(reader._h)
            assert lib.mi355x_bz2_reader_grep_set(reader._h, data, sizes, len(bad), 10, 0, 2**64 - 1, 5, 0,
                                                  ctypes.byref(lines), ctypes.byref(total)) == 103
            assert words.encode() in lib.mi355x_bz2_reader_last_error(reader._h)
            with pytest.raises(ValueError):
                reader._check(103)
        sizes = (ctypes.c_uint32 * 1)(2)
        assert lib.mi355x_bz2_reader_search_set(reader._h, None, sizes, 1, 0, 10, 0, ctypes.byref(n), None) == 103
        assert lib.mi355x_bz2_reader_search_set(reader._h, b"ab", None, 1, 0, 10, 0, ctypes.byref(n), None) == 103
        assert lib.mi355x_bz2_reader_search_set(reader._h, b"ab", sizes, 1, 0, 10, 0, None, None) == 103
        # nothing is held by a search that was refused
        assert lib.mi355x_bz2_reader_take_set_matches(reader._h, None, None, 0) == 103
