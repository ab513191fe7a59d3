"""ignore_case on the CPU: foldAscii, the seam matches and the set image with the fold flag (indexed_bzip2_amd/csrc/
bz2_search.hpp) under AddressSanitizer + UBSan -- tests/native/search_fold_cases.cpp checks them against a byte-by-byte
restatement --, the eight _ex bindings, the keyword-only argument, the flag check of the reader (no GPU is needed: an
unknown bit is refused before anything is launched or held), and the tool's option."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES

HARNESS = os.path.join(ROOT, "tests", "native", "search_fold_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")

EX = ("count_bytes_ex", "find_bytes_ex", "count_bytes_set_ex", "find_bytes_set_ex", "reader_search_ex", "reader_grep_ex",
      "reader_search_set_ex", "reader_grep_set_ex")
DECODER_METHODS = ("count_bytes", "find_bytes", "count_bytes_set", "find_bytes_set")
READER_METHODS = ("count_matches", "find_all", "find", "grep", "count_matching_lines", "grep_to_tensor", "count_matches_each",
                  "find_all_any", "find_any", "grep_any", "count_matching_lines_any", "grep_any_to_tensor")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_search_fold_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "search_fold_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "search fold ok" in run.stdout


def test_every_ex_symbol_is_bound(native):
    names = {name: arguments for name, _, arguments in native._native.SYMBOLS}
    for name in EX:
        assert "mi355x_bz2_" + name in names
        assert callable(getattr(native.lib(), "mi355x_bz2_" + name))
        # its namesake with one uint32 more
        assert len(names["mi355x_bz2_" + name]) == len(names["mi355x_bz2_" + name[:-3]]) + 1
    assert native._native.SEARCH_IGNORE_CASE == 1
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays


def test_ignore_case_is_keyword_only_and_off_by_default(native):
    classes = [(native.Decoder, DECODER_METHODS), (native.reader._IndexedBzip2FileParallel, READER_METHODS),
               (native.IndexedBzip2File, READER_METHODS)]
    for cls, methods in classes:
        for method in methods:
            parameter = inspect.signature(getattr(cls, method)).parameters["ignore_case"]
            assert parameter.kind is inspect.Parameter.KEYWORD_ONLY, (cls.__name__, method)
            assert parameter.default is False, (cls.__name__, method)
    # given positionally it is a TypeError, not a start, an end, a limit or a newline
    for opened in (native.open(PATH, parallelization=0), native.IndexedBzip2File(PATH, parallelization=0)):
        with opened as f:
            for call in (f.count_matches, f.find, f.count_matches_each, f.find_any):
                with pytest.raises(TypeError):
                    call(b"dolor" if "each" not in call.__name__ and "any" not in call.__name__ else [b"dolor"], 0, None, True)
            for call in (f.find_all, f.count_matching_lines):
                with pytest.raises(TypeError):
                    call(b"dolor", 0, None, None if call.__name__ == "find_all" else b"\n", True)
            for call in (f.find_all_any, f.count_matching_lines_any):
                with pytest.raises(TypeError):
                    call([b"dolor"], 0, None, None if call.__name__ == "find_all_any" else b"\n", True)
            for call in (f.grep, f.grep_to_tensor):
                with pytest.raises(TypeError):
                    call(b"dolor", 0, None, None, b"\n", True)
            for call in (f.grep_any, f.grep_any_to_tensor):
                with pytest.raises(TypeError):
                    call([b"dolor"], 0, None, None, b"\n", True)
            # the argument checks that need no GPU still come first with the keyword given
            with pytest.raises(ValueError):
                f.count_matches(b"", ignore_case=True)
            with pytest.raises(ValueError):
                f.find_all(b"x" * 257, ignore_case=True)
            with pytest.raises(ValueError):
                f.count_matches_each([], ignore_case=True)
            assert len(f.find_all(b"dolor", limit=0, ignore_case=True)) == 0
            assert f.grep(b"dolor", limit=0, ignore_case=True)[1] == []


def test_unknown_flag_bits_are_refused_and_nothing_is_held(native):
    """Every bit but MI355X_BZ2_SEARCH_IGNORE_CASE is 103 from the four reader calls, with a last_error that says so,
    before anything is launched (no GPU is needed) or held."""
    with native.open(PATH, parallelization=0) as f:
        reader, lib = f.bz2reader, native.lib()
        n, lines, total = ctypes.c_uint64(99), ctypes.c_uint64(), ctypes.c_uint64()
        sizes = (ctypes.c_uint32 * 2)(2, 3)
        each = (ctypes.c_uint64 * 2)()
        for flags in (2, 4, 0x80000000, 3, 0xFFFFFFFE, 0xFFFFFFFF):
            for limit in (0, 5):
                assert lib.mi355x_bz2_reader_search_ex(reader._h, b"ab", 2, flags, 0, 2**64 - 1, limit, ctypes.byref(n)) == 103
                error = lib.mi355x_bz2_reader_last_error(reader._h)
                assert b"search: unknown flag bits 0x%X" % (flags & ~1) in error, error
                assert lib.mi355x_bz2_reader_take_matches(reader._h, None, 0) == 103            # nothing is held
                assert lib.mi355x_bz2_reader_search_set_ex(reader._h, b"abcde", sizes, 2, flags, 0, 2**64 - 1, limit,
                                                           ctypes.byref(n), each) == 103
                error = lib.mi355x_bz2_reader_last_error(reader._h)
                assert b"search_set: unknown flag bits 0x%X" % (flags & ~1) in error, error
                assert lib.mi355x_bz2_reader_take_set_matches(reader._h, None, None, 0) == 103
            for max_lines in (0, 5):
                assert lib.mi355x_bz2_reader_grep_ex(reader._h, b"ab", 2, flags, 10, 0, 2**64 - 1, max_lines, 0,
                                                     ctypes.byref(lines), ctypes.byref(total)) == 103
                assert b"grep: unknown flag bits" in lib.mi355x_bz2_reader_last_error(reader._h)
                assert lib.mi355x_bz2_reader_grep_set_ex(reader._h, b"abcde", sizes, 2, flags, 10, 0, 2**64 - 1, max_lines, 0,
                                                         ctypes.byref(lines), ctypes.byref(total)) == 103
                assert b"grep_set: unknown flag bits" in lib.mi355x_bz2_reader_last_error(reader._h)
                assert lib.mi355x_bz2_reader_take_grep(reader._h, None, None, 0) == 103
            with pytest.raises(ValueError):
                reader._check(103)
        # the flag is looked at before the set: both wrong names the flag; a good flag lets the set's limits speak
        bad = (ctypes.c_uint32 * 1)(0)
        assert lib.mi355x_bz2_reader_search_set_ex(reader._h, b"ab", bad, 1, 2, 0, 10, 0, ctypes.byref(n), None) == 103
        assert b"unknown flag bits 0x2" in lib.mi355x_bz2_reader_last_error(reader._h)
        assert lib.mi355x_bz2_reader_search_set_ex(reader._h, b"ab", bad, 1, 1, 0, 10, 0, ctypes.byref(n), None) == 103
        assert b"1 to 256 bytes" in lib.mi355x_bz2_reader_last_error(reader._h)
        # the null checks of the namesakes hold for the _ex forms
        assert lib.mi355x_bz2_reader_search_ex(reader._h, None, 2, 1, 0, 10, 0, ctypes.byref(n)) == 103
        assert lib.mi355x_bz2_reader_search_ex(reader._h, b"ab", 2, 1, 0, 10, 0, None) == 103
        assert lib.mi355x_bz2_reader_search_ex(reader._h, b"ab", 0, 1, 0, 10, 0, ctypes.byref(n)) == 103
        assert lib.mi355x_bz2_reader_grep_ex(reader._h, None, 2, 1, 10, 0, 10, 0, 0, ctypes.byref(lines), ctypes.byref(total)) == 103
        # an empty range needs no launch: the known flag is accepted, and a limit holds the (empty) result
        assert lib.mi355x_bz2_reader_search_ex(reader._h, b"ab", 2, 1, 7, 7, 5, ctypes.byref(n)) == 0 and n.value == 0
        assert lib.mi355x_bz2_reader_take_matches(reader._h, None, 0) == 0
        assert lib.mi355x_bz2_reader_take_matches(reader._h, None, 0) == 103
        # a refused call leaves what an earlier call holds alone
        assert lib.mi355x_bz2_reader_search_ex(reader._h, b"ab", 2, 0, 7, 7, 5, ctypes.byref(n)) == 0
        assert lib.mi355x_bz2_reader_search_ex(reader._h, b"ab", 2, 8, 7, 7, 5, ctypes.byref(n)) == 103
        assert lib.mi355x_bz2_reader_take_matches(reader._h, None, 0) == 0


def test_help_lists_ignore_case(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --ignore-case " in run.stdout
    assert b"  -i, --input arg" in run.stdout                  # -i stays the input
    assert b"--grep error --ignore-case" in run.stdout


def test_ignore_case_alone_is_refused(native, tmp_path):
    """Refused before the input is opened: no GPU is needed."""
    for options in (["--ignore-case"], ["--ignore-case", "--count-lines"], ["--ignore-case", "-d"],
                    ["--ignore-case", "--line-number"]):
        run = subprocess.run([CLI] + options + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", options
        assert b"needs" in run.stderr, options
    run = subprocess.run([CLI, "--ignore-case", PATH], capture_output=True, timeout=300)
    assert run.stderr == (b"Option '--ignore-case' needs '--grep', '--grep-file', '--count-matches' or "
                          b"'--count-matches-file'\n")
    # with one of them it is taken: the refusals that remain are the old ones
    patterns = tmp_path / "patterns.txt"
    patterns.write_bytes(b"dolor\n")
    run = subprocess.run([CLI, "--ignore-case", "--grep", "x", "--count-matches", "y", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and b"cannot be combined" in run.stderr
    run = subprocess.run([CLI, "--ignore-case", "--count-matches-file", str(patterns), "--line-number", PATH],
                         capture_output=True, timeout=300)
    assert run.returncode != 0 and b"'--line-number' needs" in run.stderr
