"""Lines selected by a field, on the CPU: the definition of indexed_bzip2_amd/csrc/bz2_fieldmatch.hpp.

The plain Python model of fieldmatch.py is checked on known answers; tests/native/fieldmatch_cases.cpp runs the value table
and its plain model under AddressSanitizer + UBSan as a program of its own.  Then the bindings, the argument refusals (all
before anything is launched: no GPU is needed) and the tool's help and refusals."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES
import fieldmatch as FM

HARNESS = os.path.join(ROOT, "tests", "native", "fieldmatch_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
METHODS = ("where_field", "where_field_to_tensor", "count_where_field", "select_lines", "select_lines_to_tensor")
SYMBOLS = ("match_fields", "reader_field_matches", "reader_field_in_range", "reader_take_field_matches", "reader_select_lines")
INVALID_ARGUMENT = 103                                         # MI355X_BZ2_ERR_INVALID_ARGUMENT
NL, TAB = 10, 9


def test_known_answers_of_the_model():
    text = b"a\tGET\t5\nb\t\t\nc\nd\tGE\t-7\ne\tGETS\tx\n\tGET\t007"
    # values: byte-for-byte equality; the empty value matches an empty field that is present, never a missing one
    assert FM.where(text, NL, TAB, 1, values=[b"GET"]) == [0, 5]
    assert FM.where(text, NL, TAB, 1, values=[b""]) == [1]
    assert FM.where(text, NL, TAB, 2, values=[b""]) == [1]
    assert FM.where(text, NL, TAB, 3, values=[b""]) == []
    assert FM.where(text, NL, TAB, 0, values=[b""]) == [5]
    # a value that is a prefix of another; equal values count once
    assert FM.where(text, NL, TAB, 1, values=[b"GE"]) == [3]
    assert FM.where(text, NL, TAB, 1, values=[b"GE", b"GET", b"GE"]) == [0, 3, 5]
    assert FM.where(text, NL, TAB, 1, values=[b"G", b"GETSS", b"get"]) == []
    # values with the newline's neighbours and bytes 0x80..0xFF
    odd = b"k\t\x09x\n\x0b\x0c\tq\n\x80\xff\t\xfe\nz\t\x80\xff"
    assert FM.where(odd, NL, TAB, 0, values=[b"\x0b\x0c", b"\x80\xff"]) == [1, 2]
    assert FM.where(odd, NL, TAB, 1, values=[b"\x80\xff", b"\xfe", b""]) == [0, 2, 3]
    assert FM.where(odd, NL, ord("x"), 0, values=[b"k\t\t"]) == [0]
    # invert: the complement within the line range, the lines without the field included
    assert FM.where(text, NL, TAB, 1, values=[b"GET"], invert=True) == [1, 2, 3, 4]
    assert FM.where(text, NL, TAB, 1, values=[b"GET"], invert=True, first=2, count=3) == [2, 3, 4]
    assert FM.where(text, NL, TAB, 1, values=[b"GET"], first=1) == [5] and FM.where(text, NL, TAB, 1, values=[b"GET"], first=9) == []
    assert FM.where(text, NL, TAB, 1, values=[b"GET"], limit=1) == [0] and FM.where(text, NL, TAB, 1, values=[b"GET"], limit=0) == []
    # ranges: lo = hi, open sides, lo > hi, non-numbers and missing fields, bounds beyond 18 digits
    assert FM.where(text, NL, TAB, 2, between=(5, 5)) == [0]
    assert FM.where(text, NL, TAB, 2, between=(None, None)) == [0, 3, 5]
    assert FM.where(text, NL, TAB, 2, between=(6, None)) == [5] and FM.where(text, NL, TAB, 2, between=(None, 5)) == [0, 3]
    assert FM.where(text, NL, TAB, 2, between=(-7, -7)) == [3] and FM.where(text, NL, TAB, 2, between=(6, 5)) == []
    assert FM.where(text, NL, TAB, 2, between=(None, None), invert=True) == [1, 2, 4]
    assert FM.where(text, NL, TAB, 2, between=(-10**30, 10**30)) == [0, 3, 5]
    assert FM.clipped((-10**30, 10**30)) == (1 - 10**18, 10**18 - 1) == FM.clipped((None, None))
    big = b"%d\n%d\n0\nx\n" % (10**18 - 1, 1 - 10**18)
    assert FM.where(big, NL, TAB, 0, between=(10**18 - 1, None)) == [0] and FM.where(big, NL, TAB, 0, between=(None, 1 - 10**18)) == [1]
    assert FM.where(big, NL, TAB, 0, between=(10**40, None)) == [0]           # clipped to the largest number there is
    assert FM.where(big, NL, TAB, 0, between=(1, -1)) == [] and FM.where(big, NL, TAB, 0, between=(1, -1), invert=True) == [0, 1, 2, 3]
    assert FM.lines_with_delimiters(b"a\n\nb", NL) == [b"a\n", b"\n", b"b"] and FM.lines_with_delimiters(b"a\n", NL) == [b"a\n"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fieldmatch_under_sanitizers(tmp_path):
    exe = tmp_path / "fieldmatch_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "fieldmatch cases ok" in run.stdout


def test_bindings(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in SYMBOLS:
        assert "mi355x_bz2_" + name in names and callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays
    for cls in (native.reader._IndexedBzip2FileParallel, native.IndexedBzip2File):
        for method in METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
    assert "not a CSV parser" in native.reader._IndexedBzip2FileParallel.where_field.__doc__.replace("Not", "not")
    assert callable(native.Decoder.match_fields) and "k_field_match" in native.Decoder.match_fields.__doc__
    N = native._native
    assert (N.FIELD_VALUES_MAX, N.FIELD_VALUE_BYTES_MAX, N.FIELD_VALUES_BYTES_MAX, N.FIELD_NUMBER_MAX) == (1024, 256, 16384, FM.NUMBER_MAX)
    data, sizes, n = N.value_set([b"ab", b"", bytearray(b"c")])
    assert data == b"abc" and list(sizes)[:3] == [2, 0, 1] and n == 3
    assert N.number_range((None, 5)) == (0, 0, 1, 5) and N.number_range((-10**30, 10**30)) == (1, 1 - 10**18, 1, 10**18 - 1)
    assert N.number_range((7, None)) == (1, 7, 0, 0)


BAD_VALUES = ([], [b"x"] * 1025, [b"v" * 257], [b"%04d" % i + b"p" * 252 for i in range(64)] + [b"q"])


def test_argument_refusals(native):
    """All refused before anything is launched: no GPU is needed."""
    assert sum(map(len, BAD_VALUES[3])) == 16385
    for opened in (native.open(PATH, parallelization=0), native.IndexedBzip2File(PATH, parallelization=0)):
        with opened as f:
            for method in METHODS:
                call = getattr(f, method)
                # both or neither of values and between
                with pytest.raises(ValueError):
                    call(0)
                with pytest.raises(ValueError):
                    call(0, values=[b"a"], between=(1, 2))
                for values in BAD_VALUES:
                    with pytest.raises(ValueError):
                        call(0, values=values)
                for values in (b"abc", "abc", [b"a", "b"], [1]):
                    with pytest.raises(TypeError):
                        call(0, values=values)
                for between in (5, (1,), (1, 2, 3)):
                    with pytest.raises(ValueError):
                        call(0, between=between)
                for between in ((1.5, 2), ("1", 2), (True, 2)):
                    with pytest.raises(TypeError):
                        call(0, between=between)
                for field in (-1, 1024, 2**32, 2**64):
                    with pytest.raises(ValueError):
                        call(field, values=[b"a"])
                    with pytest.raises(ValueError):
                        call(field, between=(1, 2))
                for keywords in ({"delimiter": b"\n"}, {"delimiter": b",", "newline": b","}, {"delimiter": b"::"}, {"newline": b""},
                                 {"first": -1}, {"count": -1}, {"first": 2**64}, {"limit": -1}, {"seed": -1}, {"seed": 2**64}):
                    with pytest.raises(ValueError):
                        call(0, values=[b"a"], **keywords)
                    with pytest.raises(ValueError):
                        call(0, between=(None, None), **keywords)
            assert f.tell() == 0
    # the C calls refuse the same with MI355X_BZ2_ERR_INVALID_ARGUMENT, the reader's before it builds a line index
    lib = native.lib()
    N = native._native
    n, m, total = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    with native.open(PATH, parallelization=0) as f:
        handle = f._open_reader()._h
        good = N.value_set([b"a"])
        for nl, dl, field in ((10, 10, 0), (10, 9, 1024), (0, 0, 3), (10, 9, 2**32 - 1)):
            assert lib.mi355x_bz2_reader_field_matches(handle, nl, dl, field, *good, 0, 0, 0, 5, 5, 0, ctypes.byref(n), ctypes.byref(m)) \
                == INVALID_ARGUMENT
            assert b"field_matches" in lib.mi355x_bz2_reader_last_error(handle)
            assert lib.mi355x_bz2_reader_field_in_range(handle, nl, dl, field, 0, 0, 0, 0, 0, 0, 5, 5, 0, ctypes.byref(n), ctypes.byref(m)) \
                == INVALID_ARGUMENT
            assert b"field_in_range" in lib.mi355x_bz2_reader_last_error(handle)
            assert lib.mi355x_bz2_reader_select_lines(handle, nl, dl, field, *good, 0, 0, 0, 0, 0, 0, 0, 5, 5, 0, ctypes.byref(n),
                                                      ctypes.byref(total)) == INVALID_ARGUMENT
            assert b"select_lines" in lib.mi355x_bz2_reader_last_error(handle)
        for values, why in zip(BAD_VALUES, (b"1 to 1024 values, not 0", b"1 to 1024 values, not 1025", b"value 0 has 257 bytes",
                                            b"at most 16384 bytes in total, not 16385")):
            bad = N.value_set(values, check=False)
            if bad[2] > 0:      # a set of no values is select_lines' sign for a range
                assert lib.mi355x_bz2_reader_select_lines(handle, 10, 9, 0, *bad, 0, 0, 0, 0, 0, 0, 0, 5, 5, 0, ctypes.byref(n),
                                                          ctypes.byref(total)) == INVALID_ARGUMENT
                assert why in lib.mi355x_bz2_reader_last_error(handle)
            assert lib.mi355x_bz2_reader_field_matches(handle, 10, 9, 0, *bad, 0, 0, 0, 5, 5, 0, ctypes.byref(n), ctypes.byref(m)) \
                == INVALID_ARGUMENT
            assert why in lib.mi355x_bz2_reader_last_error(handle), lib.mi355x_bz2_reader_last_error(handle)
        # values and a range at once
        assert lib.mi355x_bz2_reader_select_lines(handle, 10, 9, 0, *good, 0, 1, 3, 0, 0, 0, 0, 5, 5, 0, ctypes.byref(n),
                                                  ctypes.byref(total)) == INVALID_ARGUMENT
        assert b"not both" in lib.mi355x_bz2_reader_last_error(handle)
        assert lib.mi355x_bz2_reader_take_field_matches(handle, None, 0, 0) == INVALID_ARGUMENT            # nothing is held
        assert b"no line numbers are held" in lib.mi355x_bz2_reader_last_error(handle)
        assert lib.mi355x_bz2_reader_take_field_matches(handle, None, 1, 0) == INVALID_ARGUMENT            # no destination
        assert lib.mi355x_bz2_reader_field_matches(handle, 10, 9, 0, *good, 0, 0, 0, 5, 5, 0, None, None) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_field_in_range(handle, 10, 9, 0, 0, 0, 0, 0, 0, 0, 5, 5, 0, None, None) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_select_lines(handle, 10, 9, 0, *good, 0, 0, 0, 0, 0, 0, 0, 5, 5, 0, None, None) == INVALID_ARGUMENT
        assert f.tell() == 0
        assert f.statistics()["blocks_decoded"] == 0
    assert lib.mi355x_bz2_match_fields(None, b"a", good[1], 1, 0, None, None, None, 0, 0, None) == INVALID_ARGUMENT


def test_help_lists_the_options(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    for option in (b"      --where-field arg ", b"      --equals arg ", b"      --in-file arg ", b"      --between arg ",
                   b"      --invert-match "):
        assert option in run.stdout, option
    assert b"ibzip2-mi355x --where-field 4 --between 500,599 --line-number file.tsv.bz2" in run.stdout
    assert b"not a CSV parser" in run.stdout and b"strtod" in run.stdout
    # what was there stays
    assert b"      --sum-by-field arg " in run.stdout and b"      --cut-fields arg " in run.stdout and b"      --grep arg " in run.stdout


def test_tool_refusals(native, tmp_path):
    """All refused before the input is opened: no GPU is needed."""
    def refused(options):
        run = subprocess.run([CLI] + options + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", options
        return run.stderr

    for other in (["--grep", "x"], ["--count-matches", "x"], ["--grep-file", PATH], ["--count-matches-file", PATH], ["--grep-regex", "x"],
                  ["--count-lines"], ["--line-hashes"], ["--count-distinct-lines"], ["--cut-field", "1"], ["--cut-fields", "1,2"],
                  ["--count-by-field", "1"], ["--sum-by-field", "0,1"]):
        stderr = refused(["--where-field", "0", "--equals", "x"] + other)
        assert b"cannot be combined with" in stderr, other
    for field in ("-1", "x", "", "1,2", "1024", "18446744073709551616", "0x10", " 1"):
        assert refused(["--where-field=" + field, "--equals", "x"]) == b"Bad value for --where-field\n", field
    needs_one = b"Option '--where-field' needs exactly one of '--equals', '--in-file' and '--between'\n"
    assert refused(["--where-field", "0"]) == needs_one
    assert refused(["--where-field", "0", "--equals", "x", "--between", "1,2"]) == needs_one
    assert refused(["--where-field", "0", "--equals", "x", "--in-file", PATH]) == needs_one
    assert refused(["--where-field", "0", "--invert-match"]) == needs_one
    needs_where = b"Options '--equals', '--in-file', '--between' and '--invert-match' need '--where-field'\n"
    for alone in (["--equals", "x"], ["--in-file", PATH], ["--between", "1,2"], ["--invert-match"]):
        assert refused(alone) == needs_where, alone
    for between in ("", "1", "1;2", "x,2", "1,y", "1.5,2", "1,2,3", " 1,2", "1, 2", "0x1,2", "1234567890123456789,", ",-1234567890123456789",
                    "--1,2", "+,2"):
        assert refused(["--where-field", "0", "--between=" + between]) == b"Bad value for --between\n", between
    assert refused(["--where-field", "0", "--equals", "v" * 257]) == b"Bad value for --equals: more than 256 bytes\n"
    assert refused(["--where-field", "0", "--in-file", str(tmp_path / "missing")]).startswith(b"Could not open the pattern file")
    empty = tmp_path / "empty"
    empty.write_bytes(b"")
    assert refused(["--where-field", "0", "--in-file", str(empty)]).endswith(b"holds no value\n")
    for delimiter in ("", "ab", "\n", "\\n", "\\x0a"):
        assert refused(["--where-field", "0", "--equals", "x", "--field-delimiter=" + delimiter]) == b"Bad value for --field-delimiter\n"
    assert refused(["--where-field", "0", "--equals", "x", "--seed", "x"]) == b"Bad value for --seed\n"
    run = subprocess.run([CLI, "--where-field"], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr.startswith(b"Option '--where-field' is missing an argument\n")
    # the messages that were there stay byte for byte
    assert refused(["--line-number"]) == b"Option '--line-number' needs '--grep' or '--grep-file'\n"
    assert refused(["--field-delimiter", ","]) == b"Option '--field-delimiter' needs '--cut-field'\n"
    assert refused(["--seed", "1"]) == b"Option '--seed' needs '--line-hashes' or '--count-distinct-lines'\n"
