"""Field columns on the CPU: the rule of indexed_bzip2_amd/csrc/bz2_fieldcols.hpp.

tests/native/fieldcols_cases.cpp runs under AddressSanitizer + UBSan as a program of its own.  The plain Python model of
fieldcols.py -- the column by bytes.split, and its own assembly from per-stretch packs, patches and fix-ups -- is compared
with bytes.split over random texts and cuts.  Then the bindings, the argument refusals (all before anything is launched:
no GPU is needed) and the tool's help and refusals."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES
import fieldcols as FC

HARNESS = os.path.join(ROOT, "tests", "native", "fieldcols_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
METHODS = ("read_columns", "read_columns_to_tensor")
INVALID_ARGUMENT = 103                                         # MI355X_BZ2_ERR_INVALID_ARGUMENT
SYMBOLS = ("gather_fields_tile_bytes", "gather_fields", "reader_field_columns", "reader_take_field_column")


def split_column(data, nl, dl, j):
    """The column straight from bytes.split, without fields.py."""
    lines = data.split(bytes([nl]))
    lines = lines[:-1] + ([lines[-1]] if lines[-1] else [])
    parts = [line.split(bytes([dl])) for line in lines]
    return [p[j] if j < len(p) else None for p in parts]


def test_known_answers_of_the_model():
    text = b"a\t12\t\n\n-7\n\t\t+3"
    assert FC.column(text, 10, 9, 0) == (b"a-7", [0, 1, 1, 3, 3], [1, 0, 2, 0])
    assert FC.column(text, 10, 9, 1) == (b"12", [0, 2, 2, 2, 2], [2, -1, -1, 0])
    assert FC.column(text, 10, 9, 2) == (b"+3", [0, 0, 0, 0, 2], [0, -1, -1, 2])
    assert FC.column(text, 10, 9, 1023) == (b"", [0] * 5, [-1] * 4)
    assert FC.column(b"", 10, 9, 0) == (b"", [0], [])
    assert FC.column(text, 10, 9, 0, 1, 2) == (b"-7", [0, 0, 2], [0, 2])
    assert FC.gathered(b"0123456789", [105, 2**64 - 1, 100, 109], [3, -1, 0, 1], base=100) == (4, [0, 3, 3, 3, 4], b"5679")
    # a line through three stretches: one fix-up, and the third stretch's pack from behind its first line on
    data = b"k,abcdefghij,x\nl,m\n"
    assert FC.assemble(data, [4, 9], 10, ord(","), 1) == (b"abcdefghijm", [(2, 10, 0)])
    assert FC.assemble(b"a,b\nc,tail", [], 10, ord(","), 1) == (b"btail", [(6, 4, 1)])


def test_model_against_bytes_split():
    """column and assemble over random texts, 0 to 6 random cuts, fields and windows of lines."""
    rng = random.Random(0xC01)
    fixed, windows = 0, 0
    for round_ in range(1500):
        nl = 0 if round_ % 5 == 0 else 10
        dl = (9, ord(","), 0xFF, 1)[round_ % 4]
        j = (0, 1, 2, 5, 1023)[round_ % 5 if round_ % 7 else rng.randrange(5)]
        alphabet = bytes([ord("a"), ord("b"), ord("q"), nl, dl, dl, 0xFE])
        data = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 140)))
        fields = split_column(data, nl, dl, j)
        blob, offsets, sizes = FC.column(data, nl, dl, j)
        assert sizes == [-1 if x is None else len(x) for x in fields]
        assert [blob[a:b] for a, b in zip(offsets, offsets[1:])] == [x or b"" for x in fields] and offsets[-1] == len(blob)
        cuts = [rng.randrange(len(data) + 1) for _ in range(rng.randrange(0, 7))]
        got, fixups = FC.assemble(data, cuts, nl, dl, j)
        assert got == blob, (data, nl, dl, j, cuts)
        fixed += len(fixups)
        assert all(got[at:at + size] == data[start:start + size] for start, size, at in fixups)
        first, count = rng.randrange(len(fields) + 2), rng.randrange(len(fields) + 2)
        got, _ = FC.assemble(data, cuts, nl, dl, j, first, count)
        assert got == b"".join(x or b"" for x in fields[first:first + count]), (data, nl, dl, j, cuts, first, count)
        assert FC.column(data, nl, dl, j, first, count)[0] == got
        windows += len(got)
    assert fixed > 500 and windows > 1000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fieldcols_under_sanitizers(tmp_path):
    exe = tmp_path / "fieldcols_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "fieldcols cases ok" in run.stdout


def test_bindings(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in SYMBOLS:
        assert "mi355x_bz2_" + name in names and callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays
    assert native._native.gather_fields_tile_bytes() == native.lib().mi355x_bz2_gather_fields_tile_bytes() == 16384
    assert callable(native.Decoder.gather_fields) and "k_field_gather" in native.Decoder.gather_fields.__doc__
    for cls in (native.reader._IndexedBzip2FileParallel, native.IndexedBzip2File):
        for method in METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
        assert "CSV" in native.reader._IndexedBzip2FileParallel.read_columns_to_tensor.__doc__
    for method in ("read_fields", "read_fields_to_tensor"):
        assert "read_columns" in getattr(native.reader._IndexedBzip2FileParallel, method).__doc__


def test_argument_refusals(native):
    """All refused before anything is launched: no GPU is needed."""
    for opened in (native.open(PATH, parallelization=0), native.IndexedBzip2File(PATH, parallelization=0)):
        with opened as f:
            for method in METHODS:
                call = getattr(f, method)
                for fields in ([], list(range(17)), [0] * 17, [-1], [1024], [0, 1024], [2**32], [0, 2**64]):
                    with pytest.raises(ValueError):
                        call(fields)
                for fields in ("1", b"12"):
                    with pytest.raises(TypeError):
                        call(fields)
                for newline in (b"\r\n", b"", "\n"):
                    with pytest.raises(ValueError):
                        call([0], newline=newline)
                for delimiter in (b"", b"::", "\t", None, b"\n"):
                    with pytest.raises(ValueError):
                        call([0], delimiter=delimiter)
                with pytest.raises(ValueError):
                    call([0], delimiter=b",", newline=b",")
                for first, count in ((-1, 1), (2**64, 1), (0, -1), (0, 2**64)):
                    with pytest.raises(ValueError):
                        call([0], first=first, count=count)
            assert f.tell() == 0
    # the C calls refuse the same with MI355X_BZ2_ERR_INVALID_ARGUMENT, the reader's before it builds a line index
    lib = native.lib()
    n, totals = ctypes.c_uint64(7), (ctypes.c_uint64 * 17)(*([7] * 17))
    with native.open(PATH, parallelization=0) as f:
        handle = f._open_reader()._h
        for nl, dl, fields in ((10, 9, []), (10, 9, list(range(17))), (10, 9, [1024]), (10, 9, [0, 3, 2**32 - 1]), (10, 10, [0]),
                               (0, 0, [3])):
            numbers = (ctypes.c_uint32 * max(1, len(fields)))(*fields)
            rc = lib.mi355x_bz2_reader_field_columns(handle, nl, dl, numbers, len(fields), 0, 5, 0, ctypes.byref(n), totals)
            assert rc == INVALID_ARGUMENT and n.value == 0, (nl, dl, fields)
            assert b"field_columns" in lib.mi355x_bz2_reader_last_error(handle)
            n.value = 7
        numbers = (ctypes.c_uint32 * 1)(0)
        assert lib.mi355x_bz2_reader_field_columns(handle, 10, 9, numbers, 1, 0, 5, 0, None, totals) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_field_columns(handle, 10, 9, numbers, 1, 0, 5, 0, ctypes.byref(n), None) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_field_columns(handle, 10, 9, None, 1, 0, 5, 0, ctypes.byref(n), totals) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_take_field_column(handle, 0, None, None, None, 0) == INVALID_ARGUMENT   # nothing is held
        assert f.tell() == 0
    total = ctypes.c_uint64()
    assert lib.mi355x_bz2_gather_fields(None, None, None, 0, 0, None, None, 0, ctypes.byref(total)) == INVALID_ARGUMENT


def test_help_lists_the_option(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --cut-fields arg " in run.stdout and b"cut -f1,4,6" in run.stdout and b"not a CSV parser" in run.stdout
    assert b"ibzip2-mi355x --cut-fields 0,3,5 file.tsv.bz2" in run.stdout
    # what was there stays
    assert b"      --cut-field arg " in run.stdout and b"ibzip2-mi355x --cut-field 2 file.tsv.bz2" in run.stdout
    assert b"      --sum-by-field arg " in run.stdout and b"      --count-by-field arg " in run.stdout


def test_tool_refusals(native):
    """All refused before the input is opened: no GPU is needed."""
    for other in (["--grep", "x"], ["--count-matches", "x"], ["--grep-file", PATH], ["--count-matches-file", PATH],
                  ["--grep-regex", "x"], ["--count-lines"], ["--line-hashes"], ["--count-distinct-lines"], ["--cut-field", "1"],
                  ["--count-by-field", "1"], ["--sum-by-field", "0,1"]):
        run = subprocess.run([CLI, "--cut-fields", "0,1"] + other + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", other
        assert run.stderr.startswith(b"Option '--cut-fields' cannot be combined with "), other
    for fields in ("", ",", "1,", ",1", "1,,2", "-1", "x", "1.5", "1024", "0,1024", "0,18446744073709551616", "0x10", " 1", "1, 2", "1;2",
                   ",".join(map(str, range(17))), ",".join(["0"] * 17)):
        run = subprocess.run([CLI, "--cut-fields=" + fields, PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", fields
        assert run.stderr == b"Bad value for --cut-fields\n", fields
    for delimiter in ("", "ab", "\n", "\\n", "\\x0a", "\\xg0"):
        run = subprocess.run([CLI, "--cut-fields", "0,1", "--field-delimiter=" + delimiter, PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"" and run.stderr == b"Bad value for --field-delimiter\n", delimiter
    run = subprocess.run([CLI, "--cut-fields"], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr.startswith(b"Option '--cut-fields' is missing an argument\n")
    # the messages that were there stay byte for byte
    run = subprocess.run([CLI, "--field-delimiter", ",", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr == b"Option '--field-delimiter' needs '--cut-field'\n"
