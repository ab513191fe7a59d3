"""Field access on the CPU: the summaries and the stitching rule of indexed_bzip2_amd/csrc/bz2_fields.hpp.

tests/native/fields_cases.cpp runs under AddressSanitizer + UBSan as a program of its own.  The plain Python model of
fields.py -- its summarise and stitch -- is compared with the direct definition, bytes.split per line, over random cuts
and chunk sizes 1 to 64.  Then the bindings, the argument refusals (all before anything is launched: no GPU is needed)
and the tool's help and refusals."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES
import fields as F

HARNESS = os.path.join(ROOT, "tests", "native", "fields_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
READER_METHODS = ("field_spans", "field_spans_to_tensor", "read_fields", "read_fields_to_tensor")
INVALID_ARGUMENT = 103                                         # MI355X_BZ2_ERR_INVALID_ARGUMENT
SYMBOLS = ("field_chunk_bytes", "field_spans", "reader_field_spans", "reader_take_field_spans")


def test_known_answers_of_the_model():
    text = b"a\tbc\t\n\nx\n\t\ty"
    assert F.lines_of(text, 10) == [b"a\tbc\t", b"", b"x", b"\t\ty"]
    assert F.direct(text, 10, 9, 0) == [(0, 1), (6, 0), (7, 1), (9, 0)]
    assert F.direct(text, 10, 9, 1) == [(2, 2), (6, -1), (8, -1), (10, 0)]
    assert F.direct(text, 10, 9, 2) == [(5, 0), (6, -1), (8, -1), (11, 1)]
    assert F.direct(text, 10, 9, 3) == [(5, -1), (6, -1), (8, -1), (12, -1)]
    assert F.fields_of(text, 10, 9, 1) == [b"bc", None, None, b""]
    assert F.direct(b"", 10, 9, 0) == [] and F.direct(b"\n", 10, 9, 0) == [(0, 0)] and F.direct(b"\n", 10, 9, 1) == [(0, -1)]
    # every present field is what split gives
    for j in range(4):
        for (start, size), field in zip(F.direct(text, 10, 9, j), F.fields_of(text, 10, 9, j)):
            assert (field is None and size == -1) or text[start:start + size] == field


def test_model_summaries_and_stitching():
    """summarise / stitch against the direct definition: random inputs over a small alphabet that holds nl, dl, 0 and
    0xFF, 0 to 6 random cuts, every stretch summarised with a chunk size of its own between 1 and 64."""
    rng = random.Random(0xF1E1D)
    for round_ in range(1000):
        nl = 0 if round_ % 5 == 0 else 10
        dl = (9, ord(","), 0xFF, 1)[round_ % 4]
        j = (0, 1, 2, 5, 1023)[round_ % 5 if round_ % 7 else rng.randrange(5)]
        alphabet = bytes([ord("a"), ord("b"), nl, dl, dl, 0, 0xFF])
        data = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 120)))
        want = F.direct(data, nl, dl, j)
        cuts = sorted([0, len(data)] + [rng.randrange(len(data) + 1) for _ in range(rng.randrange(0, 7))])
        summaries = [F.summarise(data[a:b], nl, dl, j, rng.randrange(1, 65)) for a, b in zip(cuts, cuts[1:])]
        assert F.stitch(summaries, j) == want, (data, nl, dl, j, cuts)
        # a summary does not depend on the chunk size
        whole = F.summarise_chunk(data, nl, dl, j)
        for chunk in (1, 2, 3, 7, 64):
            assert F.summarise(data, nl, dl, j, chunk) == whole, (data, nl, dl, j, chunk)
        assert whole["count"] == data.count(bytes([nl])) == len(whole["fields"])
        assert len(whole["head_positions"]) <= j + 1 and whole["tail_delims"] <= j + 1
        # and the fields' bytes are split's
        for (start, size), field in zip(want, F.fields_of(data, nl, dl, j)):
            assert (field is None and size == -1) or data[start:start + size] == field


def test_model_saturation_and_a_field_across_stretches():
    line = b"".join(b"%c," % (97 + i % 3) for i in range(3000)) + b"\n"
    for j in (0, 1, 255, 256, 1023):
        for chunk in (1, 5, 256):
            s = F.summarise(line, 10, ord(","), j, chunk)
            assert len(s["head_positions"]) == j + 1 and s["fields"] == [(2 * j, 1)] and s["tail_delims"] == 0
    pieces = [b"x\nab,c", b"d,efg", b"hij", b"kl,m", b"no\nq,r"]
    text = b"".join(pieces)
    for j in range(5):
        got = F.stitch([F.summarise(p, 10, ord(","), j, 2) for p in pieces], j)
        assert got == F.direct(text, 10, ord(","), j)
    assert F.direct(text, 10, ord(","), 2) == [(1, -1), (8, 8), (24, -1)]
    # from a line start that is not offset 0, beyond 2^32
    assert F.stitch([F.summarise(p, 10, ord(","), 2, 3) for p in pieces], 2, offset=2**33) == [(2**33 + 1, -1), (2**33 + 8, 8), (2**33 + 24, -1)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fields_under_sanitizers(tmp_path):
    exe = tmp_path / "fields_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "fields cases ok" in run.stdout


def test_bindings(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in SYMBOLS:
        assert "mi355x_bz2_" + name in names and callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays
    assert native._native.field_chunk_bytes() == native.lib().mi355x_bz2_field_chunk_bytes() == 256
    assert ctypes.sizeof(native._native.FieldSummary) == 56
    for cls in (native.reader._IndexedBzip2FileParallel, native.IndexedBzip2File):
        for method in READER_METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
    assert callable(native.Decoder.field_spans)
    assert "CSV" in native.reader._IndexedBzip2FileParallel.field_spans.__doc__
    assert "CSV" in native.reader._IndexedBzip2FileParallel.read_fields.__doc__


def test_argument_refusals(native):
    """All refused before anything is launched: no GPU is needed."""
    for opened in (native.open(PATH, parallelization=0), native.IndexedBzip2File(PATH, parallelization=0)):
        with opened as f:
            for method in READER_METHODS:
                call = getattr(f, method)
                for field in (-1, 1024, 2**32, 2**64):
                    with pytest.raises(ValueError):
                        call(field)
                for newline in (b"\r\n", b"", "\n"):
                    with pytest.raises(ValueError):
                        call(0, newline=newline)
                for delimiter in (b"", b"::", "\t", None):
                    with pytest.raises(ValueError):
                        call(0, delimiter=delimiter)
                with pytest.raises(ValueError):
                    call(0, delimiter=b"\n")
                with pytest.raises(ValueError):
                    call(0, delimiter=b",", newline=b",")
                for first, count in ((-1, 1), (2**64, 1), (0, -1), (0, 2**64)):
                    with pytest.raises(ValueError):
                        call(0, first, count)
    # the C calls refuse the same with MI355X_BZ2_ERR_INVALID_ARGUMENT, the reader's before it builds a line index
    lib = native.lib()
    n = ctypes.c_uint64(7)
    with native.open(PATH, parallelization=0) as f:
        handle = f._open_reader()._h
        for nl, dl, field in ((10, 10, 0), (10, 9, 1024), (0, 0, 3), (10, 9, 2**32 - 1)):
            rc = lib.mi355x_bz2_reader_field_spans(handle, nl, dl, field, 0, 5, 0, ctypes.byref(n))
            assert rc == INVALID_ARGUMENT and n.value == 0, (nl, dl, field)
            assert b"field_spans" in lib.mi355x_bz2_reader_last_error(handle)
        assert lib.mi355x_bz2_reader_take_field_spans(handle, None, None, 0, 0) == INVALID_ARGUMENT      # nothing is held
        assert f.tell() == 0
    assert lib.mi355x_bz2_field_spans(None, None, 0, 10, 9, 0, None, None, None, None, 0) == INVALID_ARGUMENT


def test_help_lists_the_options(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --cut-field arg " in run.stdout and b"      --field-delimiter arg " in run.stdout
    assert b"not a CSV parser" in run.stdout
    assert b"ibzip2-mi355x --cut-field 2 file.tsv.bz2" in run.stdout


def test_tool_refusals(native):
    """All refused before the input is opened: no GPU is needed."""
    run = subprocess.run([CLI, "--field-delimiter", ",", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b""
    assert run.stderr == b"Option '--field-delimiter' needs '--cut-field'\n"
    for other in (["--grep", "x"], ["--count-matches", "x"], ["--grep-file", PATH], ["--count-matches-file", PATH],
                  ["--grep-regex", "x"], ["--count-lines"], ["--line-hashes"], ["--count-distinct-lines"]):
        run = subprocess.run([CLI, "--cut-field", "1"] + other + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", other
        assert run.stderr.startswith(b"Option '--cut-field' cannot be combined with "), other
    for field in ("-1", "x", "", "1.5", "1024", "18446744073709551616", "0x10", " 1"):
        run = subprocess.run([CLI, "--cut-field=" + field, PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", field
        assert run.stderr == b"Bad value for --cut-field\n", field
    for delimiter in ("", "ab", "\n", "\\n", "\\x0a", "\\x0A", "\\xg0", "\\x1", "\\t\\t"):
        run = subprocess.run([CLI, "--cut-field", "0", "--field-delimiter=" + delimiter, PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", delimiter
        assert run.stderr == b"Bad value for --field-delimiter\n", delimiter
