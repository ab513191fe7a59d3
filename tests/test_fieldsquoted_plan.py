"""Quoted field access on the CPU: the rule of indexed_bzip2_amd/csrc/bz2_fieldquote.hpp.

tests/native/fields_quoted_cases.cpp runs under AddressSanitizer + UBSan as a program of its own.  The plain Python model
of fieldsquoted.py is compared with known answers, its stitch with its definition over every cut of small texts and over
random cuts, its element composition with a walk, and its fields with Python's csv module.  Then the bindings, the
argument refusals (all before anything is launched: no GPU is needed) and the tool's help and refusals."""
import csv
import ctypes
import inspect
import io
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES
import fields as F
import fieldsquoted as Q
import readershapes as R
from fieldsquotedshapes import CAPS, KINDS, RUN, reader_corpus

HARNESS = os.path.join(ROOT, "tests", "native", "fields_quoted_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
READER_METHODS = ("field_spans", "field_spans_to_tensor", "read_fields", "read_fields_to_tensor", "read_columns",
                  "read_columns_to_tensor")
INVALID_ARGUMENT = 103                                         # MI355X_BZ2_ERR_INVALID_ARGUMENT
SYMBOLS = ("field_spans_quoted", "reader_field_spans_quoted", "reader_field_columns_quoted")
NL, DL, QT = 10, ord(","), ord('"')

# empty fields, "", """", a lone quote, an unbalanced quote followed by further lines, quotes next to delimiters, delimiters
# only inside quotes, a missing field, and an unterminated tail open inside a quote
TEXTS = (b"", b"\n", b"a,b,c\n", b",,\n,\n\n", b'"","""",x\n', b'",a,b\nc,d\n', b'a,"b,c",d\n"x\ny,z"\nlast,"open, tail',
         b'"a","b"\n",",",,"\nq"r,s"t\n', b'",,,,"\n"a,b"\n', b'one\n"two"\n,""\n', b'x,"y""z",""""\nw"')


def test_known_answers_of_the_model():
    text = b'a,"b,c",d\n"x\ny,z"\nlast,"open, tail'
    assert Q.raw_direct(text, NL, DL, QT, 0) == [(0, 1), (10, 2), (13, 1), (18, 4)]
    assert Q.raw_direct(text, NL, DL, QT, 1) == [(2, 5), (12, -1), (15, 2), (23, 11)]
    assert Q.raw_direct(text, NL, DL, QT, 2) == [(8, 1), (12, -1), (17, -1), (34, -1)]
    assert Q.direct(text, NL, DL, QT, 1) == [(3, 3), (12, -1), (15, 2), (23, 11)]
    assert Q.fields_of(text, NL, DL, QT, 1) == [b"b,c", None, b'z"', b'"open, tail']
    # the content rule: "x", "", a lone quote, "a, a", "a"b, """"
    line = b'"x","","\n"a\na"\n"a"b,""""\n'
    assert Q.fields_of(line, NL, DL, QT, 0) == [b"x", b'"a', b'a"', b'"a"b']
    assert Q.fields_of(line, NL, DL, QT, 1) == [b"", None, None, b'""']
    assert Q.fields_of(line, NL, DL, QT, 2) == [b'"', None, None, None]
    assert Q.direct(line, NL, DL, QT, 1)[0] == (5, 0)          # "" is the empty field one byte further on
    # without a quote byte in the text the fields are bytes.split's
    plain = b"a,b\n\n,c,,d\ne"
    for j in range(4):
        assert Q.direct(plain, NL, DL, QT, j) == F.direct(plain, NL, DL, j)
    # the model's quick way to part a line is the definition's loop
    rng = random.Random(3)
    for _ in range(2000):
        content = bytes(rng.choice(b'ab,,""') for _ in range(rng.randrange(30)))
        for inq in (0, 1):
            assert Q.parts_of(content, DL, QT, inq) == Q.parts_of_loop(content, DL, QT, inq), (content, inq)
    s = Q.summarise_chunk(text, NL, DL, QT, 1)
    assert s["head_positions"] == [[1, 7], [4]] and not s["head_quote_parity"]
    assert s["tail_in_quote"] and s["tail_delims"] == 1 and s["tail_field_start"] == 23 and s["tail_field_end"] is None


def test_model_stitch_over_every_cut_of_small_texts():
    for text in TEXTS:
        for j in (0, 1, 2, 3):
            want = Q.raw_direct(text, NL, DL, QT, j)
            n = len(text)
            for a in range(n + 1):
                for b in range(a, n + 1):
                    pieces = (text[:a], text[a:b], text[b:])
                    assert Q.stitch([Q.summarise_chunk(p, NL, DL, QT, j) for p in pieces], j) == want, (text, j, a, b)


def test_model_stitch_and_elements_over_random_cuts():
    rng = random.Random(0xC5F)
    for round_ in range(1500):
        nl = 0 if round_ % 5 == 0 else 10
        dl = (9, ord(","), 0xFF, 1)[round_ % 4]
        q = (ord('"'), ord("'"), 2)[round_ % 3]
        j = (0, 1, 2, 5, 1023)[round_ % 5]
        alphabet = bytes([ord("a"), ord("b"), nl, dl, dl, dl, q, q])
        data = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 100)))
        cuts = sorted([0, len(data)] + [rng.randrange(len(data) + 1) for _ in range(rng.randrange(0, 6))])
        summaries = [Q.summarise_chunk(data[a:b], nl, dl, q, j) for a, b in zip(cuts, cuts[1:])]
        assert Q.stitch(summaries, j) == Q.raw_direct(data, nl, dl, q, j), (data, nl, dl, q, j, cuts)
        whole = Q.summarise_chunk(data, nl, dl, q, j)
        assert whole["count"] == data.count(bytes([nl])) == len(whole["fields"])
        assert all(len(h) <= j + 1 for h in whole["head_positions"]) and whole["tail_delims"] <= j + 1
        # the element: both bracketings of a three-way split are the walk of the whole
        cap = (1, 2, 3, 5)[round_ % 4]
        a, b = sorted((rng.randrange(len(data) + 1), rng.randrange(len(data) + 1)))
        x, y, z = (Q.element_of(p, nl, dl, q, cap) for p in (data[:a], data[a:b], data[b:]))
        want = Q.element_of(data, nl, dl, q, cap)
        assert Q.compose(Q.compose(x, y, cap), z, cap) == want == Q.compose(x, Q.compose(y, z, cap), cap), (data, a, b, cap)


def test_model_field_1023_behind_1024_counted_delimiters():
    cells = [b'",,,,x,,"' if i % 100 == 7 else b"%c" % (97 + i % 3) for i in range(1024)] + [b'"the,last"']
    line = b",".join(cells) + b"\n"
    assert Q.fields_of(line, NL, DL, QT, 1023) == [cells[1023]] and Q.fields_of(line, NL, DL, QT, 7) == [b",,,,x,,"]
    assert cells[1023] == b"a" and len(Q.parts_of(line[:-1], DL, QT)) == 1025      # 1 024 delimiters count, more do not
    s = Q.summarise_chunk(line, NL, DL, QT, 1023)
    assert len(s["head_positions"][0]) == 1024 and len(s["head_positions"][1]) > 0
    for a in range(0, len(line), 211):
        pieces = (line[:a], line[a:])
        assert Q.stitch([Q.summarise_chunk(p, NL, DL, QT, 1023) for p in pieces], 1023) == Q.raw_direct(line, NL, DL, QT, 1023)


def test_model_equals_the_csv_module():
    """20 000 random rows written by csv.writer with a tab between fields, one line each: the model's fields are csv's
    values once a doubled quote is read as one."""
    rng = random.Random(20_000)
    alphabet = 'ab \t\t""\',;x'
    rows = [["".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 9))) for _ in range(rng.randrange(1, 7))]
            for _ in range(20_000)]
    out = io.StringIO()
    csv.writer(out, delimiter="\t", lineterminator="\n").writerows(rows)
    text = out.getvalue().encode()
    assert text.count(b"\n") == len(rows) and text.count(b'"') > 10_000 and b'""""' in text
    assert [[v.encode() for v in row] for row in csv.reader(io.StringIO(out.getvalue()), delimiter="\t")] == \
           [[v.encode() for v in row] for row in rows]
    for j in range(6):
        got = Q.fields_of(text, NL, 9, QT, j)
        want = [row[j].encode() if j < len(row) else None for row in rows]
        assert [None if g is None else g.replace(b'""', b'"') for g in got] == want, j


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_quoted_fields_under_sanitizers(tmp_path):
    exe = tmp_path / "fields_quoted_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "quoted fields cases ok" in run.stdout


def test_bindings(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in SYMBOLS:
        assert "mi355x_bz2_" + name in names and callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays
    assert ctypes.sizeof(native._native.QuotedFieldSummary) == 72 and ctypes.sizeof(native._native.FieldSummary) == 56
    for cls in (native.reader._IndexedBzip2FileParallel, native.IndexedBzip2File):
        for method in READER_METHODS:
            parameter = inspect.signature(getattr(cls, method)).parameters["quote"]
            assert parameter.kind is inspect.Parameter.KEYWORD_ONLY and parameter.default is None, (cls.__name__, method)
    assert inspect.signature(native.Decoder.field_spans).parameters["quote"].kind is inspect.Parameter.KEYWORD_ONLY
    # any bytes-like of one byte is a quote, for the reader and for the Decoder alike
    for quote in (b'"', bytearray(b'"'), memoryview(b'"')):
        assert native.reader._IndexedBzip2FileParallel._quote_argument(quote, 10, 9) == 34
    assert native.reader._IndexedBzip2FileParallel._quote_argument(None, 10, 9) is None
    doc = native.reader._IndexedBzip2FileParallel.field_spans.__doc__
    assert "quote=" in doc and "doubled" in doc and "cannot hold" in doc


def test_argument_refusals(native):
    """All refused before anything is launched: no GPU is needed."""
    for opened in (native.open(PATH, parallelization=0), native.IndexedBzip2File(PATH, parallelization=0)):
        with opened as f:
            for method in READER_METHODS:
                call = getattr(f, method)
                what = [0, 1] if "columns" in method else 0
                for quote in (b"", b'""', '"', 34, b"\n", b"\t"):
                    with pytest.raises(ValueError):
                        call(what, quote=quote)
                with pytest.raises(ValueError):
                    call(what, delimiter=b",", quote=b",")
                with pytest.raises(ValueError):
                    call(what, newline=b"\0", quote=b"\0")
                with pytest.raises(TypeError):
                    call(what, 0, None, b"\t", b"\n", b'"')                 # keyword only
                with pytest.raises(ValueError):
                    call([0, 1024] if "columns" in method else 1024, quote=b'"')
    # the C calls refuse the same with MI355X_BZ2_ERR_INVALID_ARGUMENT, the reader's before it builds a line index
    lib = native.lib()
    n = ctypes.c_uint64(7)
    fields = (ctypes.c_uint32 * 2)(0, 1)
    totals = (ctypes.c_uint64 * 2)()
    with native.open(PATH, parallelization=0) as f:
        handle = f._open_reader()._h
        for nl, dl, quote, field in ((10, 9, 10, 0), (10, 9, 9, 0), (10, 10, 34, 0), (10, 9, 34, 1024)):
            rc = lib.mi355x_bz2_reader_field_spans_quoted(handle, nl, dl, field, 0, 5, 0, ctypes.byref(n), quote)
            assert rc == INVALID_ARGUMENT and n.value == 0, (nl, dl, quote, field)
            assert b"field_spans" in lib.mi355x_bz2_reader_last_error(handle)
            fields[1] = field
            rc = lib.mi355x_bz2_reader_field_columns_quoted(handle, nl, dl, fields, 2, 0, 5, 0, ctypes.byref(n), totals, quote)
            assert rc == INVALID_ARGUMENT and n.value == 0, (nl, dl, quote, field)
        assert lib.mi355x_bz2_reader_take_field_spans(handle, None, None, 0, 0) == INVALID_ARGUMENT      # nothing is held
        assert f.tell() == 0
    assert lib.mi355x_bz2_field_spans_quoted(None, None, 0, 10, 9, 34, 0, None, None, None, None, 0) == INVALID_ARGUMENT


def test_help_lists_the_option(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --field-quote arg " in run.stdout and b"doubled quotes inside stay doubled" in run.stdout
    assert b"      --cut-field arg " in run.stdout and b"      --field-delimiter arg " in run.stdout


def test_tool_refusals(native):
    """All refused before the input is opened: no GPU is needed."""
    run = subprocess.run([CLI, "--field-quote", '"', PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b""
    assert run.stderr == b"Option '--field-quote' needs '--cut-field' or '--cut-fields' and no other field option\n"
    for other in (["--count-by-field", "0"], ["--sum-by-field", "0,1"], ["--where-field", "0", "--equals", "x"]):
        run = subprocess.run([CLI, "--field-quote", '"'] + other + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", other
        assert run.stderr == b"Option '--field-quote' needs '--cut-field' or '--cut-fields' and no other field option\n", other
    for quote in ("", "ab", "\n", "\\n", "\\x0a", "\\xg0", "\\t"):     # the last one is the default delimiter
        run = subprocess.run([CLI, "--cut-field", "0", "--field-quote=" + quote, PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", quote
        assert run.stderr == b"Bad value for --field-quote\n", quote
    run = subprocess.run([CLI, "--cut-fields", "0,1", "--field-delimiter", ",", "--field-quote", ",", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr == b"Bad value for --field-quote\n"


def test_the_corpus_plants_what_it_says():
    """On the CPU: every planted case lies on a launch boundary of its cap, and the run inside a quoted field."""
    for variant in ("tail", "closed"):
        raw, enc, planted, run_at, parts = reader_corpus(variant)
        starts = R.data_block_starts(parts)
        kinds = {(cap, planted[b]) for cap in CAPS for b in R.boundaries_of(starts, cap) if b in planted}
        assert {(cap, kind) for cap in CAPS for kind in KINDS} <= kinds
        for b, kind in planted.items():
            first = raw.rfind(b"\n", 0, b) + 1
            state = raw[first:b].count(b'"') % 2                    # the quote state in front of the byte at b
            if kind == "behind-open":
                assert raw[b - 1] == QT and state == 1 and raw[b - 2] == DL
            elif kind == "before-close":
                assert raw[b] == QT and state == 1 and raw[b + 1] == DL
            elif kind == "in-doubled":
                assert raw[b - 1:b + 1] == b'""' and state == 0 and raw[first:b - 1].count(b'"') % 2 == 1
            else:
                assert raw[b] == DL and state == 1
        assert set(range(run_at, run_at + RUN)) <= set(starts)
        first = raw.rfind(b"\n", 0, run_at) + 1
        assert raw[first:run_at].count(b'"') == 1 and raw[first:run_at + RUN].count(b'"') == 1
        assert b"\n" not in raw[run_at - 2_000:run_at + 2_000]
        last = raw[raw.rfind(b"\n", 0, len(raw) - 1) + 1:]
        assert last.count(b'"') == 1                                # the last line is open inside a quote
        assert (raw[-1] == NL) == (variant == "closed")
        # quoting matters in this file
        assert sum(a != b for a, b in zip(Q.direct(raw, NL, DL, QT, 2), F.direct(raw, NL, DL, 2))) > 100
