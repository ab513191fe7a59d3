"""Lines selected by a regular expression on a field, on the CPU: the definition of
indexed_bzip2_amd/csrc/bz2_fieldregex.hpp.

The plain Python model of fieldregex.py is checked against Python's `re` on the fields of a seeded corpus;
tests/native/fieldregex_cases.cpp runs fieldRegexHolds, regexDeadState and the early stop under AddressSanitizer + UBSan as
a program of its own, over the same patterns and fields.  Then the bindings, the argument refusals (all before anything is
launched: no GPU is needed), the tool's help and refusals, and the condition under which the GPU test cannot pass with the
reader's host path dead: its pattern list selects some lines that cross a launch seam, and the tail, and leaves others."""
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, FIXTURES
import columnshapes as C
import fieldregex as FR
import regexgen as G

HARNESS = os.path.join(ROOT, "tests", "native", "fieldregex_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
METHODS = ("where_field", "where_field_to_tensor", "count_where_field", "select_lines", "select_lines_to_tensor")
SYMBOLS = ("match_fields_regex", "reader_field_matches_regex", "reader_select_lines_regex")
INVALID_ARGUMENT = 103                                         # MI355X_BZ2_ERR_INVALID_ARGUMENT
SEED = 0xD1CE                                                  # of the 300 random patterns: test_regex_plan.py compiles them all


def corpus_fields():
    """The fields of regexgen.random_corpus split at b",": none holds the byte 0x0A."""
    fields = sorted({field for line in G.random_corpus(0x5EED) for field in line.split(b",")})
    assert b"" in fields and len(fields) > 150 and not any(b"\n" in field for field in fields)
    return fields


def random_patterns():
    rng = random.Random(SEED)
    return [(G.random_pattern(rng), rng.randrange(2) == 1) for _ in range(300)]


def all_patterns():
    return [(pattern, fold) for pattern in G.FIXED_PATTERNS for fold in (False, True)] + random_patterns()


def test_the_model_against_re(native):
    """fields_of + table_matches equals re.search(pattern, field, re.DOTALL [| re.IGNORECASE]) on every field."""
    fields = corpus_fields()
    lines = [b",".join(G.random_corpus(0x5EED)[k:k + 3]) for k in range(0, 399, 3)] + [b"", b",", b"a,,b"]
    data = b"\n".join(lines) + b"\n"
    dead = 0
    for pattern, fold in all_patterns():
        regex = native.compile_regex(pattern, fold)
        for field in fields:
            assert FR.field_matches(regex, field) == FR.by_re(pattern, field, fold), (pattern, fold, field)
        assert FR.field_matches(regex, None) is False
        dead += FR.dead_state(regex) is not None
    assert 20 < dead < len(all_patterns())
    # through fields_of: the line's field j, a missing field never, an empty one iff the pattern matches the empty string
    for pattern, j in ((rb"^a", 0), (rb"b$", 1), (rb"^$", 2), (rb"a*", 2), (rb"[^a]", 3)):
        regex = native.compile_regex(pattern)
        want = [len(line.split(b",")) > j and re_search(pattern, line.split(b",")[j]) for line in lines]
        assert FR.flags_of_data(regex, data, 10, ord(","), j) == want, (pattern, j)
    empty = native.compile_regex(rb"^$")
    assert FR.flags_of_data(empty, b"a,\n,\nb\n", 10, ord(","), 1) == [True, True, False]


def re_search(pattern, field):
    import re
    return re.search(pattern, field, re.DOTALL) is not None


def test_known_dead_states(native):
    assert FR.dead_state(native.compile_regex(rb"^GET")) is not None
    assert FR.dead_state(native.compile_regex(rb"GET")) is None
    assert FR.dead_state(native.compile_regex(rb"^$")) is not None
    assert FR.dead_state(native.compile_regex(rb"a*")) is None
    assert FR.dead_state(native.compile_regex(rb"^a|b$")) is None and FR.dead_state(native.compile_regex(rb"^a")) is not None


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fieldregex_under_sanitizers(tmp_path):
    """The program's own cases, then regexgen's patterns over the corpus' fields, handed in as a file of records."""
    exe = tmp_path / "fieldregex_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    records = tmp_path / "records.bin"
    patterns, fields = all_patterns(), corpus_fields()
    with open(records, "wb") as out:
        for pattern, fold in patterns:
            out.write((b"I" if fold else b"P") + struct.pack("<I", len(pattern)) + pattern)
        for field in fields:
            out.write(b"F" + struct.pack("<I", len(field)) + field)
    for arguments in ([], [str(records)]):
        run = subprocess.run([str(exe)] + arguments, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        assert "fieldregex cases ok" in run.stdout
    # nothing was skipped: every pattern handed in compiled, beside the program's own 34
    assert "%d patterns compiled, 0 refused" % (34 + len(patterns)) in run.stdout, run.stdout


def test_bindings(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in SYMBOLS:
        assert "mi355x_bz2_" + name in names and callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays
    import inspect
    for cls in (native.reader._IndexedBzip2FileParallel, native.IndexedBzip2File):
        for method in METHODS:
            parameters = inspect.signature(getattr(cls, method)).parameters
            for name, default in (("regex", None), ("ignore_case", False)):
                assert parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and parameters[name].default is default, (method, name)
    doc = native.reader._IndexedBzip2FileParallel.where_field.__doc__
    assert "regex" in doc and "trailing" in doc and "re.DOTALL" in doc          # where Python's `$` differs is said
    assert callable(native.Decoder.match_fields_regex) and "k_field_regex" in native.Decoder.match_fields_regex.__doc__


def test_argument_refusals(native):
    """All refused before anything is launched: no GPU is needed."""
    plain = native.compile_regex(rb"get")
    for opened in (native.open(PATH, parallelization=0), native.IndexedBzip2File(PATH, parallelization=0)):
        with opened as f:
            for method in METHODS:
                call = getattr(f, method)
                # two of the three predicates, or none
                for two in (dict(values=[b"a"], regex=b"a"), dict(between=(1, 2), regex=b"a"), dict(values=[b"a"], between=(1, 2)),
                            dict(values=[b"a"], between=(1, 2), regex=b"a")):
                    with pytest.raises(ValueError) as refused:
                        call(0, **two)
                    assert "exactly one of" in str(refused.value)
                with pytest.raises(ValueError) as refused:
                    call(0)
                assert str(refused.value) == "exactly one of values and between must be given"       # the words it has today
                # regex and ignore_case are keyword only
                with pytest.raises(TypeError):
                    call(0, None, None, False, 0, None, None, b"\t", b"\n", 0, b"a")
                # ignore_case without regex; with a compiled object that does not fold
                for how in (dict(ignore_case=True), dict(values=[b"a"], ignore_case=True), dict(between=(1, 2), ignore_case=True)):
                    with pytest.raises(ValueError):
                        call(0, **how)
                with pytest.raises(ValueError) as refused:
                    call(0, regex=plain, ignore_case=True)
                assert "compile_regex" in str(refused.value)
                # the compiler's refusals, with its words
                with pytest.raises(ValueError) as refused:
                    call(0, regex=rb"(a)\1")
                assert "back-reference" in str(refused.value)
                for pattern, word in G.REFUSED[1:8]:
                    with pytest.raises(ValueError) as refused:
                        call(0, regex=pattern)
                    assert word in str(refused.value), pattern
                with pytest.raises(TypeError):
                    call(0, regex="text")
                # the other arguments are refused as they are for the other predicates
                for field in (-1, 1024, 2**32):
                    with pytest.raises(ValueError):
                        call(field, regex=b"a")
                for keywords in ({"delimiter": b"\n"}, {"delimiter": b",", "newline": b","}, {"newline": b""}, {"first": -1},
                                 {"count": -1}, {"limit": -1}):
                    with pytest.raises(ValueError):
                        call(0, regex=b"a", **keywords)
            assert f.tell() == 0
    # the C calls: null arguments, and the field arguments before a line index is built
    import ctypes
    lib = native.lib()
    n, m = ctypes.c_uint64(7), ctypes.c_uint64(7)
    with native.open(PATH, parallelization=0) as f:
        handle = f._open_reader()._h
        for nl, dl, field in ((10, 10, 0), (10, 9, 1024), (0, 0, 3)):
            assert lib.mi355x_bz2_reader_field_matches_regex(handle, nl, dl, field, plain._h, 0, 0, 5, 5, 0, ctypes.byref(n),
                                                             ctypes.byref(m)) == INVALID_ARGUMENT
            assert b"field_matches_regex" in lib.mi355x_bz2_reader_last_error(handle)
            assert lib.mi355x_bz2_reader_select_lines_regex(handle, nl, dl, field, plain._h, 0, 0, 5, 5, 0, ctypes.byref(n),
                                                            ctypes.byref(m)) == INVALID_ARGUMENT
            assert b"select_lines_regex" in lib.mi355x_bz2_reader_last_error(handle)
        assert lib.mi355x_bz2_reader_field_matches_regex(handle, 10, 9, 0, None, 0, 0, 5, 5, 0, ctypes.byref(n), ctypes.byref(m)) \
            == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_field_matches_regex(handle, 10, 9, 0, plain._h, 0, 0, 5, 5, 0, None, None) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_select_lines_regex(handle, 10, 9, 0, None, 0, 0, 5, 5, 0, ctypes.byref(n), ctypes.byref(m)) \
            == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_select_lines_regex(handle, 10, 9, 0, plain._h, 0, 0, 5, 5, 0, None, None) == INVALID_ARGUMENT
        assert f.tell() == 0 and f.statistics()["blocks_decoded"] == 0
    assert lib.mi355x_bz2_match_fields_regex(None, plain._h, None, None, 0, 0, None) == INVALID_ARGUMENT


def test_help_lists_the_option(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --matches arg " in run.stdout and b"--where-field 6 --matches '^/api/v[0-9]' file.tsv.bz2" in run.stdout
    # what was there stays
    for option in (b"      --where-field arg ", b"      --equals arg ", b"      --in-file arg ", b"      --between arg ",
                   b"      --invert-match ", b"      --ignore-case ", b"      --grep-regex arg "):
        assert option in run.stdout, option


def test_tool_refusals(native):
    """All refused before the input is opened: no GPU is needed."""
    def refused(options):
        run = subprocess.run([CLI] + options + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", options
        return run.stderr

    needs_one = b"Option '--where-field' needs exactly one of '--equals', '--in-file', '--between' and '--matches'\n"
    assert refused(["--where-field", "0", "--matches", "x", "--equals", "x"]) == needs_one
    assert refused(["--where-field", "0", "--matches", "x", "--between", "1,2"]) == needs_one
    assert refused(["--where-field", "0", "--matches", "x", "--in-file", PATH]) == needs_one
    assert refused(["--matches", "x"]) == b"Option '--matches' needs '--where-field'\n"
    # --ignore-case within --where-field: with --matches only
    for other in (["--equals", "x"], ["--between", "1,2"]):
        assert refused(["--where-field", "0", "--ignore-case"] + other).startswith(b"Option '--ignore-case' needs ")
    # a refused pattern prints the compiler's sentence
    for pattern, word in ((r"(a)\1", b"back-reference"), ("a(?=b)", b"look-around"), ("(a", b"unbalanced"), ("", b"empty pattern")):
        stderr = refused(["--where-field", "0", "--matches=" + pattern])
        assert stderr.startswith(b"Invalid regular expression: ") and word in stderr, pattern
        assert word in refused(["--where-field", "0", "--matches=" + pattern, "--ignore-case", "--invert-match"])
    for other in (["--grep", "x"], ["--grep-regex", "x"], ["--count-lines"], ["--cut-field", "1"]):
        assert b"cannot be combined with" in refused(["--where-field", "0", "--matches", "x"] + other), other
    run = subprocess.run([CLI, "--where-field", "0", "--matches"], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr.startswith(b"Option '--matches' is missing an argument\n")
    # the messages that were there stay byte for byte
    assert refused(["--where-field", "0"]) == b"Option '--where-field' needs exactly one of '--equals', '--in-file' and '--between'\n"
    assert refused(["--ignore-case"]).startswith(b"Option '--ignore-case' needs '--grep', '--grep-file', '--count-matches' or ")


def test_the_pattern_list_reaches_the_seams_and_the_tail(native):
    """On columnshapes.corpus("tail"): for each of the caps 2, 3 and 5 the list selects a line that crosses a planted launch
    boundary through a field of at least one byte -- so that its bytes must be fetched and decided on the host --, and
    leaves another; the tail is selected by one pattern and left by another."""
    e = C.expected("tail")
    raw, starts, newlines = e["raw"], e["block_starts"], e["newlines"]
    assert not raw.endswith(b"\n")
    tail = len(e["lines"]) - 1
    assert {name for name, _, _, _ in FR.PATTERNS} >= {"get", "k-keys"} and len({name for name, _, _, _ in FR.PATTERNS}) == len(FR.PATTERNS)
    flags = {}
    for name, j, pattern, fold in FR.PATTERNS:
        assert j in FR.FIELDS
        flags[name] = FR.flags_of(native.compile_regex(pattern, fold), e["fields"][j])
        assert 0 < sum(flags[name]), name                              # every pattern selects something
    for cap in C.PLANT_CAPS:
        boundaries = [b for b in C.boundaries_of(starts, cap) if b in C.planted()[0] and raw[b - 1:b] != b"\n"]
        lines = sorted({int(np.searchsorted(newlines, b, "left")) for b in boundaries})
        assert len(lines) >= 8, cap
        selected = {(name, line) for name, j, _, _ in FR.PATTERNS for line in lines if flags[name][line] and e["fields"][j][line]}
        left = {(name, line) for name, j, _, _ in FR.PATTERNS for line in lines if not flags[name][line] and e["fields"][j][line]}
        print("cap", cap, len(lines), "seam lines,", len(selected), "selections,", len(left), "left")
        assert len({line for _, line in selected}) >= 3 and len({line for _, line in left}) >= 3, cap
        # the key that the boundary cuts: GE|T is selected, GET|S is not
        assert any(flags["get"][line] for line in lines) and any(not flags["get"][line] for line in lines), cap
    assert flags["get"][tail] and flags["end"][tail] and not flags["k-keys"][tail] and not flags["empty"][tail]
