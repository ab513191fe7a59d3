"""grep_regex on the CPU: the compiler and the summaries of indexed_bzip2_amd/csrc/bz2_regex.hpp.

tests/native/regex_cases.cpp runs under AddressSanitizer + UBSan as a program of its own.  Through compile_regex (which
needs no GPU) the compiled table is simulated in Python and compared with Python's re -- re.search(p, line, re.DOTALL
[| re.IGNORECASE]) is the reference, never the code under test -- on every line of dolorem-ipsum.txt and of a seeded
corpus over a small alphabet, for the fixed pattern list of regexgen.py and 300 seeded random patterns; the model of
regexgen.py (summarise, stitch) is driven with the same tables over random cuts.  Then the refusals, the two caps, the
flag bits, the bindings and the tool's option."""
import ctypes
import inspect
import os
import random
import re
import shutil
import subprocess
import time

import pytest

from conftest import ROOT, FIXTURES
import regexgen as G

HARNESS = os.path.join(ROOT, "tests", "native", "regex_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
READER_METHODS = ("grep_regex", "count_matching_lines_regex", "grep_regex_to_tensor")
SYMBOLS = ("regex_compile", "regex_free", "regex_states", "regex_table", "regex_chunk_bytes", "match_lines", "reader_grep_regex")


@pytest.fixture(scope="module")
def lines():
    with open(os.path.join(FIXTURES, "dolorem-ipsum.txt"), "rb") as f:
        text = f.read()
    extra = [b"GET /a/b HTTP/1.1", b"POST / HTTP/1.0", b"GET /A HTTP/1.1", b"2024-01-02 boot ERROR disk", b"2024-1-02 FATAL",
             b"10.0.0.255 up", b"1.2.3", b"a,x", b"x,b", b"x", b"\xe9t\xe9", b"caf\xc9 \xc9T\xc9", b"a\x00b", b"me@example.com",
             b"xaybzc", b"}x ]y [] {}", b"a\tb", b"ends with a dot.", b"Error", b"WARNING: fatal", b"a-b", b"aab ab b"]
    return [content for _, content in G.split_lines(text)] + G.random_corpus(0x5EED) + extra


def check_against_re(native, pattern, ignore_case, lines):
    compiled = native.compile_regex(pattern, ignore_case)          # a ValueError here fails the test: nothing is skipped
    assert 2 <= compiled.states <= 64
    assert compiled.transitions.shape == (compiled.states, 256) and compiled.accepts_at_end.shape == (compiled.states,)
    transitions, accepts = compiled.transitions.tolist(), compiled.accepts_at_end.tolist()
    reference = re.compile(pattern, G.reference_flags(ignore_case))
    for line in lines:
        assert G.table_matches(transitions, accepts, line) == bool(reference.search(line)), (pattern, ignore_case, line)
    # the two fixed states: A is absorbing and accepts, nothing leads back to the start
    assert all(target == G.MATCHED for target in transitions[G.MATCHED]) and accepts[G.MATCHED] == 1
    assert all(target != G.START for row in transitions for target in row)
    return compiled


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_regex_under_sanitizers(tmp_path):
    exe = tmp_path / "regex_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "regex ok" in run.stdout


def test_fixed_patterns_against_re(native, lines):
    assert len(G.FIXED_PATTERNS) >= 40
    for required in (rb"a*", rb"^$", rb"a^b", rb"$a", rb"(^|,)x(,|$)", rb"[^a]", rb"a{,2}b"):
        assert required in G.FIXED_PATTERNS
    assert any(re.search(rb"\\x[89a-f][0-9a-f]", p) for p in G.FIXED_PATTERNS)
    for pattern in G.FIXED_PATTERNS:
        for ignore_case in (False, True):
            check_against_re(native, pattern, ignore_case, lines)
    # the state counts that the design quotes
    assert [native.compile_regex(p).states for p in (rb"error", rb"(error|warning|fatal)", rb"\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}",
                                                    rb"^(GET|POST) /[a-z/]* HTTP/1\.[01]$")] == [7, 17, 13, 19]
    # a pattern that matches the empty string: the start accepts at the end and every byte leads it to A
    empty = native.compile_regex(rb"a*")
    assert empty.accepts_at_end[0] == 1 and set(empty.transitions[0].tolist()) == {G.MATCHED}
    # [^a] does not match A when case is ignored
    folded = native.compile_regex(rb"[^a]", ignore_case=True)
    assert folded.ignore_case and not G.table_matches(folded.transitions.tolist(), folded.accepts_at_end.tolist(), b"aA")


def test_random_patterns_against_re(native, lines):
    rng = random.Random(0xD1CE)
    sample = lines[::7] + lines[-40:]
    for _ in range(300):
        pattern = G.random_pattern(rng)
        check_against_re(native, pattern, rng.randrange(2) == 1, sample)


def test_model_of_the_summaries_against_re(native):
    """summarise and stitch of regexgen.py (the mirror of bz2_regex.hpp's, and the device tests' prediction) with compiled
    tables: random texts, random cuts, chunk sizes 1 to 64 -- one offset inside every matching line, ascending."""
    rng = random.Random(0xC0FFEE)
    patterns = [rb"ab", rb"a*", rb"^$", rb"^a+$", rb"a^b", rb"b$", rb"^b", rb"(^|a)b(a|$)", rb"[^a]", rb"b.*a"]
    tables = {}
    for pattern in patterns:
        for ignore_case in (False, True):
            compiled = native.compile_regex(pattern, ignore_case)
            tables[pattern, ignore_case] = (compiled.transitions.tolist(), compiled.accepts_at_end.tolist())
    for _ in range(600):
        pattern, ignore_case = rng.choice(patterns), rng.randrange(2) == 1
        transitions, accepts = tables[pattern, ignore_case]
        data = bytes(rng.choice(b"abAB\n\n") for _ in range(rng.randrange(0, 40)))
        cuts = sorted(rng.randrange(0, len(data) + 1) for _ in range(rng.randrange(0, 4)))
        bounds = [0] + cuts + [len(data)]
        chunk = rng.randrange(1, 65)
        stretches = [(a, b - a, G.summarise(transitions, accepts, data[a:b], 10, chunk, a)) for a, b in zip(bounds, bounds[1:])]
        witnesses = G.stitch(accepts, stretches)
        assert witnesses == sorted(set(witnesses)), (pattern, data, cuts, chunk)
        assert G.lines_of_offsets(data, witnesses) == G.expected_lines(pattern, data, b"\n", ignore_case), (pattern, data, cuts, chunk)


def test_refusals_name_the_construct(native):
    for pattern, word in G.REFUSED:
        with pytest.raises(ValueError) as refused:
            native.compile_regex(pattern)
        assert word in str(refused.value), (pattern, str(refused.value))
    with pytest.raises(ValueError) as refused:
        native.compile_regex(rb"ab(?=c)")
    assert "look-around at offset 2" in str(refused.value)
    with pytest.raises(TypeError):
        native.compile_regex("text")


def test_state_cap_gives_the_count(native):
    """Any DFA for this pattern needs 2^8 states or more."""
    with pytest.raises(ValueError) as refused:
        native.compile_regex(rb"^(a|b)*a(a|b){7}$")
    count = int(re.search(r"needs (\d+) states", str(refused.value)).group(1))
    assert count >= 256 and "64" in str(refused.value)


def test_raw_cap_stops_the_construction(native):
    began = time.monotonic()
    with pytest.raises(ValueError) as refused:
        native.compile_regex(rb"(a|b)*a(a|b){20}$")
    assert time.monotonic() - began < 1.0
    assert "states" in str(refused.value)
    began = time.monotonic()
    with pytest.raises(ValueError):
        native.compile_regex(rb"((((a{200}){200}){200}){200})")
    assert time.monotonic() - began < 1.0


def test_unknown_flag_bits_are_refused(native):
    lib = native.lib()
    error = ctypes.create_string_buffer(256)
    for flags in (2, 4, 0x80000000, 3, 0xFFFFFFFE, 0xFFFFFFFF):
        handle = ctypes.c_void_p(1)
        assert lib.mi355x_bz2_regex_compile(b"ab", 2, flags, ctypes.byref(handle), error, len(error)) == 103
        assert handle.value is None
        assert b"unknown flag bits 0x%X" % (flags & ~1) in error.value, error.value
    handle = ctypes.c_void_p()
    assert lib.mi355x_bz2_regex_compile(b"ab", 2, 1, ctypes.byref(handle), None, 0) == 0 and handle.value
    assert lib.mi355x_bz2_regex_states(handle) == 4
    lib.mi355x_bz2_regex_free(handle)
    # a short buffer gets the sentence's beginning and its final 0
    short = ctypes.create_string_buffer(b"#" * 12, 12)
    assert lib.mi355x_bz2_regex_compile(b"a\\b", 3, 0, ctypes.byref(handle), short, 8) == 103
    assert short.raw[:8] == b"regex: \0" and short.raw[8:] == b"####"
    assert lib.mi355x_bz2_regex_compile(b"ab", 2, 0, None, None, 0) == 103


def test_bindings(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in SYMBOLS:
        assert "mi355x_bz2_" + name in names and callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays
    assert native._native.regex_chunk_bytes() == native.lib().mi355x_bz2_regex_chunk_bytes() >= 16
    for cls in (native.reader._IndexedBzip2FileParallel, native.IndexedBzip2File):
        for method in READER_METHODS:
            parameters = inspect.signature(getattr(cls, method)).parameters
            assert parameters["ignore_case"].kind is inspect.Parameter.KEYWORD_ONLY, (cls.__name__, method)
            assert parameters["ignore_case"].default is False
            assert "start" not in parameters and "end" not in parameters
    for opened in (native.open(PATH, parallelization=0), native.IndexedBzip2File(PATH, parallelization=0)):
        with opened as f:
            with pytest.raises(TypeError):
                f.grep_regex(b"dolor", None, b"\n", True)
            with pytest.raises(TypeError):
                f.count_matching_lines_regex(b"dolor", b"\n", True)
            # a bad pattern, a bad newline and a bad limit are refused before anything is launched: no GPU is needed
            with pytest.raises(ValueError) as refused:
                f.grep_regex(rb"dolor\b")
            assert "\\b" in str(refused.value)
            with pytest.raises(ValueError):
                f.count_matching_lines_regex(rb"(dolor")
            with pytest.raises(ValueError):
                f.grep_regex(b"dolor", newline=b"\r\n")
            with pytest.raises(ValueError):
                f.grep_regex(b"dolor", limit=-1)
            # limit=0 checks the arguments and runs nothing
            numbers, found = f.grep_regex(b"dolor", limit=0, ignore_case=True)
            assert len(numbers) == 0 and found == []
            with pytest.raises(ValueError):
                f.grep_regex(rb"dolor\1", limit=0)
            # a compiled regex is taken as it is
            compiled = native.compile_regex(b"dolor", ignore_case=True)
            assert f.grep_regex(compiled, limit=0)[1] == []
            with pytest.raises(ValueError):
                f.grep_regex(native.compile_regex(b"dolor"), limit=0, ignore_case=True)


def test_help_lists_grep_regex(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --grep-regex arg " in run.stdout
    assert b"ibzip2-mi355x --grep-regex '" in run.stdout
    assert b"      --ignore-case " in run.stdout and b"      --grep arg " in run.stdout


def test_tool_refusals(native):
    """All refused before the input is opened: no GPU is needed."""
    run = subprocess.run([CLI, "--ignore-case", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b""
    assert run.stderr == (b"Option '--ignore-case' needs '--grep', '--grep-file', '--count-matches' or "
                          b"'--count-matches-file'\n")
    run = subprocess.run([CLI, "--line-number", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stderr == b"Option '--line-number' needs '--grep' or '--grep-file'\n"
    for other in (["--grep", "x"], ["--count-matches", "x"], ["--grep-file", PATH], ["--count-matches-file", PATH]):
        run = subprocess.run([CLI, "--grep-regex", "dolor"] + other + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", other
        assert run.stderr.startswith(b"Option '--grep-regex' cannot be combined with "), other
    run = subprocess.run([CLI, "--grep-regex", "dolor\\b", "--line-number", "--ignore-case", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b""
    assert run.stderr.startswith(b"Invalid regular expression: regex: assertion \\b at offset 5")
