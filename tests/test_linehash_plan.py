"""line_hashes on the CPU: the hash, the summaries and the stitching rule of indexed_bzip2_amd/csrc/bz2_linehash.hpp.

tests/native/linehash_cases.cpp runs under AddressSanitizer + UBSan as a program of its own.  The known answers of the
hash are literals; ibz2.line_hash and mi355x_bz2_line_hash are compared with the plain Python model of linehash.py on
random contents and seeds; the model's summarise and stitch are compared with the direct definition over random cuts and
chunk sizes 1 to 64.  Then the bindings, the argument refusals (all before anything is launched: no GPU is needed) and
the tool's refusals."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES
import linehash as H

HARNESS = os.path.join(ROOT, "tests", "native", "linehash_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
READER_METHODS = ("line_hashes", "line_hashes_to_tensor", "count_distinct_lines", "first_occurrences")
SYMBOLS = ("line_hash", "line_hash_chunk_bytes", "hash_lines", "reader_line_hashes", "reader_take_line_hashes",
           "reader_line_hashes_device", "reader_distinct_lines", "reader_take_distinct_lines")


def test_known_answers_of_the_model():
    assert H.P == 2**61 - 1
    assert H.base(0) == 0x0220A8397B1DD5B6 and H.base(1) == 0x110A2DEC890261C5
    assert H.line_hash(b"") == 0 and H.line_hash(b"a") == 98
    assert H.line_hash(b"\0\0") == 153307352162751927 and H.line_hash(b"hello") == 951416200074518375
    assert H.line_hash(b"\0") != H.line_hash(b"\0\0")


def test_known_answers(native):
    assert native.line_hash(b"") == 0 and native.line_hash(b"a") == 98
    assert native.line_hash(b"\0\0") == 153307352162751927 and native.line_hash(b"hello", seed=0) == 951416200074518375
    assert native.line_hash(b"\0") != native.line_hash(b"\0\0")
    assert native.line_hash(bytearray(b"hello")) == native.line_hash(memoryview(b"hello")) == 951416200074518375
    # the base of a seed shows in the hash of a one-byte line followed by... nothing: h(b) = b + 1, h(b b') = (b + 1) x + b' + 1
    for seed, base in ((0, 0x0220A8397B1DD5B6), (1, 0x110A2DEC890261C5)):
        assert native.line_hash(b"\0\xff", seed) == (base + 256) % H.P


def test_line_hash_against_the_model(native):
    rng = random.Random(0x11E5)
    lib = native.lib()
    for round_ in range(300):
        content = bytes(rng.choice(b"ab\n\0\xff") if round_ % 2 else rng.randrange(256) for _ in range(rng.randrange(0, 400)))
        seed = rng.choice([0, 1, 2**64 - 1, rng.randrange(2**64)])
        want = H.line_hash(content, seed)
        assert 0 <= want < H.P
        assert native.line_hash(content, seed) == want, (content, seed)
        assert lib.mi355x_bz2_line_hash(content, len(content), seed) == want, (content, seed)
    # lines of one byte value and every length are pairwise different, whatever the value
    for value in (0, 0xFF):
        hashes = {native.line_hash(bytes([value]) * n) for n in range(0, 301)}
        assert len(hashes) == 301


def test_model_summaries_and_stitching():
    """summarise / stitch against the direct definition: random inputs over a small alphabet, 0 to 6 random cuts, every
    stretch summarised with a chunk size of its own between 1 and 64."""
    rng = random.Random(0xC0FFEE)
    for round_ in range(600):
        data = bytes(rng.choice(b"ab\n\0\xff") for _ in range(rng.randrange(0, 120)))
        nl = 0 if round_ % 5 == 0 else 10
        seed = rng.randrange(2**64)
        x = H.base(seed)
        want = H.direct(data, nl, seed)
        cuts = sorted([0, len(data)] + [rng.randrange(len(data) + 1) for _ in range(rng.randrange(0, 7))])
        summaries = [H.summarise(data[a:b], nl, x, rng.randrange(1, 65)) for a, b in zip(cuts, cuts[1:])]
        assert H.stitch(summaries) == want, (data, nl, cuts)
        # a summary does not depend on the chunk size
        whole = H.summarise_chunk(data, nl, x)
        for chunk in (1, 2, 3, 7, 64):
            assert H.summarise(data, nl, x, chunk) == whole, (data, nl, chunk)
        assert len(whole["hashes"]) == data.count(bytes([nl]))
        # the prefix sums the GPU tests use give the same summaries and lines
        prefix = H.Prefix(data, x)
        a, b = cuts[len(cuts) // 2 - 1], cuts[len(cuts) // 2]
        assert prefix.summary(a, b - a, nl) == H.summarise_chunk(data[a:b], nl, x) and prefix.lines(nl) == want


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_linehash_under_sanitizers(tmp_path):
    exe = tmp_path / "linehash_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "linehash cases ok" in run.stdout


def test_bindings(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in SYMBOLS:
        assert "mi355x_bz2_" + name in names and callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays
    assert native._native.line_hash_chunk_bytes() == native.lib().mi355x_bz2_line_hash_chunk_bytes() >= 16
    assert ctypes.sizeof(native._native.LineHashSummary) == 48
    for cls in (native.reader._IndexedBzip2FileParallel, native.IndexedBzip2File):
        for method in READER_METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
    assert callable(native.Decoder.hash_lines)


def test_argument_refusals(native):
    """All refused before anything is launched: no GPU is needed."""
    with pytest.raises(TypeError):
        native.line_hash("hello")
    for seed in (-1, 2**64):
        with pytest.raises(ValueError):
            native.line_hash(b"hello", seed)
    for opened in (native.open(PATH, parallelization=0), native.IndexedBzip2File(PATH, parallelization=0)):
        with opened as f:
            for method in READER_METHODS:
                call = getattr(f, method)
                with pytest.raises(ValueError):
                    call(newline=b"\r\n")
                with pytest.raises(ValueError):
                    call(newline=b"")
                with pytest.raises(ValueError):
                    call(newline="\n")
                with pytest.raises(ValueError):
                    call(seed=-1)
                with pytest.raises(ValueError):
                    call(seed=2**64)
            for method in READER_METHODS[:2]:
                call = getattr(f, method)
                for first, count in ((-1, 1), (2**64, 1), (0, -1), (0, 2**64)):
                    with pytest.raises(ValueError):
                        call(first, count)


def test_help_lists_the_options(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --line-hashes " in run.stdout and b"      --count-distinct-lines " in run.stdout
    assert b"      --seed arg " in run.stdout
    assert b"ibzip2-mi355x --count-distinct-lines file.bz2" in run.stdout


def test_tool_refusals(native):
    """All refused before the input is opened: no GPU is needed."""
    run = subprocess.run([CLI, "--seed", "5", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b""
    assert run.stderr == b"Option '--seed' needs '--line-hashes' or '--count-distinct-lines'\n"
    run = subprocess.run([CLI, "--line-hashes", "--count-distinct-lines", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b""
    assert run.stderr == b"Options '--line-hashes' and '--count-distinct-lines' cannot be combined\n"
    for option in ("--line-hashes", "--count-distinct-lines"):
        for other in (["--grep", "x"], ["--count-matches", "x"], ["--grep-file", PATH], ["--count-matches-file", PATH],
                      ["--grep-regex", "x"], ["--count-lines"]):
            run = subprocess.run([CLI, option] + other + [PATH], capture_output=True, timeout=300)
            assert run.returncode != 0 and run.stdout == b"", (option, other)
            assert run.stderr.startswith(b"Options '--line-hashes' and '--count-distinct-lines' cannot be combined with "), other
        for seed in ("-1", "x", "", "1.5", "18446744073709551616", "0x10", " 1"):
            run = subprocess.run([CLI, option, "--seed=" + seed, PATH], capture_output=True, timeout=300)
            assert run.returncode != 0 and run.stdout == b"", (option, seed)
            assert run.stderr == b"Bad value for --seed\n", (option, seed)
