"""Field hashes on the CPU: the summaries and the stitching rule of indexed_bzip2_amd/csrc/bz2_fieldhash.hpp.

tests/native/fieldhash_cases.cpp runs under AddressSanitizer + UBSan as a program of its own.  The plain Python model of
fieldhash.py -- its summarise and stitch -- is compared with the direct definition, bytes.split per line and the hash of
the field, over random cuts and chunk sizes 1 to 64.  Then the bindings, the argument refusals (all before anything is
launched: no GPU is needed) and the tool's help and refusals."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES
import fieldhash as FH
import linehash as LH

HARNESS = os.path.join(ROOT, "tests", "native", "fieldhash_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
READER_METHODS = ("field_hashes", "field_hashes_to_tensor", "count_by_field", "value_counts")
INVALID_ARGUMENT = 103                                         # MI355X_BZ2_ERR_INVALID_ARGUMENT
SYMBOLS = ("field_hashes", "reader_field_hashes", "reader_take_field_hashes", "reader_field_groups", "reader_take_field_groups")


def test_known_answers_of_the_model():
    text = b"a\tbc\t\n\nx\n\t\ty"
    h = LH.line_hash
    assert FH.MISSING == 2**61 - 1 == LH.P and FH.MISSING < 2**63
    assert h(b"") == 0 and h(b"a") == 98                          # the empty field hashes to 0 and is present
    assert FH.keys_of(text, 10, 9, 0) == [h(b"a"), 0, h(b"x"), 0]
    assert FH.keys_of(text, 10, 9, 1) == [h(b"bc"), FH.MISSING, FH.MISSING, 0]
    assert FH.keys_of(text, 10, 9, 2) == [0, FH.MISSING, FH.MISSING, h(b"y")]
    assert FH.keys_of(text, 10, 9, 3) == [FH.MISSING] * 4
    assert FH.direct(text, 10, 9, 1) == [(h(b"bc"), 2, 2), (FH.MISSING, 6, -1), (FH.MISSING, 8, -1), (0, 10, 0)]
    zeros = FH.keys_of(b"k,\0\nk,\0\0\n", 10, ord(","), 1)
    assert zeros == [1, (LH.base(0) + 1) % LH.P] and zeros[0] != zeros[1]       # "\0" and "\0\0" differ
    assert FH.keys_of(b"ab\n", 10, 9, 0, seed=5) == [h(b"ab", 5)] != [h(b"ab", 0)]
    # no hash is the key of a missing field: every hash is below p
    assert all(key < FH.MISSING for key in FH.keys_of(text, 10, 9, 0))
    # the closed form for runs is the loop
    for byte, n in ((0, 1), (97, 64), (255, 1000)):
        assert FH.run_part(byte, n, LH.base(3)) == LH.part(bytes([byte]) * n, LH.base(3))
    assert FH.part(b"xy" + b"a" * 100 + b"z" + b"\0" * 64, LH.base(1)) == LH.part(b"xy" + b"a" * 100 + b"z" + b"\0" * 64, LH.base(1))


def test_model_summaries_and_stitching():
    """summarise / stitch against the direct definition: random inputs over a small alphabet that holds nl, dl, 0 and
    0xFF, 0 to 6 random cuts, every stretch summarised with a chunk size of its own between 1 and 64."""
    rng = random.Random(0xF1E1D)
    for round_ in range(1000):
        nl = 0 if round_ % 5 == 0 else 10
        dl = (9, ord(","), 0xFF, 1)[round_ % 4]
        j = (0, 1, 2, 5, 1023)[round_ % 5 if round_ % 7 else rng.randrange(5)]
        seed = 0 if round_ % 2 else rng.randrange(2**64)
        x = LH.base(seed)
        alphabet = bytes([ord("a"), ord("b"), nl, dl, dl, 0, 0xFF])
        data = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 120)))
        want = FH.direct(data, nl, dl, j, seed)
        cuts = sorted([0, len(data)] + [rng.randrange(len(data) + 1) for _ in range(rng.randrange(0, 7))])
        summaries = [FH.summarise(data[a:b], nl, dl, j, x, rng.randrange(1, 65)) for a, b in zip(cuts, cuts[1:])]
        assert FH.stitch(summaries, j, x, dl) == want, (data, nl, dl, j, cuts)
        # a summary does not depend on the chunk size
        whole = FH.summarise_chunk(data, nl, dl, j, x)
        for chunk in (1, 2, 3, 7, 64):
            assert FH.summarise(data, nl, dl, j, x, chunk) == whole, (data, nl, dl, j, chunk)
        assert len(whole["keys"]) == whole["count"] == data.count(bytes([nl]))
        assert len(whole["head_hashes"]) == len(whole["head_positions"]) <= j + 1
        assert whole["head"] == LH.summarise_chunk(data, nl, x)["head"] and whole["tail"] == LH.summarise_chunk(data, nl, x)["tail"]


def test_model_a_field_across_three_stretches_and_large_offsets():
    pieces = [b"x\nab,c", b"d,efg", b"hij", b"kl,m", b"no\nq,r"]
    text = b"".join(pieces)
    x = LH.base(7)
    for j in range(5):
        got = FH.stitch([FH.summarise(p, 10, ord(","), j, x, 2) for p in pieces], j, x, ord(","))
        assert got == FH.direct(text, 10, ord(","), j, 7)
    # field 2 of the second line starts in the second stretch, crosses the third and ends in the fourth
    assert FH.direct(text, 10, ord(","), 2, 7) == [(FH.MISSING, 1, -1), (LH.line_hash(b"efghijkl", 7), 8, 8), (FH.MISSING, 24, -1)]
    # from a line start that is not offset 0, beyond 2^33: the keys stay, the spans move
    far = FH.stitch([FH.summarise(p, 10, ord(","), 2, x, 3) for p in pieces], 2, x, ord(","), offset=2**33 + 5)
    assert far == [(key, start + 2**33 + 5, size) for key, start, size in FH.direct(text, 10, ord(","), 2, 7)]
    # a head position beyond 2^33 of its stretch: the power is of that offset.  The stretch is 2^33 + 100 times 'a', a
    # comma, 7 times 'b'; the line in front of it is "k,": field 1 is the run, field 2 the b's
    run = 2**33 + 100
    front = FH.summarise_chunk(b"k,", 10, ord(","), 1, x)
    head = LH.followed_by(LH.followed_by(FH.run_part(97, run, x), LH.part(b",", x)), LH.part(b"bbbbbbb", x))
    middle = {"size": run + 8, "count": 0, "has_delimiter": False, "first_nl": None, "head_positions": [run], "tail_start": 0,
              "tail_delims": 1, "tail_field_start": None, "tail_field_end": None, "tail_non_empty": True, "fields": [], "keys": [],
              "head": head, "tail": (0, 1), "head_hashes": [FH.run_part(97, run, x)[0]], "tail_start_hash": None, "tail_end_hash": None}
    assert FH.stitch([front, middle], 1, x, ord(",")) == [(FH.run_part(97, run, x)[0], 2, run)]
    front2 = FH.summarise_chunk(b"k,", 10, ord(","), 2, x)
    assert FH.stitch([front2, middle], 2, x, ord(",")) == [(LH.line_hash(b"bbbbbbb", 7), 2 + run + 1, 7)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fieldhash_under_sanitizers(tmp_path):
    exe = tmp_path / "fieldhash_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "fieldhash cases ok" in run.stdout


def test_bindings(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in SYMBOLS:
        assert "mi355x_bz2_" + name in names and callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays
    assert native.FIELD_MISSING == native._native.FIELD_MISSING == 2**61 - 1
    assert ctypes.sizeof(native._native.FieldHashSummary) == 104
    for cls in (native.reader._IndexedBzip2FileParallel, native.IndexedBzip2File):
        for method in READER_METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
            assert "CSV" in getattr(native.reader._IndexedBzip2FileParallel, method).__doc__ or method.endswith("to_tensor")
    assert callable(native.Decoder.field_hashes)
    # the key of a present field is the line hash of its bytes: the CPU's, with the same seed
    assert native.line_hash(b"bc", 9) == LH.line_hash(b"bc", 9) < native.FIELD_MISSING


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
                        call(0, first=first, count=count)
                for seed in (-1, 2**64):                        # as line_hashes refuses it
                    with pytest.raises(ValueError):
                        call(0, seed=seed)
                    with pytest.raises(ValueError):
                        f.line_hashes(seed=seed)
            with pytest.raises(ValueError):
                f.value_counts(0, limit=-1)
    # the C calls refuse the same with MI355X_BZ2_ERR_INVALID_ARGUMENT, the reader's before it builds a line index
    lib = native.lib()
    n, missing = ctypes.c_uint64(7), ctypes.c_uint64(7)
    with native.open(PATH, parallelization=0) as f:
        handle = f._open_reader()._h
        for nl, dl, field in ((10, 10, 0), (10, 9, 1024), (0, 0, 3), (10, 9, 2**32 - 1)):
            rc = lib.mi355x_bz2_reader_field_hashes(handle, nl, dl, field, 0, 0, 5, 0, ctypes.byref(n))
            assert rc == INVALID_ARGUMENT and n.value == 0, (nl, dl, field)
            assert b"field_hashes" in lib.mi355x_bz2_reader_last_error(handle)
            n.value = 7
            rc = lib.mi355x_bz2_reader_field_groups(handle, nl, dl, field, 0, 0, 5, ctypes.byref(n), ctypes.byref(missing))
            assert rc == INVALID_ARGUMENT and n.value == 0 and missing.value == 0, (nl, dl, field)
            assert b"field_groups" in lib.mi355x_bz2_reader_last_error(handle)
            n.value = missing.value = 7
        assert lib.mi355x_bz2_reader_take_field_hashes(handle, None, 0, 0) == INVALID_ARGUMENT            # nothing is held
        assert lib.mi355x_bz2_reader_take_field_groups(handle, None, None, None, None, 0) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_field_hashes(handle, 10, 9, 0, 0, 0, 5, 0, None) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_field_groups(handle, 10, 9, 0, 0, 0, 5, None, None) == INVALID_ARGUMENT
        assert f.tell() == 0
    assert lib.mi355x_bz2_field_hashes(None, None, 0, 10, 9, 0, 0, None, None, None, None, None, None, 0) == INVALID_ARGUMENT


def test_help_lists_the_option(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --count-by-field arg " in run.stdout and b"count<TAB>value" in run.stdout
    assert b"ibzip2-mi355x --count-by-field 2 file.tsv.bz2" in run.stdout
    # what was there stays
    assert b"      --cut-field arg " in run.stdout and b"ibzip2-mi355x --cut-field 2 file.tsv.bz2" in run.stdout


def test_tool_refusals(native):
    """All refused before the input is opened: no GPU is needed."""
    for other in (["--grep", "x"], ["--count-matches", "x"], ["--grep-file", PATH], ["--count-matches-file", PATH],
                  ["--grep-regex", "x"], ["--count-lines"], ["--line-hashes"], ["--count-distinct-lines"], ["--cut-field", "1"]):
        run = subprocess.run([CLI, "--count-by-field", "1"] + other + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", other
        assert run.stderr.startswith(b"Option '--count-by-field' cannot be combined with "), other
    for field in ("-1", "x", "", "1.5", "1024", "18446744073709551616", "0x10", " 1"):
        run = subprocess.run([CLI, "--count-by-field=" + field, PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", field
        assert run.stderr == b"Bad value for --count-by-field\n", field
    for delimiter in ("", "ab", "\n", "\\n", "\\x0a", "\\xg0"):
        run = subprocess.run([CLI, "--count-by-field", "0", "--field-delimiter=" + delimiter, PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"" and run.stderr == b"Bad value for --field-delimiter\n", delimiter
    run = subprocess.run([CLI, "--count-by-field", "0", "--seed", "x", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr == b"Bad value for --seed\n"
    # the messages that were there stay byte for byte
    run = subprocess.run([CLI, "--field-delimiter", ",", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr == b"Option '--field-delimiter' needs '--cut-field'\n"
    run = subprocess.run([CLI, "--seed", "1", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stderr == b"Option '--seed' needs '--line-hashes' or '--count-distinct-lines'\n"
