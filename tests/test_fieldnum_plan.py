"""Field numbers on the CPU: the definition, the summaries and the stitching rule of indexed_bzip2_amd/csrc/bz2_fieldnum.hpp.

tests/native/fieldnum_cases.cpp runs under AddressSanitizer + UBSan as a program of its own.  The plain Python model of
fieldnum.py -- its summarise and stitch -- is compared with the direct definition, bytes.split per line and a regular
expression, over random cuts and chunk sizes 1 to 64, and the native parse_field_number with the model.  Then the bindings,
the argument refusals (all before anything is launched: no GPU is needed) and the tool's help and refusals."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT, FIXTURES
import fieldnum as FN

HARNESS = os.path.join(ROOT, "tests", "native", "fieldnum_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
PATH = os.path.join(FIXTURES, "dolorem-ipsum.txt.bz2")
ONE_FIELD_METHODS = ("field_ints", "field_ints_to_tensor")
TWO_FIELD_METHODS = ("sum_by_field", "value_sums")
INVALID_ARGUMENT = 103                                         # MI355X_BZ2_ERR_INVALID_ARGUMENT
SYMBOLS = ("parse_field_number", "field_numbers", "reader_field_numbers", "reader_take_field_numbers", "reader_field_sums",
           "reader_take_field_sums")
KNOWN = ((b"", None), (b"+", None), (b"-", None), (b"-0", 0), (b"007", 7), (b"9" * 18, 10**18 - 1), (b"9" * 19, None),
         (b"1 ", None), (b" 1", None), (b"1_0", None), (b"/", None), (b":", None), (b"\xb1", None), (b"+-1", None), (b"1-", None),
         (b"-" + b"9" * 18, 1 - 10**18), (b"+" + b"9" * 18, 10**18 - 1), (b"-" + b"9" * 19, None), (b"0" * 18, 0), (b"0" * 19, None),
         (b"+5", 5), (b"1.5", None), (b"0x10", None), (b"1e3", None), (b"1\n", None), (b"\xef\xbc\x91", None))


def test_known_answers_of_the_model():
    assert FN.NOT_A_NUMBER == -2**63 and FN.MISSING == -2**63 + 1
    for content, value in KNOWN:
        assert FN.number(content) == value, content
    # no value takes a sentinel
    assert FN.word(b"-" + b"9" * 18) > FN.MISSING > FN.NOT_A_NUMBER
    text = b"a\t12\t\n\n-7\n\t\t+3"
    nan, none = FN.NOT_A_NUMBER, FN.MISSING
    assert FN.words_of(text, 10, 9, 0) == [nan, nan, -7, nan]
    assert FN.words_of(text, 10, 9, 1) == [12, none, none, nan]
    assert FN.words_of(text, 10, 9, 2) == [nan, none, none, 3]
    assert FN.words_of(text, 10, 9, 3) == [none] * 4
    assert FN.direct(text, 10, 9, 1) == [(12, 2, 2), (none, 6, -1), (none, 9, -1), (nan, 11, 0)]
    # texts keep 19 bytes and their size saturates at 20, however they are cut
    digits = b"1234567890123456789012345"
    for n in range(len(digits) + 1):
        assert FN.text(digits[:n]) == (min(n, 20), digits[:min(n, 19)])
        for cut in range(n + 1):
            assert FN.join(FN.text(digits[:cut]), FN.text(digits[cut:n])) == FN.text(digits[:n])
    groups, missing = FN.group_sums(b"a\t1\nb\tx\na\t-3\n\nb\n", 10, 9, 0, 1)
    assert missing == 0 and [(g["key"], g["line"], g["count"], g["numbers"], g["sum"], g["min"], g["max"]) for g in groups] == [
        (b"a", 0, 2, 2, -2, -3, 1), (b"b", 1, 2, 0, 0, nan, nan), (b"", 3, 1, 0, 0, nan, nan)]


def test_model_summaries_and_stitching():
    """summarise / stitch against the direct definition: random inputs over a small alphabet of digits, signs, a letter, nl,
    dl and 0xFF, 0 to 6 random cuts, every stretch summarised with a chunk size of its own between 1 and 64."""
    rng = random.Random(0xF1E1D)
    numbers = 0
    for round_ in range(1000):
        nl = 0 if round_ % 5 == 0 else 10
        dl = (9, ord(","), 0xFF, 1)[round_ % 4]
        j = (0, 1, 2, 5, 1023)[round_ % 5 if round_ % 7 else rng.randrange(5)]
        alphabet = bytes([ord("0"), ord("9"), ord("-"), ord("+"), ord("a"), nl, dl, dl, 0xFF])
        data = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 120)))
        want = FN.direct(data, nl, dl, j)
        numbers += sum(1 for value, _, _ in want if value not in (FN.NOT_A_NUMBER, FN.MISSING))
        cuts = sorted([0, len(data)] + [rng.randrange(len(data) + 1) for _ in range(rng.randrange(0, 7))])
        summaries = [FN.summarise(data[a:b], nl, dl, j, rng.randrange(1, 65)) for a, b in zip(cuts, cuts[1:])]
        assert FN.stitch(summaries, j) == want, (data, nl, dl, j, cuts)
        # a summary does not depend on the chunk size
        whole = FN.summarise_chunk(data, nl, dl, j)
        for chunk in (1, 2, 3, 7, 64):
            assert FN.summarise(data, nl, dl, j, chunk) == whole, (data, nl, dl, j, chunk)
        assert len(whole["numbers"]) == whole["count"] == data.count(bytes([nl]))
        assert len(whole["head_texts"]) == min(len(whole["head_positions"]) + 1, j + 1)
    assert numbers >= 100            # the alphabet does produce numbers, not sentinels alone


def test_model_long_numbers_across_seams():
    """17 to 20 digits with and without a sign, cut at every position and into pieces of every size up to 23."""
    data = b"".join(b"k," + sign + b"9" * digits + b",x\n" for digits in (17, 18, 19, 20) for sign in (b"", b"-", b"+"))
    data += b"k,-,\nk,,\nk\nk,12"
    for j in (0, 1, 2):
        want = FN.direct(data, 10, ord(","), j)
        for cut in range(len(data) + 1):
            assert FN.stitch([FN.summarise(data[:cut], 10, ord(","), j, 5), FN.summarise(data[cut:], 10, ord(","), j, 7)], j) == want
        for piece in range(1, 24):
            assert FN.stitch([FN.summarise(data[at:at + piece], 10, ord(","), j, 3) for at in range(0, len(data), piece)], j) == want
    values = [value for value, _, _ in FN.direct(data, 10, ord(","), 1)]
    nan = FN.NOT_A_NUMBER
    assert values == [10**17 - 1, 1 - 10**17, 10**17 - 1, 10**18 - 1, 1 - 10**18, 10**18 - 1, nan, nan, nan, nan, nan, nan,
                      nan, nan, FN.MISSING, 12]
    # from a line start that is not offset 0, beyond 2^33: the numbers stay, the spans move
    far = FN.stitch([FN.summarise(data[:50], 10, ord(","), 1, 3), FN.summarise(data[50:], 10, ord(","), 1, 4)], 1, offset=2**33 + 5)
    assert far == [(value, start + 2**33 + 5, size) for value, start, size in FN.direct(data, 10, ord(","), 1)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fieldnum_under_sanitizers(tmp_path):
    exe = tmp_path / "fieldnum_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "fieldnum cases ok" in run.stdout


def test_native_parse_is_the_model(native):
    for content, value in KNOWN:
        assert native.parse_field_number(content) == value, content
        assert native.parse_field_number(bytearray(content)) == value and native.parse_field_number(memoryview(content)) == value
    rng = random.Random(0xF1E1D)
    seen = 0
    for round_ in range(1000):
        nl = 0 if round_ % 5 == 0 else 10
        dl = (9, ord(","), 0xFF, 1)[round_ % 4]
        alphabet = bytes([ord("0"), ord("9"), ord("-"), ord("+"), ord("a"), nl, dl, dl, 0xFF])
        data = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 120)))
        for j in (0, 1, 2, 5, 1023):
            for field in FN.F.fields_of(data, nl, dl, j):
                if field is not None:
                    assert native.parse_field_number(field) == FN.number(field), field
                    seen += 1
    assert seen > 10000
    for digits in range(0, 25):
        for sign in (b"", b"+", b"-"):
            content = sign + b"7" * digits
            assert native.parse_field_number(content) == FN.number(content), content
    with pytest.raises(TypeError):
        native.parse_field_number("12")
    assert native.lib().mi355x_bz2_parse_field_number(None, 0) == native.FIELD_NOT_A_NUMBER


def test_bindings(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in SYMBOLS:
        assert "mi355x_bz2_" + name in names and callable(getattr(native.lib(), "mi355x_bz2_" + name))
    assert native.lib().mi355x_bz2_abi_version() == 2          # additive: the version stays
    assert native.FIELD_NOT_A_NUMBER == native._native.FIELD_NOT_A_NUMBER == FN.NOT_A_NUMBER == -2**63
    assert native.FIELD_NUMBER_MISSING == native._native.FIELD_NUMBER_MISSING == FN.MISSING == -2**63 + 1
    assert ctypes.sizeof(native._native.FieldText) == 20 and ctypes.sizeof(native._native.FieldSummary) == 56
    assert native._native.FieldText.size.offset == 0 and native._native.FieldText.bytes.offset == 1
    for cls in (native.reader._IndexedBzip2FileParallel, native.IndexedBzip2File):
        for method in ONE_FIELD_METHODS + TWO_FIELD_METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
            doc = getattr(native.reader._IndexedBzip2FileParallel, method).__doc__
            assert "strtod" in doc or method.endswith("to_tensor"), method
    assert callable(native.Decoder.field_numbers) and "strtod" in native.Decoder.field_numbers.__doc__
    assert "strtod" in native.parse_field_number.__doc__


def refused_alike(call):
    """The refusals every method shares, `call` taking the keyword arguments behind the field numbers."""
    for newline in (b"\r\n", b"", "\n"):
        with pytest.raises(ValueError):
            call(newline=newline)
    for delimiter in (b"", b"::", "\t", None):
        with pytest.raises(ValueError):
            call(delimiter=delimiter)
    with pytest.raises(ValueError):
        call(delimiter=b"\n")
    with pytest.raises(ValueError):
        call(delimiter=b",", newline=b",")
    for first, count in ((-1, 1), (2**64, 1), (0, -1), (0, 2**64)):
        with pytest.raises(ValueError):
            call(first=first, count=count)


def test_argument_refusals(native):
    """All refused before anything is launched: no GPU is needed."""
    for opened in (native.open(PATH, parallelization=0), native.IndexedBzip2File(PATH, parallelization=0)):
        with opened as f:
            for method in ONE_FIELD_METHODS:
                call = getattr(f, method)
                for field in (-1, 1024, 2**32, 2**64):
                    with pytest.raises(ValueError):
                        call(field)
                refused_alike(lambda **kw: call(0, **kw))
            for method in TWO_FIELD_METHODS:
                call = getattr(f, method)
                for field in (-1, 1024, 2**32, 2**64):
                    with pytest.raises(ValueError):
                        call(field, 0)
                    with pytest.raises(ValueError):
                        call(0, field)
                refused_alike(lambda **kw: call(0, 1, **kw))
                for seed in (-1, 2**64):
                    with pytest.raises(ValueError):
                        call(0, 1, seed=seed)
            with pytest.raises(ValueError):
                f.value_sums(0, 1, limit=-1)
    # the C calls refuse the same with MI355X_BZ2_ERR_INVALID_ARGUMENT, the reader's before it builds a line index
    lib = native.lib()
    n, missing = ctypes.c_uint64(7), ctypes.c_uint64(7)
    with native.open(PATH, parallelization=0) as f:
        handle = f._open_reader()._h
        for nl, dl, field in ((10, 10, 0), (10, 9, 1024), (0, 0, 3), (10, 9, 2**32 - 1)):
            rc = lib.mi355x_bz2_reader_field_numbers(handle, nl, dl, field, 0, 5, 0, ctypes.byref(n))
            assert rc == INVALID_ARGUMENT and n.value == 0, (nl, dl, field)
            assert b"field_numbers" in lib.mi355x_bz2_reader_last_error(handle)
            n.value = 7
            for key_field, value_field in ((field, 0), (0, field)):
                rc = lib.mi355x_bz2_reader_field_sums(handle, nl, dl, key_field, value_field, 0, 0, 5, ctypes.byref(n),
                                                      ctypes.byref(missing))
                assert rc == INVALID_ARGUMENT and n.value == 0 and missing.value == 0, (nl, dl, key_field, value_field)
                assert b"field_sums" in lib.mi355x_bz2_reader_last_error(handle)
                n.value = missing.value = 7
        assert lib.mi355x_bz2_reader_take_field_numbers(handle, None, 0, 0) == INVALID_ARGUMENT           # nothing is held
        assert lib.mi355x_bz2_reader_take_field_sums(handle, *([None] * 9), 0) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_take_field_numbers(handle, None, 1, 0) == INVALID_ARGUMENT           # no destination
        assert lib.mi355x_bz2_reader_field_numbers(handle, 10, 9, 0, 0, 5, 0, None) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_field_sums(handle, 10, 9, 0, 1, 0, 0, 5, None, None) == INVALID_ARGUMENT
        assert lib.mi355x_bz2_reader_field_sums(handle, 10, 9, 0, 1, 0, 0, 5, ctypes.byref(n), None) == INVALID_ARGUMENT
        assert f.tell() == 0
    assert lib.mi355x_bz2_field_numbers(None, None, 0, 10, 9, 0, None, None, None, None, None, None, None, 0) == INVALID_ARGUMENT


def test_help_lists_the_option(native):
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"      --sum-by-field arg " in run.stdout and b"sum<TAB>numbers<TAB>key" in run.stdout and b"strtod" in run.stdout
    assert b"ibzip2-mi355x --sum-by-field 0,2 file.tsv.bz2" in run.stdout
    # what was there stays
    assert b"      --count-by-field arg " in run.stdout and b"ibzip2-mi355x --count-by-field 2 file.tsv.bz2" in run.stdout
    assert b"      --cut-field arg " in run.stdout and b"ibzip2-mi355x --cut-field 2 file.tsv.bz2" in run.stdout


def test_tool_refusals(native):
    """All refused before the input is opened: no GPU is needed."""
    for other in (["--grep", "x"], ["--count-matches", "x"], ["--grep-file", PATH], ["--count-matches-file", PATH],
                  ["--grep-regex", "x"], ["--count-lines"], ["--line-hashes"], ["--count-distinct-lines"], ["--cut-field", "1"],
                  ["--count-by-field", "1"]):
        run = subprocess.run([CLI, "--sum-by-field", "0,1"] + other + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", other
        assert run.stderr.startswith(b"Option '--sum-by-field' cannot be combined with "), other
    for fields in ("-1,0", "x", "", "1", "1,", ",1", "1.5,0", "1024,0", "0,1024", "0,18446744073709551616", "0x10,1", " 1,2", "1,2,3",
                   "1;2", "1, 2"):
        run = subprocess.run([CLI, "--sum-by-field=" + fields, PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", fields
        assert run.stderr == b"Bad value for --sum-by-field\n", fields
    for delimiter in ("", "ab", "\n", "\\n", "\\x0a", "\\xg0"):
        run = subprocess.run([CLI, "--sum-by-field", "0,1", "--field-delimiter=" + delimiter, PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"" and run.stderr == b"Bad value for --field-delimiter\n", delimiter
    run = subprocess.run([CLI, "--sum-by-field", "0,1", "--seed", "x", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr == b"Bad value for --seed\n"
    run = subprocess.run([CLI, "--sum-by-field"], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr.startswith(b"Option '--sum-by-field' is missing an argument\n")
    # the messages that were there stay byte for byte
    run = subprocess.run([CLI, "--field-delimiter", ",", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stdout == b"" and run.stderr == b"Option '--field-delimiter' needs '--cut-field'\n"
    run = subprocess.run([CLI, "--seed", "1", PATH], capture_output=True, timeout=300)
    assert run.returncode != 0 and run.stderr == b"Option '--seed' needs '--line-hashes' or '--count-distinct-lines'\n"
    for other in (["--grep", "x"], ["--cut-field", "1"], ["--count-lines"]):
        run = subprocess.run([CLI, "--count-by-field", "1"] + other + [PATH], capture_output=True, timeout=300)
        assert run.returncode != 0 and run.stdout == b"", other
        assert run.stderr == (b"Option '--count-by-field' cannot be combined with '--count-lines', '--grep', '--grep-regex', "
                              b"'--count-matches', '--grep-file', '--count-matches-file', '--line-hashes', "
                              b"'--count-distinct-lines' or '--cut-field'\n"), other
