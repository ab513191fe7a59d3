"""Field numbers on the GPU: the kernels under Decoder.field_numbers (k_field_numbers and k_field_texts behind the field
passes), the reader's field_ints / field_ints_to_tensor / sum_by_field / value_sums, and the tool's --sum-by-field.

The reference is the plain Python model of fieldnum.py -- bytes.split per line, a regular expression and int(), its own
summarise and stitch, and sums in Python's integers -- never the code under test.  Numbers, offsets, sizes, texts, counts
and sums are compared exactly."""
import ctypes
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import datagen
import fieldnum as FN
import fields as F
import test_gpu_fields as TF

pytestmark = pytest.mark.gpu

CLI = TF.CLI
NL, TAB, COMMA = 10, 9, ord(",")
ONES, UNTOUCHED = TF.ONES, TF.UNTOUCHED
CANARY = FN.NOT_A_NUMBER + 2                                    # what Decoder.field_numbers fills `numbers` with
NAN, NONE = FN.NOT_A_NUMBER, FN.MISSING
CHUNK, TILE = 256, 65_536
SIZES = (0, 1, 19, 20, CHUNK - 1, CHUNK, CHUNK + 1, TILE - 1, TILE, TILE + 1)
SUMMARY_KEYS = FN.FIELD_KEYS + ("head_texts", "tail_text")
OK, INVALID_ARGUMENT = 0, 103


# ------------------------------------------------------------------------------------------------ the kernels

def odd_field(rng):
    """A field that is a number, nearly one, or nothing like one."""
    kind = rng.randrange(16)
    sign = rng.choice([b"", b"", b"-", b"+"])
    if kind < 6:
        return sign + b"%d" % rng.randrange(10 ** rng.randrange(1, 17))
    if kind < 8:
        return sign + bytes(rng.choice(b"0123456789") for _ in range(rng.choice((17, 18, 19, 20))))
    if kind == 8:
        return rng.choice([b"+", b"-", b"", b"", b"-0", b"007", b"00"])
    if kind == 9:                                               # '/' and ':' lie around the digits, 0x80 is no ASCII
        digits = bytearray(sign + b"%d" % rng.randrange(10**9))
        digits[rng.randrange(len(digits))] = rng.choice([0x2F, 0x3A, 0x80])
        return bytes(digits)
    if kind == 10:
        return rng.choice([b"1 ", b" 1", b"1_0", b"0x1f", b"1.5", b"1e3", b"+-1", b"1-", b"12,5", b"3,14"])
    return bytes(rng.choice(b"abcxyz,") for _ in range(rng.randrange(1, 12)))


def device_text():
    """(text, {name: (offset, size)}): a few hundred kB."""
    rng = random.Random(0x4E756D)
    parts, at, where = [], 0, {}

    def add(piece, name=None):
        nonlocal at
        if name is not None:
            where[name] = (at, len(piece))
        parts.append(piece)
        at += len(piece)

    def records(n):
        out = bytearray()
        for _ in range(n):
            out += b"\t".join(odd_field(rng) for _ in range(rng.choice((1, 1, 2, 2, 3, 3, 4, 9, 12)))) + b"\n"
        return bytes(out)

    add(records(4000), "lines")
    # 17 to 20 digits with and without a sign, the lone signs, empty and missing fields, the three bytes in numeric fields
    special = bytearray()
    for digits in (17, 18, 19, 20):
        for sign in (b"", b"-", b"+"):
            special += b"k\t" + sign + b"9" * digits + b"\tx\n" + b"k\t" + sign + b"1" + b"0" * (digits - 1) + b"\n"
    for field in (b"+", b"-", b"", b"12/4", b"12:4", b"12\x804", b"/", b":", b"\x80", b"0", b"-0", b"+0"):
        special += b"k\t" + field + b"\tx\n" + b"k\t" + field + b"\n"
    special += b"k\n\nk\n"
    add(b"#" * (-at % 16))
    add(bytes(special), "special")
    # a line whose field 1 is a number of 9 digits, far enough from both ends for a tile in front of it and behind it
    add(records(2500), "front")
    add(b"key\t123456789\tz\n", "edge")
    add(records(2500), "back")
    # 1 024 tabs in one line: field 1023 is a number
    add(b"\t" * 1023 + b"4711\t\n" + b"\t" * 1022 + b"12\n" + b"1\t" * 1023 + b"-5", "wide")
    return b"".join(parts), where


@pytest.fixture(scope="module")
def device(native):
    text, where = device_text()
    dec = TF.decoded(native, text)
    yield {"dec": dec, "text": text, "where": where, "models": {}}
    dec.close()


def model_of(device, span, field, nl, dl):
    """The model's summary of a span, computed once per (span, field, nl, dl), shared, left unchanged."""
    key = (span, field, nl, dl)
    if key not in device["models"]:
        device["models"][key] = FN.summarise_chunk(device["text"][span[0]:span[0] + span[1]], nl, dl, field)
    return device["models"][key]


def check_spans(device, spans, field=1, nl=NL, dl=TAB, capacity=None, room=None):
    """Summaries, texts, numbers, starts and sizes of Decoder.field_numbers against the model, exactly; returns the
    model's (number, start, size) per closed line."""
    models = [model_of(device, span, field, nl, dl) for span in spans]
    summaries, numbers, starts, sizes = device["dec"].field_numbers(spans, field, bytes([dl]), bytes([nl]), capacity, room)
    assert numbers.dtype == np.int64 and starts.dtype == np.uint64 and sizes.dtype == np.int64
    for span, model, got in zip(spans, models, summaries):
        assert got == {key: model[key] for key in SUMMARY_KEYS}, (span, field)
    wanted = [(value, span[0] + start, size) for span, model in zip(spans, models)
              for value, (start, size) in zip(model["numbers"], model["fields"])]
    written = len(wanted) if capacity is None else min(capacity, len(wanted))
    assert numbers[:written].tolist() == [v for v, _, _ in wanted[:written]], (spans[:3], field)
    assert starts[:written].tolist() == [s for _, s, _ in wanted[:written]], (spans[:3], field)
    assert sizes[:written].tolist() == [n for _, _, n in wanted[:written]], (spans[:3], field)
    assert (numbers[written:] == CANARY).all() and (starts[written:] == ONES).all() and (sizes[written:] == UNTOUCHED).all(), \
        "written at or beyond the capacity"
    return wanted


def test_the_corpus_holds_every_kind(native, device):
    assert native._native.field_chunk_bytes() == CHUNK
    text = device["text"]
    assert 200_000 < len(text) < 900_000
    words = FN.words_of(text, NL, TAB, 1)
    assert sum(1 for w in words if w not in (NAN, NONE)) >= 1000 and words.count(NAN) >= 1000 and words.count(NONE) >= 100
    fields = [field for field in F.fields_of(text, NL, TAB, 1) if field is not None]
    for digits in (17, 18, 19, 20):
        for sign in (b"", b"-", b"+"):
            assert sign + b"9" * digits in fields
    for field in (b"+", b"-", b"", b"12/4", b"12:4", b"12\x804"):
        assert field in fields
    # the whole output as one span is the direct definition, tail included
    wanted = check_spans(device, [(0, len(text))])
    assert [w for w, _, _ in wanted] == words[:-1] and text[-1] != NL
    assert device["dec"].field_numbers([(0, len(text))], 1)[0][0]["tail_text"] == (1, b"1")
    # every number the kernels give is the CPU definition's, and every non-number is None there
    for value, start, size in wanted[:3000]:
        if size >= 0:
            assert native.parse_field_number(text[start:start + size]) == (None if value == NAN else value)


def test_span_sizes_at_every_alignment(device):
    text = device["text"]
    base = device["where"]["lines"][0] + 1000
    base += -base % 16                                              # the output buffer is 16-byte aligned
    spans = [(base + start, size) for start in range(16) for size in SIZES]
    assert {o % 16 for o, _ in spans} == set(range(16))
    wanted = check_spans(device, spans)
    assert len(wanted) > 10_000
    assert sum(1 for w, _, _ in wanted if w not in (NAN, NONE)) > 1000 and sum(1 for w, _, _ in wanted if w == NAN) > 1000
    assert sum(1 for w, _, _ in wanted if w == NONE) > 100
    for field in (0, 7, 1023):
        check_spans(device, spans[::3], field)
    # other delimiters: ',' between fields; 0 between lines, "\n" then a byte like any other
    check_spans(device, spans[3::7], 1, dl=COMMA)
    check_spans(device, spans[5::7], 0, nl=0)
    check_spans(device, spans[5::7], 1, nl=0, dl=NL)
    # the whole output as one span, and the same span twice
    whole = (0, len(text))
    check_spans(device, [whole, spans[25], whole, spans[25]])
    for field in (0, 7, 1023):
        check_spans(device, [whole], field)
    wide = device["where"]["wide"]
    assert check_spans(device, [(wide[0], wide[1])], 1023) == [(4711, wide[0] + 1023, 4), (NONE, wide[0] + 1029 + 1024, -1)]
    got = device["dec"].field_numbers([wide], 1023)[0][0]
    assert got["tail_text"] == (2, b"-5") and len(got["head_texts"]) == 1024 and got["head_texts"][1023] == (4, b"4711")
    got = device["dec"].field_numbers([(wide[0] + 1029 + 1025, wide[1] - 2054)], 1023)[0][0]          # the tail line alone: no nl
    assert got["head_texts"] == [(1, b"1")] * 1023 + [(2, b"-5")] and got["tail_text"] == (2, b"-5") and got["count"] == 0


def test_numbers_on_chunk_and_tile_edges(device):
    """Every byte of one number on the edge between two lanes' chunks and between two tiles, and one byte off it: the
    edges are counted from a span's first byte."""
    text = device["text"]
    offset, size = device["where"]["edge"]
    at = offset + 4                                                 # of the number's first digit
    assert text[at:at + 9] == b"123456789" and at > TILE + 300 and len(text) - at > TILE + 300
    spans = []
    for edge in (CHUNK, 2 * CHUNK, TILE):
        for digit in range(-1, 10):                                 # the tab in front, the nine digits
            for off in (0, 1):                                      # the byte as the first of a chunk, and as the last
                spans.append((at + digit - edge + off, edge + 300))
    wanted = check_spans(device, spans)
    assert sum(1 for w, start, _ in wanted if start == at and w == 123456789) == len(spans)
    check_spans(device, spans[::2], 0)
    check_spans(device, spans[1::2], 2)
    # spans that begin and end inside the number: head and tail texts are pieces of it
    inside = [(at + first, last - first) for first in range(0, 9) for last in range(first, 10)]
    check_spans(device, inside)
    got = device["dec"].field_numbers([(at + 2, 5), (at - 4 - 300, 300 + 4 + 4), (at + 5, 300)], 1)[0]
    assert got[0]["head_texts"] == [(5, b"34567")] and got[0]["tail_text"] == (0, b"") and got[0]["count"] == 0
    assert got[1]["tail_text"] == (4, b"1234") and got[1]["tail_field_start"] == 304 + 4 - 4
    assert got[2]["head_texts"][:2] == [(4, b"6789"), (1, b"z")]
    # a tile and more in front of the number and behind it, the span ending inside it
    check_spans(device, [(at - TILE - 7, TILE + 7 + k) for k in range(0, 11)] + [(at + k, TILE + 100) for k in range(0, 10)])


def test_long_digit_strings_signs_and_odd_bytes(device):
    text = device["text"]
    offset, size = device["where"]["special"]
    assert offset % 16 == 0
    wanted = check_spans(device, [(offset, size)])
    values = [w for w, _, _ in wanted]
    assert values[:12] == [10**17 - 1, 10**16, 1 - 10**17, -10**16, 10**17 - 1, 10**16,
                           10**18 - 1, 10**17, 1 - 10**18, -10**17, 10**18 - 1, 10**17]
    assert values[12:24] == [NAN] * 12                              # 19 and 20 digits
    assert values[24:48] == [NAN] * 18 + [0, 0, 0, 0, 0, 0] and values[48:] == [NONE, NONE, NONE]
    # the region cut at every byte of its first 700 and entered there: texts of 17 to 20 bytes on both sides of a cut
    check_spans(device, [(offset, k) for k in range(0, 700, 3)])
    check_spans(device, [(offset + k, size - k) for k in range(0, 700, 3)])
    check_spans(device, [(offset + k, 21) for k in range(0, 400)])
    for field in (0, 2):
        check_spans(device, [(offset, size), (offset + 5, size - 9)], field)
    assert text[offset:offset + 2] == b"k\t"


def test_capacity_smaller_than_the_count(native, device):
    offset, _ = device["where"]["lines"]
    spans = [(offset + 3, 70_000), (offset + 70_003, 5_000)]
    total = len(check_spans(device, spans))
    assert total > 1000
    for capacity in (0, 1, 2, 255, 256, total - 1, total):
        check_spans(device, spans, capacity=capacity, room=total + 64)
    check_spans(device, spans, 0, capacity=257, room=total + 64)
    # nothing is asked for: no span; spans outside the output and arguments out of range are refused
    assert device["dec"].field_numbers([], 1)[0] == []
    with pytest.raises(Exception):
        device["dec"].field_numbers([(len(device["text"]) - 5, 6)], 1)
    for field, delimiter, newline in ((1024, b"\t", b"\n"), (-1, b"\t", b"\n"), (0, b"\n", b"\n"), (0, b"", b"\n"), (0, b"\t", b"ab")):
        with pytest.raises(ValueError):
            device["dec"].field_numbers([(0, 10)], field, delimiter, newline)
    # without the span columns and without the texts the numbers are the same
    dec, lib = device["dec"], native.lib()
    whole = (0, len(device["text"]))
    again = dec.field_numbers([whole], 1)[1]
    summaries = (native._native.FieldSummary * 1)()
    arr = (native._native.ByteSpan * 1)(native._native.ByteSpan(*whole))
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    numbers, pointer = np.zeros(len(again), dtype=np.int64), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(pointer), numbers.nbytes) == 0
    try:
        assert lib.mi355x_bz2_field_numbers(dec._h, arr, 1, NL, TAB, 1, summaries, None, None, None, pointer, None, None, len(numbers)) == 0
        assert hip.hipMemcpy(numbers.ctypes.data, pointer, numbers.nbytes, 2) == 0
        # one of the two span columns alone is refused
        assert lib.mi355x_bz2_field_numbers(dec._h, arr, 1, NL, TAB, 1, summaries, None, None, None, pointer, pointer, None, 1) == INVALID_ARGUMENT
    finally:
        hip.hipFree(pointer)
    assert numbers.tolist() == again.tolist() and summaries[0].count == len(again)


# ------------------------------------------------------------------------------------------------ the reader

def reader_text():
    """About 1 MB of "key<TAB>text<TAB>number" lines: a few hundred keys with heavy repeats, numbers of up to 18 digits that
    make up a third of the bytes, some lines without the number, without text and number, or with something else in the
    number's place, and an unterminated numeric tail."""
    rng = random.Random(0x5EED5)
    keys = [b"host%d" % rng.randrange(10**5) for _ in range(300)] + [b""]
    weights = [1000 // (k + 1) + 1 for k in range(len(keys))]
    out = bytearray()
    while len(out) < 1_000_000:
        key = rng.choices(keys, weights)[0]
        kind = rng.randrange(20)
        if kind == 0:
            out += key + b"\n"
        elif kind == 1:
            out += key + b"\tsome text\n"
        elif kind == 2:
            out += key + b"\tsome text\t" + rng.choice([b"", b"-", b"n/a", b"1.5", b"12 ", b"9" * 19]) + b"\n"
        else:
            number = rng.choice([b"", b"", b"-", b"+"]) + b"%d" % rng.randrange(10 ** rng.randrange(1, 19))
            out += key + b"\t" + bytes(rng.choice(b"abc def") for _ in range(rng.randrange(12))) + b"\t" + number + b"\n"
    return bytes(out) + b"host-at-the-end\tlast\t-12345"


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("fieldnum")
    raw = reader_text()
    path = folder / "numbers.bz2"
    path.write_bytes(datagen.compress(raw, 1))
    # computed once, shared, left unchanged
    wanted = {(j, dl): FN.words_of(raw, NL, dl, j) for j, dl in ((0, TAB), (1, TAB), (2, TAB), (3, TAB), (1023, TAB), (1, ord(" ")))}
    with native.open(str(path), parallelization=0) as f:
        blocks = sorted(f.block_offsets().values())
    assert len(blocks) >= 9                                      # several launch seams
    spans = F.direct(raw, NL, TAB, 2)
    inside = [b for b in blocks[1:-1] if any(start < b < start + size for start, size in spans_near(spans, b))]
    assert len(inside) >= 1, "a block seam inside a number"
    return {"raw": raw, "path": str(path), "wanted": wanted, "blocks": blocks, "folder": folder}


def spans_near(spans, offset):
    """The spans of the lines around a decoded offset (the spans ascend)."""
    low, high = 0, len(spans)
    while high - low > 1:
        mid = (low + high) // 2
        if spans[mid][0] <= offset:
            low = mid
        else:
            high = mid
    return [s for s in spans[max(0, low - 1):low + 2] if s[1] > 0]


def ints(got):
    assert got.dtype == np.int64 and got.ndim == 1
    return got.tolist()


@pytest.mark.parametrize("parallelization", [1, 2, 0])
def test_reader_whole_file_and_windows(native, corpus, parallelization):
    raw, wanted = corpus["raw"], corpus["wanted"]
    n = len(F.lines_of(raw, NL))
    with native.open(corpus["path"], parallelization=parallelization) as f:
        for (j, dl), want in wanted.items():
            assert ints(f.field_ints(j, delimiter=bytes([dl]))) == want, (j, dl)
        want = wanted[(2, TAB)]
        assert want[-1] == -12345 and raw[-1] != NL                 # the unterminated numeric tail
        assert sum(1 for w in want if w not in (NAN, NONE)) > 10_000 and want.count(NAN) > 500 and want.count(NONE) > 1000
        # windows that start and end at launch seams and one line off them, at and past the end, and empty ones
        starts = f.line_starts(range(n)).tolist()
        seam_lines = [max(k for k in range(n) if starts[k] <= b) for b in corpus["blocks"][1:-1]]
        windows = [(0, 1), (0, 3), (n - 1, 1), (n - 1, 5), (n - 3, 3), (n - 2, 10**12), (n, 1), (n + 5, 2), (7, 0), (0, 0), (1, None)]
        for a, b in zip(seam_lines, seam_lines[1:]):                # from the line on a seam, or one off it, to the next such line
            windows += [(a - 1, b - a + 1), (a, b - a), (a, b - a + 1), (a + 1, b - a + 1), (a + 1, b - a - 1)]
        windows += [(seam_lines[0], 1), (seam_lines[1] + 1, 1), (seam_lines[0], seam_lines[3] - seam_lines[0] + 2)]
        for first, count in windows:
            end = n if count is None else first + count
            assert ints(f.field_ints(2, first, count)) == want[first:end], (first, count)
        assert ints(f.field_ints(1, seam_lines[1], 4, delimiter=b" ")) == wanted[(1, ord(" "))][seam_lines[1]:seam_lines[1] + 4]
        assert f.tell() == 0                                        # positionless
    with native.IndexedBzip2File(corpus["path"], parallelization=parallelization) as f:
        assert ints(f.field_ints(2, 3, 20)) == wanted[(2, TAB)][3:23]


def test_small_files(native, corpus):
    folder = corpus["folder"]
    cases = [("small-empty.bz2", b""), ("small-newline.bz2", b"\n"), ("small-closed.bz2", b"a\t1\n\n"),
             ("small-tail.bz2", b"a\t5\nc\t-6\te\nf\t"), ("small-tabs.bz2", b"\t\t\n\t"), ("small-tail-number.bz2", b"7\t8\n9\t10"),
             ("small-same.bz2", b"k\t1\nk\t2\nq\nk\tw\n\nk\t-3")]
    for name, raw in cases:
        with native.open(TF.small_file(folder, name, raw), parallelization=1) as f:
            for j in (0, 1, 2):
                assert ints(f.field_ints(j)) == FN.words_of(raw, NL, TAB, j), (name, j)
                assert ints(f.field_ints(j, 1)) == FN.words_of(raw, NL, TAB, j)[1:], (name, j)
                for value_field in (0, 1, 2):
                    check_sums(f, raw, j, value_field)
            assert ints(f.field_ints(0, newline=b"\0", delimiter=b"\n")) == FN.words_of(raw, 0, NL, 0), name


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import numpy as np
import indexed_bzip2_amd as m

with m.open(sys.argv[2], parallelization=int(sys.argv[3])) as f:
    for field, first, count, delimiter in ((2, 0, None, b"\t"), (0, 0, None, b"\t"), (2, 100, 2000, b"\t"), (1, 0, None, b" "),
                                           (1023, 0, None, b"\t"), (2, 10**9, 5, b"\t"), (2, 3, 0, b"\t")):
        host = f.field_ints(field, first, count, delimiter)
        tensor = f.field_ints_to_tensor(field, first, count, delimiter)
        assert tensor.dtype == torch.int64 and tensor.is_cuda and tensor.dim() == 1
        assert tensor.cpu().numpy().tolist() == host.tolist(), (field, first, count)
        print(field, first, count, len(host))
    # the sum of a column on the device: mask the two sentinels (and here what would overflow an int64 sum)
    column = f.field_ints_to_tensor(2)
    numbers = column[(column > m.FIELD_NUMBER_MISSING) & (column < 10**12) & (column > -10**12)]
    host = f.field_ints(2)
    assert int(numbers.sum()) == sum(int(v) for v in host if -10**12 < v < 10**12) and len(numbers) > 1000
    assert f.tell() == 0
with m.IndexedBzip2File(sys.argv[2], parallelization=int(sys.argv[3])) as f:
    assert f.field_ints_to_tensor(2, 5, 50).cpu().numpy().tolist() == f.field_ints(2, 5, 50).tolist()
print("field number tensors ok")
"""


def test_tensor_forms_equal_the_host_forms(native, corpus):
    """In a process of its own that imports torch first; the host forms are pinned to the model above."""
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, corpus["path"], "0"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "field number tensors ok" in run.stdout and "2 0 None 0" not in run.stdout


# ------------------------------------------------------------------------------------------------ sums

def check_sums(f, raw, key_field, value_field, first=0, count=None, dl=TAB, seed=0):
    """sum_by_field and value_sums against the model's groups, exactly; returns the model's groups."""
    groups, missing = FN.group_sums(raw, NL, dl, key_field, value_field, first, count)
    lines, counts, numbers, sums, mins, maxs, got_missing = f.sum_by_field(key_field, value_field, first, count, bytes([dl]), seed=seed)
    assert lines.dtype == counts.dtype == numbers.dtype == np.uint64 and mins.dtype == maxs.dtype == np.int64
    assert isinstance(sums, list) and all(type(s) is int for s in sums) and isinstance(got_missing, int)
    where = (key_field, value_field, first, count)
    assert lines.tolist() == [g["line"] for g in groups], where
    assert counts.tolist() == [g["count"] for g in groups], where
    assert numbers.tolist() == [g["numbers"] for g in groups], where
    assert sums == [g["sum"] for g in groups], where
    assert mins.tolist() == [g["min"] for g in groups] and maxs.tolist() == [g["max"] for g in groups], where
    assert got_missing == missing, where
    return groups


def ranked(groups):
    order = sorted(range(len(groups)), key=lambda i: (-groups[i]["sum"], groups[i]["line"]))
    return [(groups[i]["key"], groups[i]["sum"], groups[i]["numbers"]) for i in order]


@pytest.mark.parametrize("parallelization", [1, 2, 0])
def test_sum_by_field_on_the_file(native, corpus, parallelization):
    raw = corpus["raw"]
    n = len(F.lines_of(raw, NL))
    with native.open(corpus["path"], parallelization=parallelization) as f:
        position = f.tell()
        groups = check_sums(f, raw, 0, 2)
        assert 250 < len(groups) <= 302 and any(g["numbers"] < g["count"] for g in groups) and any(g["key"] == b"" for g in groups)
        assert any(abs(g["sum"]) > 2**63 for g in groups)           # beyond int64: the 128-bit sum is needed
        assert check_sums(f, raw, 0, 2, seed=0xDEADBEEF) == groups   # a second seed gives the same groups
        check_sums(f, raw, 0, 0)                                    # key_field == value_field: host names are no numbers
        check_sums(f, raw, 2, 2)                                    # ... and numbers are: all keys nearly distinct
        check_sums(f, raw, 1, 2, dl=ord(" "))
        check_sums(f, raw, 0, 3)                                    # no line has a field 3: every group sums nothing
        check_sums(f, raw, 3, 2)                                    # no line has the key field: no group
        starts = f.line_starts(range(n)).tolist()
        seam = max(k for k in range(n) if starts[k] <= corpus["blocks"][2])
        for first, count in ((seam, 1), (seam - 1, 3), (seam + 1, 5000), (n - 3, 10), (n, 5), (10, 0), (5000, 7000)):
            check_sums(f, raw, 0, 2, first, count)
        assert f.tell() == position                                 # positionless
        # value_sums: by descending sum, then first occurrence; limit
        want = ranked(groups)
        assert f.value_sums(0, 2) == want and want[0][1] > 0 > want[-1][1]
        for limit in (0, 1, 20, 10**6):
            assert f.value_sums(0, 2, limit) == want[:limit], limit
        window = FN.group_sums(raw, NL, TAB, 0, 2, 100, 50)[0]
        assert f.value_sums(0, 2, 5, 100, 50) == ranked(window)[:5]
    with native.IndexedBzip2File(corpus["path"], parallelization=parallelization) as f:
        assert check_sums(f, raw, 0, 2) == groups
        assert f.value_sums(0, 2, 3) == want[:3]


def test_sums_beyond_int64_one_key_and_distinct_keys(native, corpus):
    folder = corpus["folder"]
    big = 9 * 10**17
    raw = b"".join(b"p\t%d\nn\t-%d\nz\t%d\n" % (big, big, big if k % 2 else -big) for k in range(20))
    with native.open(TF.small_file(folder, "big.bz2", raw), parallelization=0) as f:
        groups = check_sums(f, raw, 0, 1)
        assert [(g["key"], g["sum"]) for g in groups] == [(b"p", 20 * big), (b"n", -20 * big), (b"z", 0)] and 20 * big > 2**63
        assert f.value_sums(0, 1) == [(b"p", 20 * big, 20), (b"z", 0, 20), (b"n", -20 * big, 20)]
    # all lines share one key: one run of 200 000 elements in the reduction
    raw = b"".join(b"k\t%d\n" % (k * 7919 % 10**12 - 10**11) for k in range(200_000))
    with native.open(TF.small_file(folder, "one-key.bz2", raw, 1), parallelization=0) as f:
        groups = check_sums(f, raw, 0, 1)
        assert len(groups) == 1 and groups[0]["count"] == groups[0]["numbers"] == 200_000
        check_sums(f, raw, 0, 0)                                    # ... and no value is a number
        check_sums(f, raw, 0, 1, 1000, 150_000)
    # all keys distinct
    raw = b"".join(b"%d\t%d\tx\n" % (k, -k * k) for k in range(30_000))
    with native.open(TF.small_file(folder, "distinct.bz2", raw, 1), parallelization=0) as f:
        groups = check_sums(f, raw, 0, 1)
        assert len(groups) == 30_000 and all(g["count"] == 1 for g in groups)
        check_sums(f, raw, 0, 0)
        check_sums(f, raw, 2, 1)                                    # and again one key
    # lines without the key field, without the value field, and with a value that is no number
    raw = b"a\tx\t1\nb\n\nb\tx\t2\na\tx\nc\tx\tfive\nc\tx\t\nb\tx\t-3\na\tx\t+4\nd"
    with native.open(TF.small_file(folder, "holes.bz2", raw), parallelization=1) as f:
        groups = check_sums(f, raw, 0, 2)
        assert [(g["key"], g["count"], g["numbers"], g["sum"]) for g in groups] == [
            (b"a", 3, 2, 5), (b"b", 3, 2, -1), (b"", 1, 0, 0), (b"c", 2, 0, 0), (b"d", 1, 0, 0)]
        groups = check_sums(f, raw, 1, 2)
        assert [(g["key"], g["count"], g["numbers"], g["sum"], g["min"], g["max"]) for g in groups] == [(b"x", 7, 4, 4, -3, 4)]
        assert f.sum_by_field(1, 2)[6] == 3                         # "b", "" and "d" have no field 1


def test_one_decode_per_block(native, corpus):
    """sum_by_field decodes what field_hashes over the same range decodes: the existing call is the yardstick."""
    deltas = {}
    for name, call in (("sums", lambda f: f.sum_by_field(0, 2)), ("hashes", lambda f: f.field_hashes(0)),
                       ("sums-window", lambda f: f.sum_by_field(0, 2, 3000, 9000)), ("hashes-window", lambda f: f.field_hashes(0, 3000, 9000)),
                       ("ints", lambda f: f.field_ints(2)), ("spans", lambda f: f.field_spans(2))):
        with native.open(corpus["path"], parallelization=2) as f:
            f.count_lines()                                         # the line index is built: its decodes are not the call's
            before = f.statistics()["blocks_decoded"]
            call(f)
            deltas[name] = f.statistics()["blocks_decoded"] - before
    assert deltas["sums"] == deltas["hashes"] > 0 and deltas["sums-window"] == deltas["hashes-window"] > 0
    assert deltas["ints"] == deltas["spans"] == deltas["hashes"]
    # on a fresh reader, index and all
    fresh = {}
    for name, call in (("sums", lambda f: f.sum_by_field(0, 2)), ("hashes", lambda f: f.field_hashes(0))):
        with native.open(corpus["path"], parallelization=2) as f:
            before = f.statistics()["blocks_decoded"]
            call(f)
            fresh[name] = f.statistics()["blocks_decoded"] - before
    assert fresh["sums"] == fresh["hashes"] > deltas["sums"]


def test_held_results(native, corpus):
    """The numbers are held as the field hashes are: until the next call of their own family, whatever the other families
    do; field_sums releases them and holds its groups."""
    raw, lib = corpus["raw"], native.lib()
    want = corpus["wanted"][(2, TAB)]
    with native.open(corpus["path"], parallelization=0) as f:
        h = f._open_reader()._h
        n, missing = ctypes.c_uint64(), ctypes.c_uint64()

        def take(capacity, room=None):
            out = np.full(max(1, room or capacity), CANARY, dtype=np.int64)
            return lib.mi355x_bz2_reader_take_field_numbers(h, out.ctypes.data, capacity, 0), out.tolist()

        def take_sums(capacity):
            columns = [np.full(max(1, capacity), 77, dtype=dtype) for dtype in
                       (np.uint64, np.uint64, np.uint64, np.int64, np.uint64, np.uint64, np.int64, np.int64, np.int64)]
            return lib.mi355x_bz2_reader_take_field_sums(h, *[c.ctypes.data for c in columns], capacity), [c.tolist() for c in columns]
        assert take(4)[0] == INVALID_ARGUMENT and take_sums(4)[0] == INVALID_ARGUMENT                 # nothing was ever held
        assert lib.mi355x_bz2_reader_field_numbers(h, NL, TAB, 2, 10, 300, 0, ctypes.byref(n)) == OK and n.value == 300
        assert take(300) == (OK, want[10:310]) and take(300) == (OK, want[10:310]), "a second take repeats the first"
        assert take(5, 8) == (OK, want[10:15] + [CANARY] * 3)
        # the other families leave them alone
        f.line_hashes(0, 50)
        f.field_spans(1, 0, 50)
        f.field_hashes(0, 5, 50)
        f.count_by_field(0, 0, 1000)
        f.grep(b"host1", limit=3)
        assert f.read(100) == raw[:100]
        assert take(300) == (OK, want[10:310]) and take_sums(1)[0] == INVALID_ARGUMENT
        # field_sums releases the numbers and holds the groups
        groups, gone = FN.group_sums(raw, NL, TAB, 0, 2, 100, 500)
        assert lib.mi355x_bz2_reader_field_sums(h, NL, TAB, 0, 2, 0, 100, 500, ctypes.byref(n), ctypes.byref(missing)) == OK
        assert (n.value, missing.value) == (len(groups), gone) and take(1)[0] == INVALID_ARGUMENT
        status, columns = take_sums(len(groups))
        assert status == OK and take_sums(len(groups)) == (status, columns)
        starts = dict(zip(range(len(F.lines_of(raw, NL))), F.direct(raw, NL, TAB, 0)))
        assert columns[0] == [g["line"] for g in groups] and columns[1] == [g["count"] for g in groups]
        assert columns[2] == [starts[g["line"]][0] for g in groups] and columns[3] == [len(g["key"]) for g in groups]
        assert columns[4] == [g["numbers"] for g in groups]
        assert [(hi << 64) + lo for lo, hi in zip(columns[5], columns[6])] == [g["sum"] for g in groups]
        assert columns[7] == [g["min"] for g in groups] and columns[8] == [g["max"] for g in groups]
        assert take_sums(2) == (OK, [c[:2] for c in columns])
        assert lib.mi355x_bz2_reader_take_field_sums(h, *([None] * 9), len(groups)) == OK               # any of them may be NULL
        # the field-hash family keeps its own: count_by_field after field_sums, and the sums after count_by_field
        f.count_by_field(0, 0, 1000)
        assert take_sums(2) == (OK, [c[:2] for c in columns])
        # field_numbers releases the groups; an empty range holds an empty result
        assert lib.mi355x_bz2_reader_field_numbers(h, NL, TAB, 2, 10**9, 5, 0, ctypes.byref(n)) == OK and n.value == 0
        assert take_sums(1)[0] == INVALID_ARGUMENT and take(0)[0] == OK and take(3) == (OK, [CANARY] * 3)


def test_tool(native, corpus):
    raw = corpus["raw"]
    for options, key_field, value_field, dl in ((["--sum-by-field", "0,2"], 0, 2, TAB), (["--sum-by-field=0,2", "-P", "1"], 0, 2, TAB),
                                                (["--sum-by-field", "0,2", "--seed", "99"], 0, 2, TAB),
                                                (["--sum-by-field", "1,2", "--field-delimiter", " "], 1, 2, ord(" ")),
                                                (["--sum-by-field", "2,2", "--field-delimiter=\\x09"], 2, 2, TAB),
                                                (["--sum-by-field", "9,0"], 9, 0, TAB)):
        run = subprocess.run([CLI] + options + [corpus["path"]], capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr
        groups = FN.group_sums(raw, NL, dl, key_field, value_field)[0]
        assert run.stdout == b"".join(b"%d\t%d\t%s\n" % (g["sum"], g["numbers"], g["key"]) for g in groups), options
    big = 9 * 10**17
    raw = b"".join(b"p\t%d\nn\t-%d\n" % (big, big) for _ in range(20))
    run = subprocess.run([CLI, "--sum-by-field", "0,1", TF.small_file(corpus["folder"], "tool-big.bz2", raw)], capture_output=True, timeout=300)
    assert run.returncode == 0 and run.stdout == b"18000000000000000000\t20\tp\n-18000000000000000000\t20\tn\n"
