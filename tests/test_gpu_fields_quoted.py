"""Quoted field access on the GPU: the kernels under Decoder.field_spans(quote=) (k_field_chunks_quoted, k_field_link_quoted,
k_field_emit_quoted, k_field_sizes, k_field_unquote), the reader's quote= on field_spans / read_fields / read_columns and
their tensor forms, and the tool's --field-quote.

The reference is the plain Python model of fieldsquoted.py -- the definition's loop per line, and its own summarise and
stitch -- never the code under test.  Offsets, sizes and bytes are compared exactly."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import datagen
import fields as F
import fieldsquoted as Q
import readershapes as R
from fieldsquotedshapes import FIELDS, record, reader_corpus

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
NL, DL, QT = 10, ord(","), ord('"')
QUOTE = b'"'
ONES = 2**64 - 1
UNTOUCHED = -1 - 2**62
INVALID_ARGUMENT = 103
SIZES = (0, 1, 255, 256, 257, 65_535, 65_536, 65_537, 131_073)
EDGES = (255, 256, 257, 65_535, 65_536)
KEYS = ("count", "has_delimiter", "first_nl", "head_positions", "head_quote_parity", "tail_start", "tail_delims",
        "tail_field_start", "tail_field_end", "tail_in_quote", "tail_non_empty")


# ------------------------------------------------------------------------------------------------ the kernels

def device_text():
    """(text, {name: (offset, size)})."""
    rng = random.Random(0xC5F1E1D)
    parts, at, where = [], 0, {}

    def add(piece, name=None):
        nonlocal at
        if name is not None:
            where[name] = (at, len(piece))
        parts.append(piece)
        at += len(piece)

    def filler(n):
        out = bytearray()
        while len(out) < n:
            out += record(rng) + b"\n"
        return bytes(out[:n - 1]) + b"\n"

    def noise(n):
        return bytes(rng.choice(b"abcdefgh\0\xff ") for _ in range(n))

    add(filler(max(SIZES) + 40), "lines")
    # one record behind 70 000 bytes of lines: spans are placed so that its bytes fall on the edges
    add(b'aaa,"bb,b""c,c",dd\n', "record")
    add(filler(70_000), "behind")
    # the content rule: "x", "", a lone quote, "a, a", "a"b, and a field that opens a quote that never closes
    add(b'"x","",z\nq,"\n"a\na"\n"a"b,c\nk,"open,,\n', "trim")
    # quoted fields longer than a tile, full of delimiters: the in-quote state crosses tiles, and the field's first and
    # last bytes lie in different tiles
    for n in (70_000, 200_000):
        inner = bytearray(noise(n))
        for k in range(0, n, 7):
            inner[k] = DL
        add(b"x," + b'"' + bytes(inner) + b'"' + b",y,z", "line-%d" % n)
        add(b"\n")
    add(filler(1000))
    return b"".join(parts), where


def decoded(native, text):
    enc = datagen.compress(text, 9)
    dec = native.Decoder(device=0)
    dec.set_input(enc)
    results, total = dec.decode_batch(native.find_magic(enc))
    assert total == len(text) and dec.copy_output(0, total) == text
    return dec


@pytest.fixture(scope="module")
def device(native):
    text, where = device_text()
    dec = decoded(native, text)
    yield {"dec": dec, "text": text, "where": where, "models": {}}
    dec.close()


def model_of(device, span, field, nl=NL, dl=DL, q=QT):
    """The model's summary of a span, computed once per (span, field, nl, dl, q), shared, left unchanged."""
    key = (span, field, nl, dl, q)
    if key not in device["models"]:
        device["models"][key] = Q.summarise_chunk(device["text"][span[0]:span[0] + span[1]], nl, dl, q, field)
    return device["models"][key]


def contents_of(device, span, model, q=QT):
    """The model's closed lines of a span as contents, offsets in the output."""
    piece = device["text"][span[0]:span[0] + span[1]]
    return [(span[0] + s, n) for s, n in (Q.content_of(piece, raw, q) for raw in model["fields"])]


def check_spans(device, spans, field=1, nl=NL, dl=DL, q=QT, capacity=None, room=None):
    """Summaries (raw), starts and sizes (contents) of Decoder.field_spans(quote=) against the model, exactly."""
    models = [model_of(device, span, field, nl, dl, q) for span in spans]
    summaries, starts, sizes = device["dec"].field_spans(spans, field, bytes([dl]), bytes([nl]), capacity, room, quote=bytes([q]))
    assert starts.dtype == np.uint64 and sizes.dtype == np.int64
    for span, model, got in zip(spans, models, summaries):
        assert got == {key: model[key] for key in KEYS}, (span, field)
    wanted = [pair for span, model in zip(spans, models) for pair in contents_of(device, span, model, q)]
    written = len(wanted) if capacity is None else min(capacity, len(wanted))
    assert starts[:written].tolist() == [s for s, _ in wanted[:written]], (spans[:3], field)
    assert sizes[:written].tolist() == [n for _, n in wanted[:written]], (spans[:3], field)
    assert (starts[written:] == ONES).all() and (sizes[written:] == UNTOUCHED).all(), "written at or beyond the capacity"
    return wanted


def test_span_sizes_at_every_alignment(native, device):
    base = device["where"]["lines"][0]
    base += -base % 16                                              # the output buffer is 16-byte aligned
    spans = [(base + start, size) for start in range(16) for size in SIZES]
    assert {o % 16 for o, _ in spans} == set(range(16))
    wanted = check_spans(device, spans)
    raw = [pair for span in spans for pair in ((span[0] + s, n) for s, n in model_of(device, span, 1)["fields"])]
    assert len(wanted) > 10_000 and 1000 < sum(1 for _, size in wanted if size < 0) < len(wanted) - 1000
    assert sum(1 for a, b in zip(wanted, raw) if a != b) > 500          # the trim matters
    for field in (0, 2, 7, 1023):
        check_spans(device, spans[::7], field)
    # other bytes in the three roles
    check_spans(device, spans[3::11], 1, dl=ord(" "))
    check_spans(device, spans[5::11], 0, nl=0)
    check_spans(device, spans[5::11], 1, q=ord("a"))
    check_spans(device, spans[7::11], 1, nl=ord('"'), dl=ord(","), q=NL)
    # the whole output as one span, and the same span twice with another between: the trim finds each line's span
    whole = (0, len(device["text"]))
    check_spans(device, [whole, spans[20], (5, 0), whole, (9, 0)])
    check_spans(device, [whole], 0)


def test_quotes_and_quoted_delimiters_on_chunk_and_tile_edges(device):
    text = device["text"]
    offset, size = device["where"]["record"]
    assert text[offset:offset + size] == b'aaa,"bb,b""c,c",dd\n' and text[offset - 1] == NL
    places = {"opening quote": 4, "closing quote": 14, "first of a doubled quote": 9, "second of a doubled quote": 10,
              "delimiter inside quotes": 7, "delimiter inside quotes behind the doubled quote": 12}
    for name, k in places.items():
        p = offset + k
        assert text[p] == (DL if "delimiter" in name else QT)
        for edge in EDGES:
            for field in (0, 1, 2) if edge in (256, 65_536) else (1,):
                # the byte at exactly this offset of a span, as the span's last byte, and as its first
                wanted = check_spans(device, [(p - edge, edge + 300), (p - edge, edge + 1), (p, 300)], field)
                assert (offset + 5, 9) in wanted or field != 1, (name, edge)


def test_quoted_fields_longer_than_a_tile(device):
    text, where = device["text"], device["where"]
    for length in (70_000, 200_000):
        offset, size = where["line-%d" % length]
        assert size == length + 8 and text[offset - 1] == NL and text[offset + size] == NL
        assert text.count(b",", offset, offset + size) > length // 7
        for field in (0, 1, 2, 3, 4):
            # the line whole; entered inside its quoted field and outside it; and as the head of a span that goes on
            check_spans(device, [(offset, size + 1), (offset + 12_345, size + 1 - 12_345), (offset + size - 2, 3),
                                 (offset - 1, size + 300)], field)
        # its first and last bytes lie in different tiles of the span
        assert check_spans(device, [(offset, size + 1)], 1) == [(offset + 3, length)]
        assert check_spans(device, [(offset, size + 1)], 3) == [(offset + size - 1, 1)]
        assert check_spans(device, [(offset, size + 1)], 4) == [(offset + size, -1)]
    # many spans in one call, each its own workgroup of the link and its own search of the trim
    check_spans(device, [(offset + 7 * k, 1 + k % 3) for k in range(600)], 0)
    start = where["trim"][0]
    check_spans(device, [(start + k, 12) for k in range(40)], 0)


def test_the_trim(device):
    offset, size = device["where"]["trim"]
    span = (offset, size)
    assert check_spans(device, [span], 0) == [(offset + 1, 1), (offset + 9, 1), (offset + 13, 2), (offset + 16, 2), (offset + 19, 4),
                                              (offset + 26, 1)]
    assert check_spans(device, [span], 1) == [(offset + 5, 0), (offset + 11, 1), (offset + 15, -1), (offset + 18, -1), (offset + 24, 1),
                                              (offset + 28, 7)]
    assert check_spans(device, [span], 2)[0] == (offset + 7, 1)
    # every start of a span inside these lines
    check_spans(device, [(offset + k, size - k) for k in range(size)], 0)
    check_spans(device, [(offset + k, size - k) for k in range(size)], 1)


def test_spans_that_begin_inside_and_outside_quotes_stitch_to_the_whole(device):
    """Consecutive spans cut at every kind of place: their summaries, stitched by the model's rule, are the model on the
    whole.  The lines the stitch patches are raw; every other line is the content the launch wrote."""
    text, where = device["text"], device["where"]
    rng = random.Random(5)
    begin = where["record"][0]
    end = where["line-70000"][0] + where["line-70000"][1] + 1
    inside = where["line-70000"][0] + 30_000
    record = where["record"][0]
    cuts = sorted({begin, end, inside, inside + 1, inside + 9, record + 5, record + 10, record + 15, where["trim"][0] + 11}
                  | {rng.randrange(begin, end) for _ in range(40)})
    piece = text[begin:end]
    spans = [(a, b - a) for a, b in zip(cuts, cuts[1:])]
    starts_of_lines = [0] + [k + 1 for k in range(len(piece)) if piece[k] == NL]
    for field in (0, 1, 2):
        summaries, starts, sizes = device["dec"].field_spans(spans, field, b",", b"\n", quote=QUOTE)
        at = 0
        for (offset, size), s in zip(spans, summaries):
            s["size"] = size
            s["fields"] = [(int(a) - offset, int(n)) for a, n in zip(starts[at:at + s["count"]], sizes[at:at + s["count"]])]
            at += s["count"]
        assert at == len(starts) == piece.count(b"\n")
        # some of the spans begin inside quotes and some outside
        assert {piece[piece.rfind(b"\n", 0, c - begin) + 1:c - begin].count(b'"') % 2 for c in cuts[1:-1]} == {0, 1}
        got = Q.stitch(summaries, field)
        raw, content = Q.raw_direct(piece, NL, DL, QT, field), Q.direct(piece, NL, DL, QT, field)
        assert len(got) == len(raw)
        patched = 0
        for k, pair in enumerate(got):
            first, last = starts_of_lines[k], starts_of_lines[k + 1] - 1        # the line's first byte and its nl
            crosses = any(first < c - begin <= last for c in cuts[1:-1])
            patched += crosses
            assert pair == (raw[k] if crosses else content[k]), (field, k, crosses)
        assert patched > 10


def test_capacity_smaller_than_the_count(native, device):
    offset, _ = device["where"]["lines"]
    spans = [(offset + 3, 70_000), (offset + 70_003, 5_000)]
    total = len(check_spans(device, spans))
    assert total > 2 * 257                                          # well beyond every capacity tried below
    for capacity in (0, 1, 2, 255, 256, total - 1, total):
        check_spans(device, spans, capacity=capacity, room=total + 64)
    check_spans(device, spans, 0, capacity=257, room=total + 64)
    assert device["dec"].field_spans([], 1, b",", quote=QUOTE)[0] == []
    with pytest.raises(Exception):
        device["dec"].field_spans([(len(device["text"]) - 5, 6)], 1, b",", quote=QUOTE)
    for field, delimiter, newline, quote in ((1024, b",", b"\n", b'"'), (0, b",", b"\n", b","), (0, b",", b"\n", b"\n"),
                                             (0, b",", b"\n", b""), (0, b",", b"\n", b'""')):
        with pytest.raises(ValueError):
            device["dec"].field_spans([(0, 10)], field, delimiter, newline, quote=quote)
    # the C call refuses the same before anything is launched: nothing is written, and the context goes on working
    lib, N = native.lib(), native._native
    span = (N.ByteSpan * 1)(N.ByteSpan(0, 10))
    summary = (N.QuotedFieldSummary * 1)()
    summary[0].count = 77
    for nl, dl, quote, field in ((10, 44, 10, 0), (10, 44, 44, 0), (10, 10, 34, 0), (10, 44, 34, 1024)):
        rc = lib.mi355x_bz2_field_spans_quoted(device["dec"]._h, span, 1, nl, dl, quote, field, summary, None, None, None, 0)
        assert rc == INVALID_ARGUMENT and summary[0].count == 77, (nl, dl, quote, field)
    check_spans(device, spans[:1], capacity=3, room=8)


def test_a_span_of_more_than_256_tiles(native):
    """Just over 16 MiB in one span are more tiles than one step of k_field_link_quoted scans, and the quoted field
    crosses the step: it opens in the first step and closes in the second, with delimiters inside it in both.  Runs of
    one byte, so that the file is small."""
    rng = random.Random(7)
    front = b"".join(record(rng) + b"\n" for _ in range(60))
    text = front + b'x,y,"' + b"a" * 9_000_000 + b",,," + b'""' + b"b" * 8_000_000 + b'",c\n' + front + b'no newline,"at, the end'
    assert len(text) > 257 * 65_536
    dec = decoded(native, text)
    try:
        device = {"dec": dec, "text": text, "models": {}}
        long_at, n = len(front), text.count(b"\n")
        for field in (0, 1, 2, 3, 4):
            wanted = check_spans(device, [(0, len(text))], field)
            assert len(wanted) == n and wanted[60][0] >= long_at
        assert check_spans(device, [(0, len(text))], 2)[60] == (long_at + 5, 17_000_005)
        assert check_spans(device, [(0, len(text))], 3)[60] == (long_at + 5 + 17_000_005 + 2, 1)
        # the line entered inside its quoted field, in a span that starts off the 16-byte grid, and the head of another
        check_spans(device, [(long_at + 1_000_001, len(text) - long_at - 1_000_001), (3, 17_000_000)], 2)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ the reader

@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("fieldsquoted")
    files = {}
    for variant in ("tail", "closed"):
        raw, enc, planted, run_at, parts = reader_corpus(variant)
        path = folder / (variant + ".bz2")
        path.write_bytes(enc)
        # computed once, shared, left unchanged
        files[variant] = {"raw": raw, "path": str(path), "planted": planted, "run_at": run_at,
                          "block_starts": R.data_block_starts(parts),
                          "spans": {j: Q.direct(raw, NL, DL, QT, j) for j in FIELDS},
                          "values": {j: Q.fields_of(raw, NL, DL, QT, j) for j in FIELDS},
                          "plain": {j: F.direct(raw, NL, DL, j) for j in FIELDS},
                          "newlines": [k for k in range(len(raw)) if raw[k] == NL]}
    return {"files": files, "folder": folder}


def pairs(spans):
    starts, sizes = spans
    assert starts.dtype == np.uint64 and sizes.dtype == np.int64 and len(starts) == len(sizes)
    return list(zip(starts.tolist(), sizes.tolist()))


def line_of(entry, offset):
    return int(np.searchsorted(entry["newlines"], offset, "left"))


@pytest.mark.parametrize("parallelization", [1, 2, 3, 5, 0])
@pytest.mark.parametrize("variant", ["tail", "closed"])
def test_reader_whole_file_and_windows(native, corpus, variant, parallelization):
    entry = corpus["files"][variant]
    raw = entry["raw"]
    n = len(F.lines_of(raw, NL))
    assert n == raw.count(b"\n") + (variant == "tail")
    with native.open(entry["path"], parallelization=parallelization) as f:
        for j in FIELDS:
            assert pairs(f.field_spans(j, delimiter=b",", quote=QUOTE)) == entry["spans"][j], j
            # without the keyword, and with None, today's call
            assert pairs(f.field_spans(j, delimiter=b",")) == entry["plain"][j], j
            assert pairs(f.field_spans(j, delimiter=b",", quote=None)) == entry["plain"][j], j
        assert f.read_fields(2, delimiter=b",", quote=QUOTE) == entry["values"][2]
        assert f.read_fields(2, delimiter=b",") == F.fields_of(raw, NL, DL, 2)
        columns = f.read_columns([0, 2, 2, 5], delimiter=b",", quote=QUOTE)
        assert columns == [entry["values"][j] for j in (0, 2, 2, 5)]
        assert f.read_columns([2, 5], delimiter=b",") == [F.fields_of(raw, NL, DL, j) for j in (2, 5)]
        # windows: starting and ending on the planted lines, around the long quoted field, at and past the end, empty
        seams = sorted(line_of(entry, b) for b in entry["planted"])
        long_line = line_of(entry, entry["run_at"])
        windows = [(0, 1), (0, 3), (seams[0], 1), (seams[1] - 1, 3), (seams[2] + 1, 1), (seams[3], seams[6] - seams[3] + 2),
                   (long_line, 1), (long_line - 1, 3), (long_line + 1, 2), (n - 1, 1), (n - 1, 5), (n - 3, 3), (n - 2, 10**12),
                   (n, 1), (n + 5, 2), (7, 0), (1, None), (n // 2, None)]
        for first, count in windows:
            end = n if count is None else first + count
            assert pairs(f.field_spans(2, first, count, delimiter=b",", quote=QUOTE)) == entry["spans"][2][first:end], (first, count)
        for first, count in windows[2:9] + windows[9:14]:
            assert f.read_fields(5, first, count, delimiter=b",", quote=QUOTE) == entry["values"][5][first:first + count], (first, count)
            got = f.read_columns([0, 2, 2, 5], first, count, delimiter=b",", quote=QUOTE)
            assert got == [entry["values"][j][first:first + count] for j in (0, 2, 2, 5)], (first, count)
        assert f.tell() == 0                                        # positionless
    with native.IndexedBzip2File(entry["path"], parallelization=parallelization) as f:
        assert pairs(f.field_spans(2, 3, 20, delimiter=b",", quote=QUOTE)) == entry["spans"][2][3:23]
        assert f.read_fields(1, 3, 20, delimiter=b",", quote=QUOTE) == entry["values"][1][3:23]
        assert f.read_columns([5, 0], 3, 20, delimiter=b",", quote=QUOTE) == [entry["values"][j][3:23] for j in (5, 0)]


def test_small_files(native, corpus):
    folder = corpus["folder"]
    cases = [("q-empty.bz2", b""), ("q-newline.bz2", b"\n"), ("q-closed.bz2", b'"a,b",c\n\n'), ("q-tail.bz2", b'a,"b\nc,"d,e"\n"f,'),
             ("q-quotes.bz2", b'"",""""\n"\n""'), ("q-trim.bz2", b'"x","","\n"a\na"\n"a"b,c\nk,"open,,')]
    for name, raw in cases:
        path = folder / name
        path.write_bytes(datagen.compress(raw, 9))
        with native.open(str(path), parallelization=1) as f:
            for j in (0, 1, 2):
                assert pairs(f.field_spans(j, delimiter=b",", quote=QUOTE)) == Q.direct(raw, NL, DL, QT, j), (name, j)
                assert f.read_fields(j, delimiter=b",", quote=QUOTE) == Q.fields_of(raw, NL, DL, QT, j), (name, j)
                assert pairs(f.field_spans(j, 1, delimiter=b",", quote=QUOTE)) == Q.direct(raw, NL, DL, QT, j)[1:], (name, j)
            assert f.read_columns([1, 0], delimiter=b",", quote=QUOTE) == [Q.fields_of(raw, NL, DL, QT, j) for j in (1, 0)], name
            assert pairs(f.field_spans(0, delimiter=b"\n", newline=b",", quote=b"a")) == Q.direct(raw, DL, NL, ord("a"), 0), name


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import numpy as np
import indexed_bzip2_amd as m

q = b'"'
with m.open(sys.argv[2], parallelization=int(sys.argv[3])) as f:
    for field, first, count in ((0, 0, None), (2, 0, None), (5, 100, 700), (2, 10**9, 5), (2, 3, 0)):
        starts, sizes = f.field_spans(field, first, count, b",", quote=q)
        got = f.field_spans_to_tensor(field, first, count, b",", quote=q)
        for tensor, host in zip(got, (starts, sizes)):
            assert tensor.dtype == torch.int64 and tensor.is_cuda and tensor.dim() == 1
            assert tensor.cpu().numpy().tolist() == host.tolist(), (field, first, count)
        fields = f.read_fields(field, first, count, b",", quote=q)
        data, offsets = f.read_fields_to_tensor(field, first, count, b",", quote=q)
        assert data.dtype == torch.uint8 and data.is_cuda and offsets.dtype == torch.int64 and not offsets.is_cuda
        blob, bounds = bytes(data.cpu().numpy()), offsets.tolist()
        assert [blob[a:b] for a, b in zip(bounds, bounds[1:])] == [x or b"" for x in fields], (field, first, count)
        assert [b - a for a, b in zip(bounds, bounds[1:])] == [max(int(n), 0) for n in sizes]
        print(field, first, count, len(fields))
    for first, count in ((0, None), (100, 700)):
        host = f.read_columns([0, 2, 2, 5], first, count, b",", quote=q)
        device = f.read_columns_to_tensor([0, 2, 2, 5], first, count, b",", quote=q)
        for column, (data, offsets, sizes) in zip(host, device):
            assert data.is_cuda and offsets.is_cuda and sizes.is_cuda
            blob, bounds, present = bytes(data.cpu().numpy()), offsets.tolist(), sizes.tolist()
            assert [blob[a:b] if n >= 0 else None for a, b, n in zip(bounds, bounds[1:], present)] == column
    assert f.tell() == 0
print("quoted field tensors ok")
"""


@pytest.mark.parametrize("parallelization", [2, 0])
def test_tensor_forms_equal_the_host_forms(native, corpus, parallelization):
    """In a process of its own that imports torch first; the host forms are pinned to the model above."""
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, corpus["files"]["tail"]["path"], str(parallelization)],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "quoted field tensors ok" in run.stdout and "0 0 None 0" not in run.stdout


def test_tool(native, corpus):
    entry = corpus["files"]["tail"]
    values = entry["values"]
    run = subprocess.run([CLI, "--cut-fields", "0,2", "--field-delimiter", ",", "--field-quote", '"', entry["path"]],
                         capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert run.stdout == b"".join((a or b"") + b"," + (b or b"") + b"\n" for a, b in zip(values[0], values[2]))
    run = subprocess.run([CLI, "--cut-field", "2", "--field-delimiter=,", "--field-quote=\\x22", "-P", "2", entry["path"]],
                         capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert run.stdout == b"".join((field or b"") + b"\n" for field in values[2])
