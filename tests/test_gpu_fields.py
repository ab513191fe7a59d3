"""Field access on the GPU: the kernels under Decoder.field_spans (k_field_chunks, k_field_link, k_field_emit,
k_field_sizes), the reader's field_spans / field_spans_to_tensor / read_fields / read_fields_to_tensor, and the tool's
--cut-field.

The reference is the plain Python model of fields.py -- bytes.split per line, and its own summarise and stitch -- never
the code under test.  Offsets, sizes and bytes are compared exactly."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, FIXTURES, fixture_names, read_fixture
import datagen
import fields as F

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
NL, TAB = 10, 9
ONES = 2**64 - 1
UNTOUCHED = -1 - 2**62
SIZES = (0, 1, 255, 256, 257, 65_535, 65_536, 65_537, 131_073)
EDGES = (255, 256, 257, 511, 512, 65_535, 65_536)
KEYS = ("count", "has_delimiter", "first_nl", "head_positions", "tail_start", "tail_delims", "tail_field_start",
        "tail_field_end", "tail_non_empty")


# ------------------------------------------------------------------------------------------------ the kernels

def device_text():
    """(text, {name: (offset, size)})."""
    rng = random.Random(0xF1E1D)
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
            out += bytes(rng.choice(b"aab\t\t,xyz \0\xff") for _ in range(rng.choice([0, 0, 1, 3, 8, 20, 60, 300]))) + b"\n"
        return bytes(out[:n - 1]) + b"\n"

    def noise(n):
        return bytes(rng.choice(b"abcdefgh\0\xff ") for _ in range(n))

    def long_line(n, delimiters):
        line = bytearray(noise(n))
        for k in delimiters:
            line[k] = TAB
        return bytes(line)

    add(filler(max(SIZES) + 40), "lines")
    # nl, then dl, at the edges of chunks and of a tile, counted from the region's start, and nowhere else
    for name, value in (("edges-nl", NL), ("edges-dl", TAB)):
        add(noise(-at % 16))                                        # the region starts at a 16-byte boundary
        edges = bytearray(noise(EDGES[-1] + 600))
        for k in EDGES:
            edges[k] = value
        add(bytes(edges) + b"\n", name)
    add(b"\n" * 700, "empty-lines")
    add(noise(3 * 256 + 9), "no-dl")
    add(b"\n")
    add(b"\t" * 2100, "only-dl")
    add(b"\n")
    add(noise(300) + b"\n" + noise(500), "one-nl")
    add(b"\n")
    # lines longer than a tile: field 1 inside one tile (and fields up to 9, far apart), field 1 across the tile edge at
    # 65 536 of a span that starts with the line, and no field 1 at all
    for n in (70_000, 200_000):
        add(long_line(n, [100, 200] + [200 + (n - 300) * k // 8 for k in range(1, 8)]), "line-%d-inside" % n)
        add(b"\n")
        add(long_line(n, [65_000, 66_000]), "line-%d-straddling" % n)
        add(b"\n")
        add(long_line(n, []), "line-%d-missing" % n)
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


def model_of(device, span, field, nl, dl):
    """The model's summary of a span, computed once per (span, field, nl, dl), shared, left unchanged."""
    key = (span, field, nl, dl)
    if key not in device["models"]:
        device["models"][key] = F.summarise_chunk(device["text"][span[0]:span[0] + span[1]], nl, dl, field)
    return device["models"][key]


def check_spans(device, spans, field=1, nl=NL, dl=TAB, capacity=None, room=None):
    """Summaries, starts and sizes of Decoder.field_spans against the model, exactly; returns the model's fields."""
    models = [model_of(device, span, field, nl, dl) for span in spans]
    summaries, starts, sizes = device["dec"].field_spans(spans, field, bytes([dl]), bytes([nl]), capacity, room)
    assert starts.dtype == np.uint64 and sizes.dtype == np.int64
    for span, model, got in zip(spans, models, summaries):
        assert got == {key: model[key] for key in KEYS}, (span, field)
    wanted = [(span[0] + start, size) for span, model in zip(spans, models) for start, size in model["fields"]]
    written = len(wanted) if capacity is None else min(capacity, len(wanted))
    assert starts[:written].tolist() == [s for s, _ in wanted[:written]], (spans[:3], field)
    assert sizes[:written].tolist() == [n for _, n in wanted[:written]], (spans[:3], field)
    assert (starts[written:] == ONES).all() and (sizes[written:] == UNTOUCHED).all(), "written at or beyond the capacity"
    return wanted


def test_span_sizes_at_every_alignment(native, device):
    assert native._native.field_chunk_bytes() == 256
    base = device["where"]["lines"][0]
    base += -base % 16                                              # the output buffer is 16-byte aligned
    spans = [(base + start, size) for start in range(16) for size in SIZES]
    assert {o % 16 for o, _ in spans} == set(range(16))
    wanted = check_spans(device, spans)
    assert len(wanted) > 10_000 and 1000 < sum(1 for _, size in wanted if size < 0) < len(wanted) - 1000
    for field in (0, 7, 1023):
        check_spans(device, spans[::7], field)
    # other delimiters: ',' between fields; 0 between lines, "\n" then a byte like any other
    check_spans(device, spans[3::11], 1, dl=ord(","))
    check_spans(device, spans[5::11], 0, nl=0)
    check_spans(device, spans[5::11], 1, nl=0, dl=NL)
    # the whole output as one span, and the same span twice
    whole = (0, len(device["text"]))
    check_spans(device, [whole, spans[20], whole])
    check_spans(device, [whole], 0)


def test_delimiters_on_chunk_and_tile_edges(device):
    text = device["text"]
    for name, value in (("edges-nl", NL), ("edges-dl", TAB)):
        offset, size = device["where"][name]
        assert offset % 16 == 0 and all(text[offset + k] == value for k in EDGES)
        assert text.count(bytes([value]), offset, offset + size) == len(EDGES) + (value == NL)
        for field in (0, 1, 7):
            # the delimiters at exactly these offsets of a span, and one and two bytes in front of them
            check_spans(device, [(offset + shift, size - shift) for shift in (0, 1, 2)], field)
        # a delimiter as a span's first byte, as its last byte, and as all of it
        for k in EDGES:
            spans = [(offset + k, 300), (offset + k - 299, 300), (offset + k, 1), (offset + k, EDGES[-1] + 300 - k)]
            check_spans(device, spans, 0)
            check_spans(device, spans, 1)
    # the two roles swapped: the tabs close the lines and the newlines part the fields
    for name in ("edges-nl", "edges-dl"):
        check_spans(device, [device["where"][name]], 1, nl=TAB, dl=NL)
        check_spans(device, [device["where"][name]], 0, nl=TAB, dl=NL)


def test_empty_lines_and_lines_without_and_of_delimiters(device):
    where = device["where"]
    offset, size = where["empty-lines"]
    wanted = check_spans(device, [(offset, size), (offset + 1, 255), (offset + 3, 256), (offset + 5, 513)], 0)
    assert wanted[:700] == [(offset + k, 0) for k in range(700)]
    wanted = check_spans(device, [(offset, size)], 1)
    assert wanted == [(offset + k, -1) for k in range(700)]
    none, only, one = where["no-dl"], where["only-dl"], where["one-nl"]
    for field in (0, 1, 7, 1023):
        check_spans(device, [none, (none[0], none[1] + 1), only, (only[0], only[1] + 1), (only[0] + 700, only[1] - 699), one,
                             (one[0] + 301, one[1] - 301)], field)
    # a line of 2 100 tabs has 2 101 empty fields; without its newline the span closes nothing and knows both ends
    assert check_spans(device, [(only[0], only[1] + 1)], 1023) == [(only[0] + 1023, 0)]
    summaries, _, _ = device["dec"].field_spans([only, none], 1023)
    assert summaries[0]["tail_delims"] == 1024 and summaries[0]["tail_field_start"] == summaries[0]["tail_field_end"] == 1023
    assert len(summaries[0]["head_positions"]) == 1024 and not summaries[0]["has_delimiter"]
    assert summaries[1]["tail_delims"] == 0 and summaries[1]["tail_field_start"] is None and summaries[1]["head_positions"] == []
    assert check_spans(device, [(none[0], none[1] + 1)], 0) == [(none[0], none[1])]
    assert check_spans(device, [(none[0], none[1] + 1)], 1) == [(none[0] + none[1], -1)]


@pytest.mark.parametrize("length", [70_000, 200_000])
def test_lines_longer_than_a_tile(device, length):
    text, where = device["text"], device["where"]
    for kind in ("inside", "straddling", "missing"):
        offset, size = where["line-%d-%s" % (length, kind)]
        assert size == length and text[offset - 1] == NL and text[offset + size] == NL and NL not in text[offset:offset + size]
        for field in (0, 1, 7):
            # the line whole, closed by its newline; entered in its middle; and as the head of a span that goes on
            wanted = check_spans(device, [(offset, size + 1), (offset + 12_345, size + 1 - 12_345), (offset - 1, size + 300)], field)
            parts = text[offset:offset + size].split(b"\t")
            if field < len(parts):
                assert wanted[0] == (offset + sum(len(p) + 1 for p in parts[:field]), len(parts[field])), (kind, field)
            else:
                assert wanted[0] == (offset + size, -1), (kind, field)
    offset, size = where["line-%d-straddling" % length]
    assert check_spans(device, [(offset, size + 1)], 1) == [(offset + 65_001, 999)]         # across the tile edge at 65 536
    offset, size = where["line-%d-inside" % length]
    assert check_spans(device, [(offset, size + 1)], 1) == [(offset + 101, 99)]
    # many spans in one call, each its own workgroup of the link
    check_spans(device, [(offset + 7 * k, 1 + k % 3) for k in range(600)], 0)
    check_spans(device, [(offset + 95 + k, 10) for k in range(120)], 1)


def test_capacity_smaller_than_the_count(device):
    offset, _ = device["where"]["lines"]
    spans = [(offset + 3, 70_000), (offset + 70_003, 5_000)]
    total = len(check_spans(device, spans))
    assert total > 1000
    for capacity in (0, 1, 2, 255, 256, total - 1, total):
        check_spans(device, spans, capacity=capacity, room=total + 64)
    check_spans(device, spans, 0, capacity=257, room=total + 64)
    # nothing is asked for: no span; spans outside the output and arguments out of range are refused
    assert device["dec"].field_spans([], 1)[0] == []
    with pytest.raises(Exception):
        device["dec"].field_spans([(len(device["text"]) - 5, 6)], 1)
    for field, delimiter, newline in ((1024, b"\t", b"\n"), (-1, b"\t", b"\n"), (0, b"\n", b"\n"), (0, b"", b"\n"), (0, b"\t", b"ab")):
        with pytest.raises(ValueError):
            device["dec"].field_spans([(0, 10)], field, delimiter, newline)


def test_a_span_of_more_than_256_tiles(native):
    """Just over 16 MiB in one span are more tiles than one step of k_field_link scans, and the long line crosses the
    step: its field 3 starts in the first step and ends in the second.  Runs of one byte, so that the file is small."""
    rng = random.Random(7)
    front = b"".join(bytes(rng.choice(b"ab\t") for _ in range(rng.randrange(30))) + b"\n" for _ in range(60))
    text = front + b"x\ty\t" + b"a" * 9_000_000 + b"\t" + b"b" * 8_000_000 + b"\tc\n" + front + b"no newline\tat the end"
    assert len(text) > 257 * 65_536
    dec = decoded(native, text)
    try:
        device = {"dec": dec, "text": text, "models": {}}
        long_at = len(front)
        for field in (0, 1, 2, 3, 4, 5):
            wanted = check_spans(device, [(0, len(text))], field)
            assert wanted[60][0] >= long_at and len(wanted) == 121
        assert check_spans(device, [(0, len(text))], 3)[60] == (long_at + 4 + 9_000_001, 8_000_000)
        # the line entered behind its second tab, in a span that starts off the 16-byte grid
        check_spans(device, [(long_at + 5, len(text) - long_at - 5), (3, 17_000_000)], 1)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ the reader

def reader_text(tail=True):
    """About 700 kB of records: tab-separated lines of 0 to 12 fields, some with commas, runs of empty lines, one line
    of 250 kB -- longer than two 100 kB blocks -- with its tabs far apart, and an unterminated tail or none."""
    rng = random.Random(0x5EED)
    out = bytearray()

    def records(n):
        while n > 0:
            kind = rng.randrange(10)
            if kind == 0:
                line = b"\n" * rng.randrange(1, 4)
            elif kind == 1:
                line = bytes(rng.choice(b"ab\0\xff,\t") for _ in range(rng.randrange(1, 600))) + b"\n"
            else:
                fields = [b"%d" % len(out)] + [bytes(rng.choice(b"abcdefghij,") for _ in range(rng.randrange(12)))
                                                for _ in range(rng.randrange(12))]
                line = b"\t".join(fields) + b"\n"
            out.extend(line)
            n -= len(line)
    records(300_000)
    long_line = bytearray(rng.choice(b"abcdefgh \0\xff") for _ in range(250_000))
    for k in (5, 90_000, 90_001, 230_000):
        long_line[k] = TAB
    out.extend(long_line + b"\n")
    records(150_000)
    return bytes(out) + (b"the\ttail has\tno newline" if tail else b"")


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("fields")
    files = {}
    for name, raw in (("tail", reader_text(True)), ("closed", reader_text(False))):
        path = folder / (name + ".bz2")
        path.write_bytes(datagen.compress(raw, 1))
        # computed once, shared, left unchanged
        wanted = {(j, dl): F.direct(raw, NL, dl, j) for j, dl in ((0, TAB), (1, TAB), (3, TAB), (7, TAB), (1023, TAB), (1, ord(",")))}
        files[name] = {"raw": raw, "path": str(path), "wanted": wanted}
    with native.open(files["tail"]["path"], parallelization=0) as f:
        blocks = f.block_offsets()
    assert len(blocks) >= 6                                     # several launch seams, and the long line crosses two
    return {"files": files, "folder": folder, "blocks": sorted(blocks.values())}


def pairs(spans):
    starts, sizes = spans
    assert starts.dtype == np.uint64 and sizes.dtype == np.int64 and len(starts) == len(sizes)
    return list(zip(starts.tolist(), sizes.tolist()))


@pytest.mark.parametrize("parallelization", [1, 2, 0])
@pytest.mark.parametrize("name", ["tail", "closed"])
def test_reader_whole_file_and_windows(native, corpus, name, parallelization):
    entry = corpus["files"][name]
    raw, wanted = entry["raw"], entry["wanted"]
    n = len(F.lines_of(raw, NL))
    assert n == raw.count(b"\n") + (name == "tail")
    with native.open(entry["path"], parallelization=parallelization) as f:
        for (j, dl), want in wanted.items():
            got = pairs(f.field_spans(j, delimiter=bytes([dl])))
            assert got == want, (j, dl)
            if j == 1:
                fields = F.fields_of(raw, NL, dl, j)
                assert [raw[s:s + size] if size >= 0 else None for s, size in got] == fields
                assert f.read_fields(j, delimiter=bytes([dl])) == fields
        starts = f.field_spans(0)[0]
        assert starts.tolist() == f.line_starts(range(n)).tolist()
        # windows: inside one block, across blocks, around block seams, at and past the end, and empty ones
        starts = starts.tolist()
        seam_lines = [max(k for k in range(n) if starts[k] <= b) for b in corpus["blocks"][1:-1]]
        windows = [(0, 1), (0, 3), (5, 7), (seam_lines[0], 1), (seam_lines[0] - 1, 3), (seam_lines[1] + 1, 1),
                   (seam_lines[0], seam_lines[3] - seam_lines[0] + 2), (n - 1, 1), (n - 1, 5), (n - 3, 3), (n - 2, 10**12),
                   (n, 1), (n + 5, 2), (7, 0), (0, 0), (1, None), (n // 2, None)]
        want, fields = wanted[(3, TAB)], F.fields_of(raw, NL, TAB, 3)
        for first, count in windows:
            end = n if count is None else first + count
            assert pairs(f.field_spans(3, first, count)) == want[first:end], (first, count)
        for first, count in windows[3:7] + windows[8:13]:
            assert f.read_fields(3, first, count) == fields[first:first + count], (first, count)
        assert pairs(f.field_spans(1, seam_lines[1], 4, delimiter=b",")) == wanted[(1, ord(","))][seam_lines[1]:seam_lines[1] + 4]
        assert f.tell() == 0                                        # positionless
    with native.IndexedBzip2File(entry["path"], parallelization=parallelization) as f:
        assert pairs(f.field_spans(1, 3, 2)) == wanted[(1, TAB)][3:5]
        assert f.read_fields(0, 3, 2) == F.fields_of(raw, NL, TAB, 0)[3:5]


def small_file(folder, name, raw, level=9):
    path = folder / name
    path.write_bytes(datagen.compress(raw, level))
    return str(path)


def test_small_files_and_the_fixtures(native, corpus):
    folder = corpus["folder"]
    cases = [("small-empty.bz2", b""), ("small-newline.bz2", b"\n"), ("small-closed.bz2", b"a\tb\n\n"),
             ("small-tail.bz2", b"a\tb\nc\td\te\nf\t"), ("small-tabs.bz2", b"\t\t\n\t"), ("small-nul.bz2", b"\0\t\0\n\0\0\n\0")]
    for name, raw in cases:
        with native.open(small_file(folder, name, raw), parallelization=1) as f:
            for j in (0, 1, 2, 3):
                assert pairs(f.field_spans(j)) == F.direct(raw, NL, TAB, j), (name, j)
                assert f.read_fields(j) == F.fields_of(raw, NL, TAB, j), (name, j)
                assert pairs(f.field_spans(j, 1)) == F.direct(raw, NL, TAB, j)[1:], (name, j)
            assert pairs(f.field_spans(0, newline=b"\0", delimiter=b"\n")) == F.direct(raw, 0, NL, 0), name
    assert F.direct(b"a\tb\n\n", NL, TAB, 1) == [(2, 1), (4, -1)] and F.fields_of(b"f\t", NL, TAB, 1) == [b""]
    for name in fixture_names():
        enc, raw = read_fixture(name)
        with native.open(os.path.join(FIXTURES, name + ".bz2"), parallelization=0) as f:
            for j, dl in ((0, ord(" ")), (2, ord(" ")), (1, TAB)):
                assert pairs(f.field_spans(j, delimiter=bytes([dl]))) == F.direct(raw, NL, dl, j), (name, j, dl)
            assert f.read_fields(2, 0, 50, delimiter=b" ") == F.fields_of(raw, NL, ord(" "), 2)[:50], name


def test_interleaved_with_other_calls(native, corpus):
    entry = corpus["files"]["tail"]
    raw = entry["raw"]
    with native.open(entry["path"], parallelization=0) as f:
        head = f.read(1000)
        assert head == raw[:1000] and f.tell() == 1000
        hashes = f.line_hashes(0, 500)
        numbers, lines = f.grep(b"abc", limit=20)
        assert pairs(f.field_spans(1, 10, 300)) == entry["wanted"][(1, TAB)][10:310]
        assert f.read_fields(0, 100, 50) == F.fields_of(raw, NL, TAB, 0)[100:150]
        assert f.tell() == 1000
        assert f.line_hashes(0, 500).tolist() == hashes.tolist()
        again = f.grep(b"abc", limit=20)
        assert again[0].tolist() == numbers.tolist() and again[1] == lines
        assert f.read(500) == raw[1000:1500] and f.tell() == 1500
        assert pairs(f.field_spans(7)) == entry["wanted"][(7, TAB)]
        assert f.read(100) == raw[1500:1600]


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import numpy as np
import indexed_bzip2_amd as m

with m.open(sys.argv[2], parallelization=int(sys.argv[3])) as f:
    for field, first, count, delimiter in ((0, 0, None, b"\t"), (1, 0, None, b"\t"), (3, 100, 2000, b"\t"), (1, 0, None, b","),
                                           (1023, 0, None, b"\t"), (2, 10**9, 5, b"\t"), (2, 3, 0, b"\t")):
        starts, sizes = f.field_spans(field, first, count, delimiter)
        got = f.field_spans_to_tensor(field, first, count, delimiter)
        for tensor, host in zip(got, (starts, sizes)):
            assert tensor.dtype == torch.int64 and tensor.is_cuda and tensor.dim() == 1
            assert tensor.cpu().numpy().tolist() == host.tolist(), (field, first, count)
        fields = f.read_fields(field, first, count, delimiter)
        data, offsets = f.read_fields_to_tensor(field, first, count, delimiter)
        assert data.dtype == torch.uint8 and data.is_cuda and offsets.dtype == torch.int64 and not offsets.is_cuda
        assert len(offsets) == len(fields) + 1 and int(offsets[0]) == 0 and int(offsets[-1]) == data.numel()
        blob, bounds = bytes(data.cpu().numpy()), offsets.tolist()
        assert [blob[a:b] for a, b in zip(bounds, bounds[1:])] == [x or b"" for x in fields], (field, first, count)
        assert [b - a for a, b in zip(bounds, bounds[1:])] == [max(int(n), 0) for n in sizes]
        print(field, first, count, len(fields))
    assert f.tell() == 0
print("field tensors ok")
"""


@pytest.mark.parametrize("parallelization", [1, 0])
def test_tensor_forms_equal_the_host_forms(native, corpus, parallelization):
    """In a process of its own that imports torch first; the host forms are pinned to the model above."""
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, corpus["files"]["tail"]["path"], str(parallelization)],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "field tensors ok" in run.stdout and "0 0 None 0" not in run.stdout


def test_tool(native, corpus):
    for name, options, j, dl in (("tail", ["--cut-field", "1"], 1, TAB), ("closed", ["--cut-field=3", "-P", "1"], 3, TAB),
                                 ("tail", ["--cut-field", "1", "--field-delimiter", ","], 1, ord(",")),
                                 ("closed", ["--cut-field", "0", "--field-delimiter=\\x09"], 0, TAB)):
        entry = corpus["files"][name]
        run = subprocess.run([CLI] + options + [entry["path"]], capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr
        assert run.stdout == b"".join((field or b"") + b"\n" for field in F.fields_of(entry["raw"], NL, dl, j)), options
