"""Field columns on the GPU: the kernels under Decoder.gather_fields (k_fieldcol_sums, k_fieldcol_top, k_fieldcol_offsets,
k_field_gather) on one decoded text of about 200 kB, the reader's read_columns / read_columns_to_tensor and their C entry
points, the count of decoded blocks, and the tool's --cut-fields.

The reference is the plain Python model of fieldcols.py and fields.py -- slices of the text and bytes.split per line --,
never the code under test.  Totals, offsets, sizes and bytes are compared exactly, and the bytes of a destination behind
the total must be as they were before the call."""
import bisect
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, FIXTURES, fixture_names, read_fixture
import datagen
import fieldcols as FC
import fields as F

pytestmark = pytest.mark.gpu

NL, TAB = 10, 9
FILL = 0xA5
INVALID_ARGUMENT = 103                                         # MI355X_BZ2_ERR_INVALID_ARGUMENT
LINES_END = 120_000                                            # the text's lines of fields lie in front of this offset


def device_text():
    """About 200 kB: lines of tab-separated fields -- short ones, empty ones, lines with too few fields, a field longer than
    two tiles of the gather --, then noise in which no byte repeats its neighbour, so that a copy from a wrong source
    offset shows."""
    rng = random.Random(0xC01)
    out = bytearray()
    while len(out) < LINES_END - 40_000:
        fields = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789 ,\0\xff") for _ in range(rng.choice([0, 0, 1, 2, 5, 9, 20, 33, 70])))
                  for _ in range(rng.choice([0, 1, 1, 2, 3, 5, 9]))]
        out += b"\t".join(fields) + b"\n"
    long_at = len(out) + 2
    out += b"k\t" + bytes((7 * i + i // 251) % 251 + 1 if (7 * i + i // 251) % 251 + 1 not in (NL, TAB) else 0xFE for i in range(34_000)) + b"\tz\n"
    assert len(out) < LINES_END
    out += b"\n" * (LINES_END - len(out))
    out += bytes((i * 131 + i // 256 * 7) % 256 for i in range(80_000))
    out += b"tail\twithout\tnewline"
    return bytes(out), long_at


@pytest.fixture(scope="module")
def device(native):
    text, long_at = device_text()
    enc = datagen.compress(text, 9)
    dec = native.Decoder(device=0)
    dec.set_input(enc)
    _, total = dec.decode_batch(native.find_magic(enc))
    assert total == len(text) and dec.copy_output(0, total) == text
    yield {"dec": dec, "text": text, "long_at": long_at, "tile": native._native.gather_fields_tile_bytes()}
    dec.close()


def check(device, starts, sizes, base=0, extra=64, **how):
    """Decoder.gather_fields against the model, exactly; `extra` bytes of room behind the total must stay as they were."""
    total, offsets, data = FC.gathered(device["text"], starts, sizes, base)
    got_total, got_offsets, got = device["dec"].gather_fields(starts, sizes, base, room=total + extra, capacity=total + extra // 2,
                                                              fill=FILL, **how)
    assert got_total == total
    assert got_offsets.dtype == np.uint64 and got_offsets.tolist() == offsets
    assert got.dtype == np.uint8 and got.size == total + extra
    assert got[:total].tobytes() == data, first_difference(got[:total].tobytes(), data)
    assert (got[total:] == FILL).all(), "written behind the total"
    return offsets


def first_difference(got, want):
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "first difference at byte %d of %d" % (at, len(want))


def test_tile_size(native, device):
    assert device["tile"] == native.lib().mi355x_bz2_gather_fields_tile_bytes() == 16384


def test_every_source_and_destination_alignment(device):
    """Source starts at all 16 alignments crossed with sizes 0 to 33: packed back to back, the fields begin at every
    destination alignment, whatever the destination's own."""
    pairs = [(a, size) for a in range(16) for size in range(34)]
    random.Random(1).shuffle(pairs)
    starts = [LINES_END + 1024 + 64 * k + a for k, (a, _) in enumerate(pairs)]
    sizes = [size for _, size in pairs]
    assert {(s % 16, n) for s, n in zip(starts, sizes)} == {(a, n) for a in range(16) for n in range(34)}
    for misalign in (0, 1, 7, 15):
        offsets = check(device, starts, sizes, misalign=misalign)
        seen = {((o + misalign) % 16, s % 16) for o, s, n in zip(offsets, starts, sizes) if n > 0}
        assert {d for d, _ in seen} == set(range(16)) and len(seen) > 200
    # sizes 16 to 33 from every source alignment to every destination alignment: the vectors inside one span
    for lead in range(16):
        check(device, [LINES_END + 5] + starts, [lead] + [max(n, 16) for n in sizes], misalign=3)


def test_tile_edges_and_long_fields(device):
    tile = device["tile"]
    src = LINES_END + 13
    for misalign in (0, 3):
        edge = tile - misalign                                     # the packed byte at which the second workgroup begins
        for d in (-1, 0, 1):
            # a field that ends 1 byte before, at and 1 byte behind the edge; then small ones, then the same at the next edge
            sizes = [edge + d, 1, 2, 33, tile - 36 - d - 1 + d, 5, 0, -1, 9]
            starts = [src, 3, 70_001, src + 4, 11, LINES_END + 7, 0, 0, 50]
            offsets = check(device, starts, sizes, misalign=misalign)
            assert offsets[1] == edge + d and offsets[5] == edge + tile + d - 1
        # many small fields across three edges and more: 11.8 bytes each on average
        rng = random.Random(misalign)
        sizes = [rng.choice([0, -1, 1, 2, 3, 15, 16, 17, 31, 33]) for _ in range(6000)]
        starts = [rng.randrange(0, len(device["text"]) - 40) for _ in sizes]
        assert check(device, starts, sizes, misalign=misalign)[-1] > 3 * tile
    # one field longer than two tiles, from an odd source offset, alone and between others; and all of the output
    long_size = 2 * tile + 4321
    check(device, [src], [long_size])
    check(device, [5, src + 2, 9], [3, long_size, 40], misalign=9)
    check(device, [0], [len(device["text"])])
    # the 34 000-byte field of the text's own lines
    text = device["text"]
    at = device["long_at"]
    assert text[at - 3:at] == b"\nk\t" and text[at + 34_000] == TAB
    check(device, [at], [34_000], misalign=1)


def test_a_search_not_a_walk(device):
    """One byte, 100 000 empty and missing fields, one byte."""
    sizes = [1] + [0, -1] * 50_000 + [1]
    starts = [LINES_END + 3] + [2**64 - 1, 0] * 50_000 + [LINES_END + 9]
    offsets = check(device, starts, sizes)
    assert offsets[-1] == 2 and offsets[1] == offsets[100_001] == 1
    # the same between two fields that fill their vectors, and at a tile's edge
    tile = device["tile"]
    check(device, [7] + [0] * 100_000 + [11], [tile - 1] + [-1, 0] * 50_000 + [40])
    check(device, [7] + [0] * 100_000 + [11, 13], [tile] + [0] * 100_000 + [1, 16], misalign=15)


def test_any_order_overlaps_and_the_last_byte(device):
    end = len(device["text"])
    starts = list(range(end - 40, LINES_END, -997))                # descending
    check(device, starts, [37] * len(starts))
    check(device, [LINES_END + 100] * 50 + [LINES_END + 90 + k for k in range(50)], [64] * 50 + [k for k in range(50)])   # overlapping
    check(device, [end - 1], [1])                                  # a span that ends at the output's last byte
    check(device, [end - 16, end - 33, end - 1, end], [16, 33, 1, 0], misalign=2)
    check(device, [3, end - 4099], [2, 4099])


def test_few_spans_no_bytes_no_destination(device):
    dec = device["dec"]
    for starts, sizes in (([], []), ([5], [3]), ([5], [0]), ([5], [-1]), ([2**64 - 1] * 3000, [-1] * 3000), ([0, 1, 2], [0, -1, 0])):
        check(device, starts, sizes)
        total, offsets, data = dec.gather_fields(starts, sizes, dst=False)
        assert data is None and (total, offsets.tolist()) == FC.gathered(device["text"], starts, sizes)[:2]
    # no destination: the total and the offsets come first
    starts, sizes = [LINES_END + 15 * k for k in range(5000)], [k % 23 - 1 for k in range(5000)]
    total, offsets, data = dec.gather_fields(starts, sizes, dst=False)
    assert data is None and (total, offsets.tolist()) == FC.gathered(device["text"], starts, sizes)[:2]


def test_capacity_one_byte_short(device):
    starts, sizes = [LINES_END + 15 * k for k in range(5000)], [k % 23 - 1 for k in range(5000)]
    want_total, want_offsets, want = FC.gathered(device["text"], starts, sizes)
    total, offsets, data = device["dec"].gather_fields(starts, sizes, room=want_total + 8, capacity=want_total - 1, fill=FILL)
    assert total == want_total and offsets.tolist() == want_offsets
    assert (data == FILL).all(), "a destination that is too small was written"
    total, offsets, data = device["dec"].gather_fields(starts, sizes, room=want_total + 8, capacity=want_total, fill=FILL)
    assert total == want_total and data[:total].tobytes() == want and (data[total:] == FILL).all()


def test_base_beyond_32_bits(device):
    base = 2**32 + 5
    rng = random.Random(32)
    sizes = [rng.choice([-1, 0, 1, 7, 16, 40, 300]) for _ in range(3000)]
    starts = [base + rng.randrange(0, len(device["text"]) - 300) for _ in sizes]
    check(device, starts, sizes, base=base)
    check(device, [base, base + len(device["text"]) - 1], [1, 1], base=base)


def test_spans_outside_the_output(native, device):
    """One byte outside at either end: refused by the GPU's check, and no byte of the destination is written."""
    end = len(device["text"])
    good = ([LINES_END + 40 * k for k in range(300)], [k % 34 for k in range(300)])
    for base, start, size in ((7, 6, 3), (0, end - 2, 3), (0, end, 1), (0, end + 1, 1), (2**32 + 5, 2**32 + 4, 1), (2**32 + 5, 3, 1),
                              (0, 5, end), (0, 0, end + 1), (0, 1, 2**62), (0, 2**64 - 1, 2), (0, 2**63, 2**63 - 1)):
        for at in (0, 123, 299):
            starts = [base + s for s in good[0]]
            sizes = list(good[1])
            starts[at], sizes[at] = start, size
            starts[200] = starts[at] if at < 200 else starts[200]         # a second offender behind the first
            sizes[200] = sizes[at] if at < 200 else sizes[200]
            with pytest.raises(native.Bz2Error) as refused:
                device["dec"].gather_fields(starts, sizes, base, room=20_000, fill=FILL)
            assert refused.value.status == INVALID_ARGUMENT
            assert "gather_fields: span %d lies outside the last batch's output" % at in str(refused.value), (base, start, size)
            assert (refused.value.destination == FILL).all(), "a refused call wrote to its destination"
    # a span without bytes may have any start; the decoder still serves
    check(device, [2**64 - 1, end + 5, 3], [0, -1, 2])
    with pytest.raises(native.Bz2Error) as refused:
        device["dec"].gather_fields([0, 0, end], [1, 1, 1])
    assert "span 2 " in str(refused.value) and "(1 of the spans do)" in str(refused.value)


def test_the_fields_that_field_spans_found(device):
    """field_spans' two arrays straight into gather_fields: the column of the model, for several fields and delimiters."""
    text, dec = device["text"], device["dec"]
    for field, dl, span in ((0, TAB, (0, len(text))), (1, TAB, (0, len(text))), (3, TAB, (0, LINES_END)), (1023, TAB, (0, LINES_END)),
                            (1, ord(","), (0, LINES_END)), (2, TAB, (1000, 50_000))):
        part = text[span[0]:span[0] + span[1]]
        closed = part.count(b"\n")
        _, starts, sizes = dec.field_spans([span], field, bytes([dl]))
        assert len(starts) == closed
        want, want_offsets, want_sizes = FC.column(part[:part.rindex(b"\n") + 1], NL, dl, field)
        assert sizes.tolist() == want_sizes
        total, offsets, data = dec.gather_fields(starts, sizes, room=len(want) + 16, fill=FILL)
        assert total == len(want) and offsets.tolist() == want_offsets
        assert data[:total].tobytes() == want and (data[total:] == FILL).all()
    assert len(FC.column(text[:LINES_END], NL, TAB, 1)[0]) > 10_000


# ------------------------------------------------------------------------------------------------ the reader

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
FIELDS = [0, 3, 7, 1023, 3]
LONG_TABS = (5, 90_000, 90_001, 230_000)


def reader_text(tail=True):
    """About 700 kB of records, shaped like test_gpu_fields.py's corpus: tab-separated lines of 0 to 12 fields, some with
    commas, runs of empty lines, one line of 250 kB -- longer than two 100 kB blocks, so its fields cross two launch seams
    -- with its tabs far apart, and an unterminated tail or none.  Returns (text, the number of the long line)."""
    rng = random.Random(0xC015)
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
    long_number = out.count(b"\n")
    long_line = bytearray(rng.choice(b"abcdefgh \0\xff") for _ in range(250_000))
    for k in LONG_TABS:
        long_line[k] = TAB
    out.extend(long_line + b"\n")
    records(150_000)
    return bytes(out) + (b"the\ttail has\tno newline" if tail else b""), long_number


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("fieldcols")
    files = {}
    for name, (raw, long_number) in (("tail", reader_text(True)), ("closed", reader_text(False))):
        path = folder / (name + ".bz2")
        path.write_bytes(datagen.compress(raw, 1))
        # computed once, shared, left unchanged
        wanted = {(j, dl): F.fields_of(raw, NL, dl, j) for j, dl in ((0, TAB), (3, TAB), (7, TAB), (1023, TAB), (1, ord(",")), (1, TAB))}
        starts = [0]
        for line in raw.split(b"\n")[:-1]:
            starts.append(starts[-1] + len(line) + 1)
        files[name] = {"raw": raw, "path": str(path), "wanted": wanted, "long": long_number, "starts": starts}
    with native.open(files["tail"]["path"], parallelization=0) as f:
        blocks = sorted(f.block_offsets().values())
    assert len(blocks) >= 6                                     # several launch seams, and the long line crosses two
    long_at = files["tail"]["starts"][files["tail"]["long"]]
    assert sum(1 for b in blocks if long_at < b < long_at + 250_000) >= 2
    return {"files": files, "folder": folder, "blocks": blocks}


@pytest.mark.parametrize("parallelization", [1, 2, 0])
@pytest.mark.parametrize("name", ["tail", "closed"])
def test_reader_whole_file_and_windows(native, corpus, name, parallelization):
    entry = corpus["files"][name]
    raw, wanted, starts = entry["raw"], entry["wanted"], entry["starts"]
    n = len(F.lines_of(raw, NL))
    assert n == raw.count(b"\n") + (name == "tail")
    with native.open(entry["path"], parallelization=parallelization) as f:
        got = f.read_columns(FIELDS)
        assert len(got) == len(FIELDS)
        for j, column in zip(FIELDS, got):
            assert column == wanted[(j, TAB)], (j, first_unequal(column, wanted[(j, TAB)]))
        # the 250 kB line, whose fields cross two seams
        long_fields = [len(column[entry["long"]]) for column in f.read_columns([0, 1, 2, 3, 4])]
        assert long_fields == [5, 89_994, 0, 139_998, 19_999]
        assert f.read_columns([1], delimiter=b",") == [wanted[(1, ord(","))]]
        # windows: inside one block, across blocks, around block seams, at and past the end, and empty ones
        seam_lines = [bisect.bisect_right(starts, b) - 1 for b in corpus["blocks"][1:-1]]
        windows = [(0, 1), (0, 3), (5, 7), (seam_lines[0], 1), (seam_lines[0] - 1, 3), (seam_lines[1] + 1, 1),
                   (seam_lines[0], seam_lines[3] - seam_lines[0] + 2), (n - 1, 1), (n - 1, 5), (n - 3, 3), (n - 2, 10**12),
                   (n, 1), (n + 5, 2), (7, 0), (0, 0), (1, None), (n // 2, None)]
        for first, count in windows:
            end = n if count is None else first + count
            got = f.read_columns(FIELDS, first, count)
            assert got == [wanted[(j, TAB)][first:end] for j in FIELDS], (first, count)
            assert f.read_columns([1], first, count, delimiter=b",") == [wanted[(1, ord(","))][first:end]], (first, count)
        assert f.tell() == 0                                        # positionless
        assert f.read_columns([1], 3, 40) == [f.read_fields(1, 3, 40)]
    with native.IndexedBzip2File(entry["path"], parallelization=parallelization) as f:
        assert f.read_columns([1, 0], 3, 2) == [wanted[(1, TAB)][3:5], wanted[(0, TAB)][3:5]]


def first_unequal(got, want):
    return next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), (len(got), len(want)))


def test_small_files_and_the_fixtures(native, corpus):
    folder = corpus["folder"]
    cases = [("small-empty.bz2", b""), ("small-newline.bz2", b"\n"), ("small-closed.bz2", b"a\tb\n\n"),
             ("small-tail.bz2", b"a\tb\nc\td\te\nf\t"), ("small-tabs.bz2", b"\t\t\n\t"), ("small-nul.bz2", b"\0\t\0\n\0\0\n\0")]
    for name, raw in cases:
        path = folder / name
        path.write_bytes(datagen.compress(raw, 9))
        with native.open(str(path), parallelization=1) as f:
            assert f.read_columns([0, 1, 2, 3]) == [F.fields_of(raw, NL, TAB, j) for j in (0, 1, 2, 3)], name
            assert f.read_columns([2, 0], 1) == [F.fields_of(raw, NL, TAB, j)[1:] for j in (2, 0)], name
            assert f.read_columns([0], newline=b"\0", delimiter=b"\n") == [F.fields_of(raw, 0, NL, 0)], name
    for name in fixture_names():
        enc, raw = read_fixture(name)
        with native.open(os.path.join(FIXTURES, name + ".bz2"), parallelization=0) as f:
            assert f.read_columns([0, 2], delimiter=b" ") == [F.fields_of(raw, NL, ord(" "), j) for j in (0, 2)], name
            assert f.read_columns([1]) == [F.fields_of(raw, NL, TAB, 1)], name


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import indexed_bzip2_amd as m

with m.open(sys.argv[2], parallelization=int(sys.argv[3])) as f:
    for fields, first, count, delimiter in (([0, 3, 7, 1023, 3], 0, None, b"\t"), ([1], 0, None, b","), ([3, 1], 100, 2000, b"\t"),
                                            ([2], 10**9, 5, b"\t"), ([2, 2], 3, 0, b"\t")):
        host = f.read_columns(fields, first, count, delimiter)
        got = f.read_columns_to_tensor(fields, first, count, delimiter)
        assert len(got) == len(host) == len(fields)
        for (data, offsets, sizes), column in zip(got, host):
            assert data.dtype == torch.uint8 and offsets.dtype == torch.int64 and sizes.dtype == torch.int64
            assert data.is_cuda and offsets.is_cuda and sizes.is_cuda and data.dim() == offsets.dim() == sizes.dim() == 1
            assert len(sizes) == len(column) and len(offsets) == len(column) + 1
            bounds, blob = offsets.cpu().tolist(), bytes(data.cpu().numpy())
            assert bounds[0] == 0 and bounds[-1] == data.numel()
            assert sizes.cpu().tolist() == [-1 if x is None else len(x) for x in column], (fields, first, count)
            assert [blob[a:b] for a, b in zip(bounds, bounds[1:])] == [x or b"" for x in column], (fields, first, count)
        print(fields, first, count, len(host[0]))
    assert f.tell() == 0
print("column tensors ok")
"""


@pytest.mark.parametrize("parallelization", [1, 0])
def test_tensor_forms_equal_the_host_forms(native, corpus, parallelization):
    """In a process of its own that imports torch first; the host forms are pinned to the model above."""
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, corpus["files"]["tail"]["path"], str(parallelization)],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "column tensors ok" in run.stdout and "[0, 3, 7, 1023, 3] 0 None 0" not in run.stdout


def test_interleaved_with_other_calls_and_the_hold_rules(native, corpus):
    entry = corpus["files"]["tail"]
    raw, wanted = entry["raw"], entry["wanted"]
    lib = native.lib()
    with native.open(entry["path"], parallelization=0) as f:
        handle = f._open_reader()._h
        none = [None] * 3
        assert lib.mi355x_bz2_reader_take_field_column(handle, 0, *none, 0) == INVALID_ARGUMENT          # nothing is held
        assert b"no field columns are held" in lib.mi355x_bz2_reader_last_error(handle)
        assert f.read(1000) == raw[:1000] and f.tell() == 1000
        hashes = f.line_hashes(0, 500)
        numbers, lines = f.grep(b"abc", limit=20)
        spans = f.field_spans(1, 10, 300)
        assert f.read_columns([1, 0], 10, 300) == [wanted[(1, TAB)][10:310], wanted[(0, TAB)][10:310]]
        assert f.tell() == 1000
        # the field spans held before read_columns are still takeable
        starts, sizes = np.zeros(300, dtype=np.uint64), np.zeros(300, dtype=np.int64)
        assert lib.mi355x_bz2_reader_take_field_spans(handle, ctypes.c_void_p(starts.ctypes.data), ctypes.c_void_p(sizes.ctypes.data), 300, 0) == 0
        assert starts.tolist() == spans[0].tolist() and sizes.tolist() == spans[1].tolist()
        assert f.line_hashes(0, 500).tolist() == hashes.tolist()
        again = f.grep(b"abc", limit=20)
        assert again[0].tolist() == numbers.tolist() and again[1] == lines
        assert f.read(500) == raw[1000:1500] and f.tell() == 1500
        # the columns are held until the next call of their own: taken twice, in any order, with and without the bytes
        n, totals = ctypes.c_uint64(), (ctypes.c_uint64 * 2)()
        numbers = (ctypes.c_uint32 * 2)(3, 0)
        assert lib.mi355x_bz2_reader_field_columns(handle, NL, TAB, numbers, 2, 20, 100, 1, ctypes.byref(n), totals) == 0
        want = [wanted[(3, TAB)][20:120], wanted[(0, TAB)][20:120]]
        assert n.value == 100 and list(totals) == [sum(len(x or b"") for x in column) for column in want]
        f.grep(b"abc", limit=5)
        f.field_spans(0, 0, 5)
        for column in (1, 0, 1):
            data = np.full(totals[column] + 8, FILL, dtype=np.uint8)
            offsets, sizes = np.zeros(101, dtype=np.uint64), np.zeros(100, dtype=np.int64)
            assert lib.mi355x_bz2_reader_take_field_column(handle, column, None, ctypes.c_void_p(offsets.ctypes.data),
                                                           ctypes.c_void_p(sizes.ctypes.data), 0) == 0
            assert sizes.tolist() == [-1 if x is None else len(x) for x in want[column]]
            assert offsets[-1] == totals[column] and offsets[0] == 0
            assert lib.mi355x_bz2_reader_take_field_column(handle, column, ctypes.c_void_p(data.ctypes.data), None, None, 0) == 0
            blob, bounds = data.tobytes(), offsets.tolist()
            assert [blob[a:b] for a, b in zip(bounds, bounds[1:])] == [x or b"" for x in want[column]]
            assert (data[totals[column]:] == FILL).all()
        assert lib.mi355x_bz2_reader_take_field_column(handle, 2, *none, 0) == INVALID_ARGUMENT          # two columns are held
        # the next call replaces them; a call over no lines holds columns without lines
        assert lib.mi355x_bz2_reader_field_columns(handle, NL, TAB, numbers, 1, 10**9, 5, 1, ctypes.byref(n), totals) == 0
        assert n.value == 0 and totals[0] == 0
        offsets = np.full(1, 7, dtype=np.uint64)
        assert lib.mi355x_bz2_reader_take_field_column(handle, 0, None, ctypes.c_void_p(offsets.ctypes.data), None, 0) == 0 and offsets[0] == 0
        assert lib.mi355x_bz2_reader_take_field_column(handle, 1, *none, 0) == INVALID_ARGUMENT
        assert f.tell() == 1500


def test_tool(native, corpus):
    for name, options, fields, dl in (("tail", ["--cut-fields", "0,3,5"], (0, 3, 5), TAB), ("closed", ["--cut-fields=3", "-P", "1"], (3,), TAB),
                                      ("tail", ["--cut-fields", "1,0,1", "--field-delimiter", ","], (1, 0, 1), ord(",")),
                                      ("closed", ["--cut-fields", "7,1023", "--field-delimiter=\\x09", "-P", "2"], (7, 1023), TAB)):
        entry = corpus["files"][name]
        run = subprocess.run([CLI] + options + [entry["path"]], capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr
        columns = [F.fields_of(entry["raw"], NL, dl, j) for j in fields]
        assert run.stdout == b"".join(bytes([dl]).join(x or b"" for x in row) + b"\n" for row in zip(*columns)), options


def blocks_decoded(f, call):
    before = f.statistics()
    call()
    after = f.statistics()
    return after["blocks_decoded"] - before["blocks_decoded"], after["batches"] - before["batches"]


def test_every_block_is_decoded_once(native, corpus):
    """With the line index built first: three columns cost the decodes of field_spans for one field -- and, where lines
    cross launch seams, at most one more of the blocks that hold a byte of such a line.  On the corpus without a tail: an
    unterminated tail is fetched as the seam lines are, which decodes its block a second time."""
    entry = corpus["files"]["closed"]
    raw, starts, blocks = entry["raw"], entry["starts"], None
    with native.open(entry["path"], parallelization=0) as f:
        blocks = sorted(f.block_offsets().values())
        data_blocks = [b for b in blocks if b < len(raw)]
        f.count_lines()
        # a window inside one block, behind the block's first line
        inside = bisect.bisect_right(starts, blocks[2]) + 2
        assert starts[inside + 20] < blocks[3]
        spans = blocks_decoded(f, lambda: f.field_spans(3, inside, 20))
        columns = blocks_decoded(f, lambda: f.read_columns([0, 3, 7], inside, 20))
        print("one block:", spans, columns)
        assert columns[0] == spans[0] == 1
        # the whole file in one launch
        spans = blocks_decoded(f, lambda: f.field_spans(3))
        columns = blocks_decoded(f, lambda: f.read_columns([0, 3, 7]))
        print("whole file, parallelization 0:", spans, columns)
        assert spans[1] == 1 and columns[1] == 1
        assert columns[0] == spans[0] == len(data_blocks)
    # the distinct blocks that hold a byte of a line crossing a block boundary, from the block map and the raw text
    crossing = set()
    for boundary in data_blocks[1:]:
        if raw[boundary - 1:boundary] != b"\n":
            begin = raw.rfind(b"\n", 0, boundary) + 1
            end = raw.find(b"\n", boundary)
            end = len(raw) if end < 0 else end
            crossing.update(range(bisect.bisect_right(data_blocks, begin) - 1, bisect.bisect_right(data_blocks, max(begin, end - 1))))
    assert 2 <= len(crossing) <= len(data_blocks)
    with native.open(entry["path"], parallelization=2) as f:
        f.count_lines()
        spans = blocks_decoded(f, lambda: f.field_spans(3))
        columns = blocks_decoded(f, lambda: f.read_columns([0, 3, 7]))
        print("whole file, parallelization 2:", spans, columns, "crossing blocks:", len(crossing))
        assert spans[0] == len(data_blocks) and spans[1] > 1
        assert spans[0] <= columns[0] <= spans[0] + len(crossing)
