"""line_hashes on the GPU: the kernels under Decoder.hash_lines (k_linehash_chunks, k_linehash_link, k_linehash_emit),
the reader's line_hashes / line_hashes_to_tensor / count_distinct_lines / first_occurrences, and the tool's
--line-hashes and --count-distinct-lines.

The reference is the plain Python model of linehash.py -- the definition h = (h * x + b + 1) mod (2^61 - 1) in Python's
integers, over prefix sums so that a text is paid for once -- and for the distinct lines a Python dict over the contents;
never the code under test.  Hashes are compared exactly."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import datagen
import linehash as H

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
NL = 10
ONES = 2**64 - 1
SIZES = (0, 1, 255, 256, 257, 65_535, 65_536, 65_537, 131_073)
EDGES = (255, 256, 257, 511, 512, 65_535, 65_536)


# ------------------------------------------------------------------------------------------------ the kernels

def device_text():
    """(text, {name: (offset, size)})."""
    rng = random.Random(0x11E5)
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
            out += bytes(rng.choice(b"aab,xyz \0\xff") for _ in range(rng.choice([0, 0, 1, 3, 8, 20, 60, 300]))) + b"\n"
        return bytes(out[:n - 1]) + b"\n"

    def noise(n):
        return bytes(rng.choice(b"abcdefgh\0\xff ") for _ in range(n))

    add(filler(max(SIZES) + 40), "lines")
    # delimiters at the edges of chunks and of a tile, counted from the region's start, and nowhere else
    add(noise(-at % 16))                                            # the region starts at a 16-byte boundary
    edges = bytearray(noise(EDGES[-1] + 600))
    for k in EDGES:
        edges[k] = NL
    add(bytes(edges) + b"\n", "edges")
    add(b"\n" * 700, "empty-lines")
    add(noise(3 * 256 + 9), "no-delimiter")
    add(b"\n")
    add(noise(300) + b"\n" + noise(500), "one-delimiter")
    add(b"\n")
    add(noise(70_000), "line-70000")
    add(b"\n")
    add(noise(200_000), "line-200000")
    add(b"\n")
    add(b"".join(b"\0" * n + b"\n" for n in range(1, 301)), "zeros")
    add(b"".join(b"\xff" * n + b"\n" for n in range(1, 301)), "ones")
    add(filler(1000))
    return b"".join(parts), where


@pytest.fixture(scope="module")
def device(native):
    text, where = device_text()
    enc = datagen.compress(text, 9)
    dec = native.Decoder(device=0)
    dec.set_input(enc)
    offsets = native.find_magic(enc)
    results, total = dec.decode_batch(offsets)
    assert total == len(text) and dec.copy_output(0, total) == text
    prefixes = {seed: H.Prefix(text, H.base(seed)) for seed in (0, 1)}           # computed once, shared, left unchanged
    yield {"dec": dec, "text": text, "where": where, "prefixes": prefixes}
    dec.close()


def check_spans(device, spans, seed=0, nl=NL, capacity=None, room=None):
    """Summaries, counts and hashes of Decoder.hash_lines against the model, exactly; returns the model's hashes."""
    if nl == NL:
        models = [device["prefixes"][seed].summary(o, n, nl) for o, n in spans]
    else:
        models = [H.summarise_chunk(device["text"][o:o + n], nl, H.base(seed)) for o, n in spans]
    summaries, hashes = device["dec"].hash_lines(spans, bytes([nl]), seed, capacity, room)
    for span, model, got in zip(spans, models, summaries):
        assert got["count"] == len(model["hashes"]), span
        assert got["has_delimiter"] == model["has_delimiter"] and got["tail_non_empty"] == model["tail_non_empty"], span
        assert got["head"] == model["head"] and got["tail"] == model["tail"], span
    wanted = [h for model in models for h in model["hashes"]]
    written = len(wanted) if capacity is None else min(capacity, len(wanted))
    assert hashes[:written].tolist() == wanted[:written], spans[:3]
    assert (hashes[written:] == ONES).all(), "written at or beyond the capacity"
    return wanted


def test_span_sizes_at_every_alignment(native, device):
    assert native._native.line_hash_chunk_bytes() == 256
    base = device["where"]["lines"][0]
    base += -base % 16                                              # the output buffer is 16-byte aligned
    spans = [(base + start, size) for start in range(16) for size in SIZES]
    assert {o % 16 for o, _ in spans} == set(range(16))
    wanted = check_spans(device, spans)
    assert len(wanted) > 10_000
    check_spans(device, spans[::7], seed=1)
    # another delimiter: ',' ends the lines and "\n" is a byte like any other
    check_spans(device, [(base + 3, 257), (base + 5, 4099)], nl=ord(","))
    # the whole output as one span, and the same span twice
    whole = (0, len(device["text"]))
    check_spans(device, [whole, spans[20], whole])


def test_delimiters_on_chunk_and_tile_edges(device):
    offset, size = device["where"]["edges"]
    text = device["text"]
    assert offset % 16 == 0 and all(text[offset + k] == NL for k in EDGES)
    assert text.count(b"\n", offset, offset + size) == len(EDGES) + 1
    # the delimiters at exactly these offsets of a span, and one and two bytes in front of them
    check_spans(device, [(offset + shift, size - shift) for shift in (0, 1, 2)])
    check_spans(device, [(offset, size)], seed=1)
    # a delimiter as a span's first byte, as its last byte, and as all of it
    for k in EDGES:
        check_spans(device, [(offset + k, 300), (offset + k - 299, 300), (offset + k, 1), (offset + k, EDGES[-1] + 300 - k)])


def test_empty_lines_and_few_delimiters(device):
    where = device["where"]
    offset, size = where["empty-lines"]
    wanted = check_spans(device, [(offset, size), (offset + 1, 255), (offset + 3, 256), (offset + 5, 513)])
    assert wanted[:700] == [0] * 700
    none, one = where["no-delimiter"], where["one-delimiter"]
    summaries, _ = device["dec"].hash_lines([none, one])
    assert [s["has_delimiter"] for s in summaries] == [False, True] and [s["count"] for s in summaries] == [0, 1]
    assert summaries[0]["tail"] == (0, 1) and summaries[0]["tail_non_empty"]
    check_spans(device, [none, one, (none[0], none[1] + 1), (one[0] + 301, one[1] - 301)])


def test_long_lines_carry_across_tiles_and_link_steps(device):
    text, where = device["text"], device["where"]
    for name in ("line-70000", "line-200000"):
        offset, size = where[name]
        assert text[offset - 1] == NL and text[offset + size] == NL and NL not in text[offset:offset + size]
        # the line whole, closed by its delimiter; entered in its middle; and as the head of a span that goes on
        wanted = check_spans(device, [(offset, size + 1), (offset + 12_345, size + 1 - 12_345), (offset - 1, size + 300)])
        assert wanted[0] == device["prefixes"][0].part(offset, offset + size)[0]
    # many spans in one call, each its own workgroup of the link
    offset, size = where["line-200000"]
    check_spans(device, [(offset + 7 * k, 1 + k % 3) for k in range(600)])


def test_lines_of_one_byte_value(device):
    for name, value in (("zeros", 0), ("ones", 0xFF)):
        offset, size = device["where"][name]
        wanted = check_spans(device, [(offset, size)])
        assert len(wanted) == 300 and len(set(wanted)) == 300
        assert wanted == [H.line_hash(bytes([value]) * n) for n in range(1, 301)]
        assert check_spans(device, [(offset, size)], seed=1) != wanted


def test_capacity_smaller_than_the_count(device):
    offset, _ = device["where"]["lines"]
    spans = [(offset + 3, 70_000), (offset + 70_003, 5_000)]
    total = len(check_spans(device, spans))
    assert total > 1000
    for capacity in (0, 1, 2, 255, 256, total - 1, total):
        check_spans(device, spans, capacity=capacity, room=total + 64)
    # nothing is asked for: no span, and spans outside the output are refused
    assert device["dec"].hash_lines([])[0] == []
    with pytest.raises(Exception):
        device["dec"].hash_lines([(len(device["text"]) - 5, 6)])


# ------------------------------------------------------------------------------------------------ the reader

def reader_text():
    """About 600 kB: seeded lines over a small alphabet, with runs of empty lines, and an unterminated tail."""
    rng = random.Random(0x5EED)
    out = bytearray()
    while len(out) < 600_000:
        kind = rng.randrange(10)
        if kind == 0:
            out += b"\n" * rng.randrange(1, 4)
        elif kind == 1:
            out += bytes(rng.choice(b"ab\0\xff,") for _ in range(rng.randrange(1, 600))) + b"\n"
        else:
            out += b"line %d of the corpus, %s\n" % (len(out), bytes(rng.choice(b"abcdefghij") for _ in range(rng.randrange(40))))
    return bytes(out) + b"the tail has no delimiter"


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("linehash")
    raw = reader_text()
    path = folder / "text.bz2"
    path.write_bytes(datagen.compress(raw, 1))
    with native.open(str(path), parallelization=0) as f:
        blocks = f.block_offsets()
    assert len(blocks) >= 5                                     # at least four data blocks: several launch seams
    wanted = {(seed, NL): H.Prefix(raw, H.base(seed)).lines(NL) for seed in (0, 1)}
    wanted[(0, ord(","))] = H.Prefix(raw, H.base(0)).lines(ord(","))
    return {"raw": raw, "path": str(path), "folder": folder, "wanted": wanted, "blocks": sorted(blocks.values())}


@pytest.mark.parametrize("parallelization", [1, 0])
def test_reader_whole_file_and_ranges(native, corpus, parallelization):
    raw, wanted = corpus["raw"], corpus["wanted"][(0, NL)]
    n = len(wanted)
    assert n == raw.count(b"\n") + 1 == len(H.lines_of(raw, NL))            # the lines grep would number
    with native.open(corpus["path"], parallelization=parallelization) as f:
        got = f.line_hashes()
        assert got.dtype == np.uint64 and len(got) == n and got.tolist() == wanted
        assert f.line_hashes(seed=1).tolist() == corpus["wanted"][(1, NL)]
        assert f.line_hashes(newline=b",").tolist() == corpus["wanted"][(0, ord(","))]
        # ranges: inside one block, across blocks, around block seams, at and past the end, and empty ones
        starts = f.line_starts(range(n)).tolist()
        seam_lines = [max(k for k in range(n) if starts[k] <= b) for b in corpus["blocks"][1:-1]]
        ranges = [(0, 1), (0, 3), (5, 7), (seam_lines[0], 1), (seam_lines[0] - 1, 3), (seam_lines[1] + 1, 1),
                  (seam_lines[0], seam_lines[2] - seam_lines[0] + 2), (n - 1, 1), (n - 1, 5), (n - 3, 3), (n - 2, 10**12),
                  (n, 1), (n + 5, 2), (7, 0), (0, 0), (1, None), (n // 2, None)]
        for first, count in ranges:
            end = n if count is None else first + count
            assert f.line_hashes(first, count).tolist() == wanted[first:end], (first, count)
        assert f.line_hashes(seam_lines[1], 4, seed=1).tolist() == corpus["wanted"][(1, NL)][seam_lines[1]:seam_lines[1] + 4]
        assert f.tell() == 0                                        # positionless
    with native.IndexedBzip2File(corpus["path"], parallelization=parallelization) as f:
        assert f.line_hashes(3, 2).tolist() == wanted[3:5]


def small_file(folder, name, raw, level=9):
    path = folder / name
    path.write_bytes(datagen.compress(raw, level))
    return str(path)


def test_tails_empty_files_and_one_long_line(native, corpus):
    folder = corpus["folder"]
    for name, raw in (("empty.bz2", b""), ("newline.bz2", b"\n"), ("closed.bz2", b"beta\n\n"), ("tail.bz2", b"beta\nalpha beta\nalpha"),
                      ("nul.bz2", b"\0\n\0\0\n\0")):
        wanted = H.direct(raw, NL)
        with native.open(small_file(folder, name, raw), parallelization=1) as f:
            assert f.line_hashes().tolist() == wanted, name
            assert f.line_hashes(1).tolist() == wanted[1:] and f.line_hashes(0, 1).tolist() == wanted[:1], name
            assert f.count_distinct_lines() == len(set(H.lines_of(raw, NL))), name
            assert f.first_occurrences().tolist() == first_occurrences_of(H.lines_of(raw, NL)), name
    assert H.direct(b"beta\n\n", NL) == [H.line_hash(b"beta"), 0] and len(H.direct(b"\n", NL)) == 1
    # one line of 300 kB across several launches, terminated and not
    rng = random.Random(3)
    line = bytes(rng.choice(b"abcdefgh \0\xff") for _ in range(300_000))
    for name, raw in (("line.bz2", line), ("line-closed.bz2", line + b"\n"), ("line-between.bz2", b"a\n" + line + b"\nb")):
        path = small_file(folder, name, raw, level=1)
        for parallelization in (1, 0):
            with native.open(path, parallelization=parallelization) as f:
                assert len(f.block_offsets()) >= 4
                assert f.line_hashes().tolist() == H.direct(raw, NL), (name, parallelization)


def test_a_line_longer_than_one_step_of_the_link(native, corpus):
    """17 MB in one line are 260 tiles, more than the 256 that one step of k_linehash_link scans: the carry between its
    steps.  Runs of one byte, so that the file is small and the model is a closed form: x^n by squaring."""
    def run_of(value, n, x):
        unit, out = ((value + 1) % H.P, x), (0, 1)
        while n:
            if n & 1:
                out = H.followed_by(out, unit)
            unit = H.followed_by(unit, unit)
            n >>= 1
        return out
    raw = b"x\n" + b"a" * 9_000_000 + b"b" * 8_000_001 + b"\n\nthe tail"
    path = small_file(corpus["folder"], "runs.bz2", raw)
    for seed in (0, 1):
        x = H.base(seed)
        line = H.followed_by(run_of(ord("a"), 9_000_000, x), run_of(ord("b"), 8_000_001, x))[0]
        assert run_of(ord("a"), 5, x) == H.part(b"aaaaa", x)
        wanted = [H.line_hash(b"x", seed), line, 0, H.line_hash(b"the tail", seed)]
        with native.open(path, parallelization=0) as f:
            assert f.line_hashes(seed=seed).tolist() == wanted
            assert f.line_hashes(1, 2, seed=seed).tolist() == wanted[1:3]


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import numpy as np
import indexed_bzip2_amd as m

with m.open(sys.argv[2], parallelization=int(sys.argv[3])) as f:
    for first, count, seed in ((0, None, 0), (0, None, 1), (100, 2000, 0), (10**9, 5, 0), (3, 0, 0)):
        wanted = f.line_hashes(first, count, seed=seed)
        got = f.line_hashes_to_tensor(first, count, seed=seed)
        assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 1
        assert got.cpu().numpy().view(np.uint64).tolist() == wanted.tolist(), (first, count, seed)
        assert len(got) == 0 or int(got.min()) >= 0
        print(first, count, seed, len(got))
    hashes = f.line_hashes_to_tensor()
    assert int(torch.unique(hashes).numel()) == f.count_distinct_lines()
    assert f.tell() == 0
print("line hash tensor ok")
"""


@pytest.mark.parametrize("parallelization", [1, 0])
def test_line_hashes_to_tensor(native, corpus, parallelization):
    """In a process of its own that imports torch first; line_hashes itself is pinned to the model above."""
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, corpus["path"], str(parallelization)], capture_output=True, text=True,
                         timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "line hash tensor ok" in run.stdout and "0 None 0 0" not in run.stdout


def first_occurrences_of(lines):
    seen, numbers = {}, []
    for k, content in enumerate(lines):
        if content not in seen:
            seen[content] = k
            numbers.append(k)
    return numbers


def duplicates_text():
    """The reader's corpus with planted duplicates: adjacent, far apart, across blocks, empty lines, and an unterminated
    tail that equals an earlier terminated line."""
    lines = reader_text().split(b"\n")[:-1]
    rng = random.Random(0xD0B1E)
    n = len(lines)
    for k in rng.sample(range(10, n - 10), 300):
        lines[k] = lines[k - 1]                                     # adjacent
    for k in rng.sample(range(n // 2, n), 300):
        lines[k] = lines[rng.randrange(0, n // 4)]                  # far apart, in other blocks
    for k in rng.sample(range(n), 50):
        lines[k] = b"the same line everywhere"
    lines[n - 1] = lines[0]
    lines[7] = b"line seven is also the tail"
    return b"\n".join(lines) + b"\n" + lines[7]                     # the tail is line 7 again, without a delimiter


@pytest.fixture(scope="module")
def duplicates(native, corpus):
    raw = duplicates_text()
    lines = H.lines_of(raw, NL)
    assert not raw.endswith(b"\n") and lines[-1] == lines[7]
    # a condition on the input, checked on the CPU with the model: distinct contents have distinct hashes under both
    # seeds, so a collision can neither hide a failure nor cause one
    for seed in (0, 1):
        hashes = H.Prefix(raw, H.base(seed)).lines(NL)
        assert len(set(hashes)) == len(set(lines)) and len(hashes) == len(lines)
    return {"raw": raw, "lines": lines, "path": small_file(corpus["folder"], "duplicates.bz2", raw, level=1)}


@pytest.mark.parametrize("parallelization", [1, 0])
def test_distinct_lines(native, duplicates, parallelization):
    lines = duplicates["lines"]
    numbers = first_occurrences_of(lines)
    assert 1000 < len(numbers) < len(lines) - 500
    with native.open(duplicates["path"], parallelization=parallelization) as f:
        assert len(f.block_offsets()) >= 5                          # a full read: it moves the position
    with native.open(duplicates["path"], parallelization=parallelization) as f:
        for seed in (0, 1):
            assert f.count_distinct_lines(seed=seed) == len(numbers)
            got = f.first_occurrences(seed=seed)
            assert got.dtype == np.uint64 and got.tolist() == numbers
        # the numbers are ready for read_line_ranges
        some = numbers[:5] + numbers[-5:]
        assert f.read_line_ranges([(k, 1) for k in some]) == [lines[k] + (b"\n" if k < len(lines) - 1 else b"") for k in some]
        # another delimiter
        pieces = H.lines_of(duplicates["raw"], ord(" "))
        assert f.count_distinct_lines(newline=b" ") == len(set(pieces))
        assert f.tell() == 0
    with native.IndexedBzip2File(duplicates["path"], parallelization=parallelization) as f:
        assert f.count_distinct_lines() == len(numbers) and f.first_occurrences().tolist() == numbers


def test_tool(native, corpus, duplicates):
    for seed in (0, 1):
        options = [] if seed == 0 else ["--seed", "1"]
        run = subprocess.run([CLI, "--line-hashes"] + options + ["-P", "1", corpus["path"]], capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr
        assert run.stdout == b"".join(b"%016x\n" % h for h in corpus["wanted"][(seed, NL)])
        run = subprocess.run([CLI, "--count-distinct-lines"] + options + [duplicates["path"]], capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr
        assert run.stdout == b"%d\n" % len(set(duplicates["lines"]))
