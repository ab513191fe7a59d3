"""Line access on the GPU: the newline index (line_offsets, count_lines), line_starts, read_line_ranges / read_lines /
read_line_ranges_to_tensor of the reader, the k_count_byte and k_find_byte kernels under them (Decoder.count_byte,
Decoder.find_byte), and `ibzip2-mi355x --count-lines`.

The corpus is seeded and compressed with CPython's bz2: lines of random length 0-400 up to 6 MB, with ONE 3.5 MB line of
random printable bytes in the middle (random, because a run of one byte would collapse into a single block), no newline at
the end: about 9.5 MB and 30 000 newlines, about 95 blocks at level 1 and 11 at level 9; the long line spans dozens of
level-1 blocks, which therefore hold no newline.  It is used at level 1, at level 9, as two streams behind each other and
with a newline at the end; plus the golden fixtures `empty`, `1B` and `zeros`.

Every expected value comes from the raw bytes: raw.count(nl), and the line starts from numpy.flatnonzero (never
bytes.splitlines, which also splits on \\r)."""
import bisect
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, read_fixture
import datagen

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
NL = b"\n"
LINES_BYTES = 6_000_000
LONG_LINE = 3_500_000
RANGES = 500


def make_raw(seed=0x11E5):
    r = datagen.rng(seed)
    lengths = r.integers(0, 401, LINES_BYTES // 150)
    ends = np.cumsum(lengths + 1)                       # position behind every line's newline
    ends = ends[ends <= LINES_BYTES]
    text = r.integers(32, 127, int(ends[-1]), dtype=np.uint8)
    text[ends - 1] = 10
    half = int(ends[len(ends) // 2])                     # a line start in the middle
    long_line = r.integers(32, 127, LONG_LINE, dtype=np.uint8)
    long_line[-1] = 10
    tail = r.integers(32, 127, 173, dtype=np.uint8)      # an unterminated last line
    return np.concatenate([text[:half], long_line, text[half:], tail]).tobytes()


def line_starts_of(raw, nl=NL):
    """s(k) for k = 0..N as a numpy array of N + 1 offsets."""
    positions = np.flatnonzero(np.frombuffer(raw, dtype=np.uint8) == nl[0])
    return np.concatenate([[0], positions + 1]).astype(np.int64)


def expected_range(raw, s, first, count):
    n = len(s) - 1
    if first > n or count == 0:
        return b""
    if first + count <= n:
        return raw[int(s[first]):int(s[first + count])]
    return raw[int(s[first]):]


def data_block_starts(block_index):
    items = sorted(block_index.items())
    return [s for (_, s), (_, e) in zip(items, items[1:]) if e > s]


def python_line_index(raw, block_index, nl=NL):
    s = line_starts_of(raw, nl)
    index = {start: int(np.searchsorted(s[1:], start, side="right")) for start in data_block_starts(block_index)}
    # (s[k] <= start  <=>  the k-th delimiter lies in front of `start`)
    index[len(raw)] = len(s) - 1
    return index


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    raw = make_raw()
    assert 9_000_000 < len(raw) < 10_000_000 and 25_000 < raw.count(NL) < 35_000 and not raw.endswith(NL)
    folder = tmp_path_factory.mktemp("lines")
    variants = {
        "level1": (raw, datagen.compress(raw, 1)),
        "level9": (raw, datagen.compress(raw, 9)),
        "two-streams": (raw + raw, datagen.compress(raw, 9) + datagen.compress(raw, 5)),
        "ends-with-newline": (raw + NL, datagen.compress(raw + NL, 9)),
    }
    out = {}
    for name, (data, enc) in variants.items():
        path = folder / (name + ".bz2")
        path.write_bytes(enc)
        with native.open(str(path), parallelization=0) as f:
            block_index = f.block_offsets()
        out[name] = {"path": str(path), "raw": data, "enc": enc, "blocks": block_index,
                     "starts": line_starts_of(data), "lines": python_line_index(data, block_index)}
    assert 80 <= len(data_block_starts(out["level1"]["blocks"])) <= 110
    assert 9 <= len(data_block_starts(out["level9"]["blocks"])) <= 13
    # dozens of level-1 blocks without any newline
    values = [v for _, v in sorted(out["level1"]["lines"].items())]
    assert sum(1 for a, b in zip(values, values[1:]) if a == b) >= 25
    return out


VARIANTS = ["level1", "level9", "two-streams", "ends-with-newline"]


def seeded_line_ranges(s, seed, count=RANGES):
    """Counts 0, 1, a few and thousands; starts anywhere up to a little beyond N; neighbours that overlap; ranges that
    cover the long line (the longest one)."""
    rng = np.random.default_rng(seed)
    n = len(s) - 1
    longest = int(np.argmax(np.diff(s)))
    out = [(longest, 1), (max(longest - 2, 0), 5), (longest, 0), (longest + 1, 3), (0, 1), (n, 1), (n + 1, 1), (n, 7),
           (0, 0), (n - 1, 2), (n + 3, 10**12)]
    while len(out) < count:
        kind = len(out) % 8
        first = int(rng.integers(0, n + 6))
        size = 0 if kind == 0 else 1 if kind < 3 else int(rng.integers(2, 20)) if kind < 6 \
            else int(rng.integers(1000, 6000))
        out.append((first, size))
        if kind == 4:
            out.append((first + 1, size))     # overlaps its neighbour
    return out[:count]


def spanned_blocks(line_index, ranges):
    """The distinct data blocks the ranges span, from the two indexes alone: the block that holds the first-th delimiter
    (the first block for line 0) through the block that holds the (first + count)-th, or the last block."""
    values = [v for _, v in sorted(line_index.items())]    # lines in front of block b, ..., N
    n, last = values[-1], len(values) - 2
    holding = lambda k: bisect.bisect_left(values, k) - 1   # values[b] < k <= values[b + 1]
    needed = set()
    for first, count in ranges:
        if first > n or count == 0 or last < 0:
            continue
        begin = 0 if first == 0 else holding(first)
        end = last if first + count > n else holding(first + count)
        needed.update(range(begin, end + 1))
    return needed


# ------------------------------------------------------------------------------------------------ the kernels

def test_count_and_find_kernels(native, corpus):
    """Counts and positions for spans at every start alignment 0-15, lengths 0-40 and several tiles, inside one block and
    across a block boundary; rank 1, last, and one too many; against the same slices of copy_output."""
    c = corpus["level9"]
    offsets = sorted(k for k, v in c["blocks"].items())[:2]
    dec = native.Decoder(device=0)
    dec.set_input(c["enc"])
    results, total = dec.decode_batch(offsets)
    out = dec.copy_output(0, total)
    assert out == c["raw"][:total]
    first = results[0]["decoded_size"]
    arr = np.frombuffer(out, dtype=np.uint8)
    for value in (10, ord("e"), 0):
        for crossing in (False, True):
            base = ((first - 24) & ~15) if crossing else 16 * 1000
            for sm in range(16):
                spans = []
                for size in list(range(41)) + [1000, 65536, 65537, 3 * 65536 + 13, 700_000]:
                    src = base + sm if size < 1000 else base + sm - (size // 2 if crossing else 0)
                    spans.append((src, size))
                want = [out[o:o + n].count(bytes([value])) for o, n in spans]
                assert dec.count_byte(value, spans) == want, (value, crossing, sm)
                queries, expect = [], []
                for (o, n), count in zip(spans, want):
                    hits = o + np.flatnonzero(arr[o:o + n] == value)
                    for rank in {1, max(1, count // 2), max(1, count), count + 1}:
                        queries.append((o, n, rank))
                        expect.append(int(hits[rank - 1]) if rank <= count else None)
                assert dec.find_byte(value, queries) == expect, (value, crossing, sm)
    # the whole output as one span: dozens of tiles
    hits = np.flatnonzero(arr == 10)
    assert dec.count_byte(10, [(0, total), (0, total), (1, total - 1)]) == [len(hits), len(hits), len(hits[hits >= 1])]
    ranks = [1, 2, len(hits) // 3, len(hits) // 2, len(hits) - 1, len(hits)]
    assert dec.find_byte(10, [(0, total, r) for r in ranks] + [(0, total, len(hits) + 1)]) \
        == [int(hits[r - 1]) for r in ranks] + [None]
    assert dec.count_byte(10, []) == [] and dec.find_byte(10, []) == []
    # spans outside the output and rank 0 are refused
    with pytest.raises(native.Bz2Error):
        dec.count_byte(10, [(total - 10, 11)])
    with pytest.raises(native.Bz2Error):
        dec.find_byte(10, [(total + 1, 0, 1)])
    with pytest.raises(native.Bz2Error):
        dec.find_byte(10, [(0, 100, 0)])
    dec.close()


# ------------------------------------------------------------------------------------------------ the index

@pytest.mark.parametrize("indexed", [True, False], ids=["imported-block-index", "on-the-fly"])
@pytest.mark.parametrize("parallelization", [1, 4, 0])
@pytest.mark.parametrize("variant", VARIANTS)
def test_line_offsets(native, corpus, variant, parallelization, indexed):
    c = corpus[variant]
    raw = c["raw"]
    with native.open(c["path"], parallelization=parallelization) as f:
        if indexed:
            f.set_block_offsets(c["blocks"])
        f.seek(1_234_567)
        assert f.read(1000) == raw[1_234_567:1_235_567]
        before = f.statistics()
        got = f.line_offsets()
        after = f.statistics()
        assert got == c["lines"]
        assert f.count_lines() == raw.count(NL)
        if indexed:
            # (the read() in front may have had look-ahead launches in flight: they are counted when they finish)
            blocks = len(data_block_starts(c["blocks"]))
            assert after["blocks_decoded"] - before["blocks_decoded"] >= blocks
        # positionless: tell() and the next read() are as if the call had not happened
        assert f.tell() == 1_235_567
        assert f.read(300_000) == raw[1_235_567:1_535_567]
        assert f.block_offsets() == c["blocks"]
        # another delimiter replaces the index
        assert f.count_lines(b"e") == raw.count(b"e")
        assert f.line_offsets(b"e") == python_line_index(raw, c["blocks"], b"e")


@pytest.mark.parametrize("variant", ["level1", "two-streams"])
def test_index_decodes_each_block_once(native, corpus, variant):
    """With the block map imported and nothing else around the call, building the line index decodes every data block
    exactly once, in as few launches as the batch size allows."""
    c = corpus[variant]
    blocks = len(data_block_starts(c["blocks"]))
    for parallelization, cap in ((1, 1), (4, 4), (0, 512)):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            before = f.statistics()
            assert f.count_lines() == c["raw"].count(NL)
            after = f.statistics()
            assert after["blocks_decoded"] - before["blocks_decoded"] == blocks
            assert after["batches"] - before["batches"] == -(-blocks // cap)
            assert f.count_lines() == c["raw"].count(NL) and f.line_offsets() == c["lines"]
            assert f.statistics()["blocks_decoded"] == after["blocks_decoded"]      # the index is kept
            assert f.tell() == 0
            assert f.read(5000) == c["raw"][:5000]


# ------------------------------------------------------------------------------------------------ line ranges

@pytest.mark.parametrize("parallelization", [1, 4, 0])
@pytest.mark.parametrize("variant", VARIANTS)
def test_random_line_ranges(native, corpus, variant, parallelization):
    c = corpus[variant]
    raw, s = c["raw"], c["starts"]
    n = len(s) - 1
    ranges = seeded_line_ranges(s, 0x11AE + parallelization)
    want = [expected_range(raw, s, first, count) for first, count in ranges]
    assert any(len(w) > LONG_LINE for w in want) and any(w == b"" for w in want)
    lines = [first for first, _ in ranges] + [0, n, n + 1, 2**63]
    want_starts = [int(s[k]) if k <= n else len(raw) for k in lines]
    for both in (True, False):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            if both:
                f.set_line_offsets(c["lines"])
            f.seek(777)
            got = f.read_line_ranges(ranges)
            for (first, count), g, w in zip(ranges, got, want):
                assert g == w, (first, count, len(g), len(w))
            starts = f.line_starts(lines)
            assert starts.dtype == np.uint64 and list(starts) == want_starts
            for first, count in ranges[:12] + ranges[-6:]:
                assert f.read_lines(first, count) == expected_range(raw, s, first, count)
            assert f.read_lines(5) == expected_range(raw, s, 5, 1)
            assert f.read_line_ranges([]) == []
            assert f.tell() == 777
            assert f.read(100_000) == raw[777:100_777]
            assert f.line_offsets() == c["lines"]
            assert f.block_offsets() == c["blocks"]


def test_each_block_once_per_call(native, corpus):
    """With both indexes imported and nothing else around the call, the statistics count exactly the call's launches:
    every block the ranges span once (the set is computed here from the two indexes), in launches of at most the cap."""
    c = corpus["level1"]
    raw, s = c["raw"], c["starts"]
    rng = np.random.default_rng(0x0CE)
    n = len(s) - 1
    ranges = [(int(rng.integers(0, n + 3)), int(rng.integers(0, 40))) for _ in range(60)] + [(n, 3), (0, 2)]
    distinct = len(spanned_blocks(c["lines"], ranges))
    assert 20 < distinct < len(data_block_starts(c["blocks"]))
    want = [expected_range(raw, s, first, count) for first, count in ranges]
    for parallelization, cap in ((1, 1), (4, 4), (0, 512)):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            f.set_line_offsets(c["lines"])
            before = f.statistics()
            got = f.read_line_ranges(ranges)
            after = f.statistics()
            assert got == want
            assert after["blocks_decoded"] - before["blocks_decoded"] == distinct
            assert after["batches"] - before["batches"] == -(-distinct // cap)
            # a second call decodes them again (nothing is kept), and gives the same bytes
            assert f.read_line_ranges(ranges) == got
            # line_starts decodes only the blocks that hold a boundary
            lines = [first for first, _ in ranges]
            values = [v for _, v in sorted(c["lines"].items())]
            holding = {bisect.bisect_left(values, k) - 1 for k in lines if 1 <= k <= n}
            before = f.statistics()
            assert list(f.line_starts(lines)) == [int(s[k]) if k <= n else len(raw) for k in lines]
            after = f.statistics()
            assert after["blocks_decoded"] - before["blocks_decoded"] == len(holding) <= distinct


def test_bounded_residency(native, corpus, monkeypatch):
    """The compressed file is not kept on the GPU: every launch brings the packed windows of its own blocks."""
    c = corpus["level1"]
    raw, s = c["raw"], c["starts"]
    ranges = seeded_line_ranges(s, 0xB0B, count=80)
    want = [expected_range(raw, s, first, count) for first, count in ranges]
    monkeypatch.setenv("MI355X_BZ2_INPUT_BUDGET", "1048576")
    for parallelization in (4, 0):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            assert f.statistics()["input_resident"] == 0
            assert f.line_offsets() == c["lines"]
            assert f.read_line_ranges(ranges) == want
            few = ranges[-5:]
            before = f.statistics()["input_bytes_uploaded"]
            assert f.read_line_ranges(few) == want[-5:]
            uploaded = f.statistics()["input_bytes_uploaded"] - before
            assert 0 < uploaded
        with native.open(c["path"], parallelization=parallelization) as f:      # everything on the fly
            assert f.read_line_ranges(ranges[:20]) == want[:20]
            assert f.statistics()["input_resident"] == 0


def test_lying_line_index(native, corpus):
    """An imported line index with one count raised by 1 fails the call that looks for the promised delimiter; the
    reader works afterwards."""
    c = corpus["level9"]
    raw, s = c["raw"], c["starts"]
    keys = sorted(c["lines"])
    values = [c["lines"][k] for k in keys]
    # block b gets one more, in both possible readings: only the entry behind it raised (the next block then has one
    # fewer), or every entry behind it raised (N grows by one)
    b = 2
    assert values[b + 2] - values[b + 1] >= 1
    one_entry = dict(c["lines"])
    one_entry[keys[b + 1]] += 1
    all_behind = {k: v + (1 if i > b else 0) for i, (k, v) in enumerate(zip(keys, values))}
    for lying in (one_entry, all_behind):
        with native.open(c["path"], parallelization=4) as f:
            f.set_block_offsets(c["blocks"])
            f.set_line_offsets(lying)
            assert f.line_offsets() == lying
            promised = lying[keys[b + 1]]       # the last delimiter block b is said to hold
            with pytest.raises(native.Bz2Error) as failure:
                f.read_line_ranges([(3, 2), (promised, 1)])
            assert failure.value.status == 106 and "line index" in str(failure.value)
            with pytest.raises(native.Bz2Error):
                f.line_starts([promised])
            with pytest.raises(native.Bz2Error):
                f.read_lines(promised - 1)       # ends with the delimiter that is not there
            # lines in blocks the lie does not touch are served; then the true index is served as ever
            assert f.read_lines(3, 2) == expected_range(raw, s, 3, 2)
            f.set_line_offsets(c["lines"])
            assert f.read_lines(promised, 2) == expected_range(raw, s, promised, 2)
            assert f.read(1000) == raw[:1000]


def test_damaged_block(native, corpus, tmp_path):
    """One byte flipped inside a block: building the line index (its counting launches decode every block) fails with
    the block's status and bit offset and leaves no index behind -- a second call fails the same way instead of returning
    a partial one --, and read_ranges of clean ranges works after each failure."""
    c = corpus["level9"]
    raw = c["raw"]
    items = sorted(c["blocks"].items())
    blocks = [(b, nb, s, e) for (b, s), (nb, e) in zip(items, items[1:]) if e > s]
    bits, next_bits, start, stop = blocks[4]
    damaged = bytearray(c["enc"])
    damaged[(bits + next_bits) // 16] ^= 0xFF
    bad = tmp_path / "damaged.bz2"
    bad.write_bytes(bytes(damaged))
    avoid = [(blocks[k][2] + 10, 5000) for k in (0, 3, 5, 8)] + [(start - 100, 100), (stop, 300)]
    with native.open(str(bad), parallelization=4) as f:
        f.set_block_offsets(c["blocks"])
        for call in (f.line_offsets, f.line_offsets, f.count_lines):
            with pytest.raises(native.Bz2Error) as failure:
                call()
            assert failure.value.status != 0
            assert f"bit offset {bits}" in str(failure.value)
            assert f.read_ranges(avoid) == [raw[o:o + s] for o, s in avoid]
        assert f.read(1000) == raw[:1000]


def test_argument_errors(native, corpus):
    c = corpus["level9"]
    with native.open(c["path"], parallelization=4) as f:
        for bad in (b"", b"\r\n", "\n", None, 10):
            with pytest.raises(ValueError):
                f.count_lines(bad)
            with pytest.raises(ValueError):
                f.read_lines(0, 1, bad)
        with pytest.raises(ValueError):
            f.read_line_ranges([(-1, 1)])
        with pytest.raises(ValueError):
            f.read_line_ranges([(0, -1)])
        with pytest.raises(ValueError):
            f.read_lines(-1)
        with pytest.raises(ValueError):
            f.line_starts([3, -3])
        # a line index needs the complete block map
        with pytest.raises(ValueError):
            f.set_line_offsets(c["lines"])
        f.set_block_offsets(c["blocks"])
        f.set_line_offsets(c["lines"])
        keys = sorted(c["lines"])
        for wrong in ({k: v for k, v in c["lines"].items() if k != keys[3]},            # a block is missing
                      {**c["lines"], keys[3] + 1: c["lines"][keys[3]]},                # not a block start
                      {k: v + 1 for k, v in c["lines"].items()},                       # does not start at 0
                      {**c["lines"], keys[3]: c["lines"][keys[4]] + 1},                # decreases behind it
                      {k: (v if i < 2 else v + 2_000_000) for i, (k, v) in enumerate(sorted(c["lines"].items()))},
                      {}):
            with pytest.raises(ValueError):
                f.set_line_offsets(wrong)
        assert f.line_offsets() == c["lines"]        # a refused import changes nothing
        assert f.read_lines(7) == expected_range(c["raw"], c["starts"], 7, 1)
    with pytest.raises(ValueError):
        f.read_lines(0)


# ------------------------------------------------------------------------------------------------ fixtures, tool

def test_golden_fixtures(native, tmp_path):
    for parallelization in (1, 0):
        enc, raw = read_fixture("empty")
        path = tmp_path / "empty.bz2"
        path.write_bytes(enc)
        with native.open(str(path), parallelization=parallelization) as f:
            assert raw == b"" and f.line_offsets() == {0: 0} and f.count_lines() == 0
            assert f.read_line_ranges([(0, 1), (0, 0), (1, 5)]) == [b"", b"", b""]
            assert list(f.line_starts([0, 1, 9])) == [0, 0, 0]
            assert f.read() == b""

        enc, raw = read_fixture("1B")
        path = tmp_path / "1B.bz2"
        path.write_bytes(enc)
        with native.open(str(path), parallelization=parallelization) as f:
            assert len(raw) == 1
            assert f.count_lines() == raw.count(NL)
            assert f.read_lines(0, 5) == raw
            assert f.count_lines(raw) == 1              # its one byte as the delimiter
            assert f.read_line_ranges([(0, 1), (1, 1), (2, 1)], raw) == [raw, b"", b""]
            assert f.read() == raw

        enc, raw = read_fixture("zeros")
        path = tmp_path / "zeros.bz2"
        path.write_bytes(enc)
        with native.open(str(path), parallelization=parallelization) as f:
            assert raw.count(b"\0") == len(raw) > 50
            assert f.count_lines(b"\0") == len(raw)     # every byte is a delimiter
            rng = np.random.default_rng(5)
            lines = [0, len(raw) - 1] + [int(x) for x in rng.integers(0, len(raw), 48)]
            assert f.read_line_ranges([(k, 1) for k in lines], b"\0") == [b"\0"] * 50
            assert list(f.line_starts(lines + [len(raw), len(raw) + 1], b"\0")) == lines + [len(raw), len(raw)]
            assert f.read_lines(len(raw), 1, b"\0") == b""          # the empty tail
            assert f.read_lines(len(raw) - 3, 10, b"\0") == b"\0" * 3
            assert f.count_lines() == 0
            assert f.read_lines(0) == raw


def test_count_lines_tool(native, corpus, tmp_path):
    for name in ("level9", "ends-with-newline"):
        run = subprocess.run([CLI, "--count-lines", corpus[name]["path"]], capture_output=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        assert run.stdout == b"%d\n" % corpus[name]["raw"].count(NL)
    run = subprocess.run([CLI, "--count-lines", "-P", "4", os.path.join(ROOT, "tests", "golden", "fixtures", "empty.bz2")],
                         capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b"0\n"


# ------------------------------------------------------------------------------------------------ device destination

CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import indexed_bzip2_amd as m
from test_gpu_lines import expected_range, line_starts_of, seeded_line_ranges

path, raw = sys.argv[2], open(sys.argv[3], "rb").read()
s = line_starts_of(raw)
for parallelization in (1, 4, 0):
    ranges = seeded_line_ranges(s, 0x7E4 + parallelization)
    want = [expected_range(raw, s, first, count) for first, count in ranges]
    with m.open(path, parallelization=parallelization) as f:
        before = f.statistics()
        data, offsets = f.read_line_ranges_to_tensor(ranges)
        assert data.dtype == torch.uint8 and data.is_cuda and data.dim() == 1
        assert offsets.dtype == torch.int64 and not offsets.is_cuda and offsets.numel() == len(ranges) + 1
        bounds = [0]
        for w in want:
            bounds.append(bounds[-1] + len(w))
        assert offsets.tolist() == bounds and data.numel() == bounds[-1]
        assert bytes(data.cpu().numpy()) == b"".join(want)
        assert f.read_line_ranges(ranges) == want
        # nothing to gather
        data, offsets = f.read_line_ranges_to_tensor([(0, 0), (10**9, 4)])
        assert data.numel() == 0 and offsets.tolist() == [0, 0, 0]
        data, offsets = f.read_line_ranges_to_tensor([])
        assert data.numel() == 0 and offsets.tolist() == [0]
        # a device result is not handed to a host destination
        f.bz2reader._read_line_ranges([(0, 1)], b"\n", True)
        try:
            f.bz2reader._check(m.lib().mi355x_bz2_reader_take_line_ranges(f.bz2reader._h, None, 0))
            raise SystemExit("a held device result was written to the host")
        except ValueError:
            pass
        assert f.tell() == 0
        assert f.read(4096) == raw[:4096]
print("device lines ok")
"""


@pytest.mark.parametrize("variant", ["level1", "two-streams"])
def test_device_destination(native, corpus, variant, tmp_path):
    c = corpus[variant]
    raw_path = tmp_path / "raw"
    raw_path.write_bytes(c["raw"])
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, c["path"], str(raw_path)], capture_output=True, text=True,
                         timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "device lines ok" in run.stdout
