"""Search on the GPU: count_matches / find_all / find of the reader, the k_count_bytes / k_emit_bytes kernels under them
(Decoder.count_bytes, Decoder.find_bytes) and `ibzip2-mi355x --count-matches`.

Corpus A: 1 000 000 seeded printable bytes with no two equal neighbours, compressed with CPython's bz2 at level 1.  Such
data holds no run, so every block takes exactly 99 981 decoded bytes: 10 blocks of 99 981 and one of 190 (asserted from
block_offsets()).  The needles are the prefixes of one seeded 256-byte string without equal neighbours, of the lengths
m in {2, 3, 4, 5, 15, 16, 17, 33, 255, 256}.  A needle is planted so that it starts j bytes in front of a block boundary
k * 99 981 and in front of every multiple of 4 096 in the first 256 KiB, j in {1, m/2, m - 1, m} (j = m ends exactly on
the boundary), and at a few seeded places inside blocks.  Two plants of one boundary would overwrite each other -- all of
them cover the byte in front of it -- so there is ONE copy of corpus A PER NEEDLE, and in it j takes its four values in
turn from boundary to boundary, in an order that lets the needle straddle nine of the ten block boundaries (at least 8
expected matches that straddle a block boundary are asserted per needle) and end exactly on the remaining one.  The
shorter needles are prefixes of the longer ones, so the copy of m = 256 holds matches of every needle at every plant.

Corpus B: 60 concatenated streams of b"ab", b"c", b"", b"abc", b"a", b"bca" repeated: blocks of 1 to 3 bytes and streams
without any block, so that at parallelization 1 the extents are shorter than the patterns and one match crosses several
launches.

Every expected value comes from the raw bytes: a raw.find(P, p + 1) loop, numpy.flatnonzero for single bytes, never
bytes.count (which skips matches that overlap the one before)."""
import bz2
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, read_fixture
import datagen

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
SIZE = 1_000_000
BLOCK = 99_981
LENGTHS = [2, 3, 4, 5, 15, 16, 17, 33, 255, 256]
ALL = 2**64 - 1


def no_equal_neighbours(r, n):
    """n printable bytes, each different from the one in front of it."""
    steps = r.integers(1, 95, n)
    steps[0] = r.integers(0, 95)
    return (32 + np.cumsum(steps) % 95).astype(np.uint8)


def matches_of(raw, pattern, start=0, end=None):
    """Every p with raw[p:p + m] == pattern, start <= p and p + m <= end (clipped), overlapping ones included."""
    end = len(raw) if end is None else min(end, len(raw))
    start = min(start, end)
    if len(pattern) == 1:
        return [start + int(p) for p in np.flatnonzero(np.frombuffer(raw, dtype=np.uint8)[start:end] == pattern[0])]
    found = []
    p = raw.find(pattern, start, end)
    while p != -1:
        found.append(p)
        p = raw.find(pattern, p + 1, end)
    return found


def js_of(m):
    return [1, max(1, m // 2), m - 1, m]


def make_corpus_a(m, master, base):
    """The copy of corpus A for the needle of length m: (raw, needle, plants)."""
    data = base.copy()
    needle = master[:m]
    r = datagen.rng(0xA000 + m)
    # the ten block boundaries: nine straddled, j in turn, and one (the fourth) that the needle ends on; the last
    # boundary has 190 bytes behind it and gets j = m - 1
    one, half, most, whole = js_of(m)
    turn = [one, half, most, whole, one, half, most, one, half, most]
    plants = [k * BLOCK - j for k, j in zip(range(1, 11), turn)]
    # every multiple of 4 096 in the first 256 KiB that no block-boundary plant is near
    for k in range(1, 64):
        at = k * 4096 - js_of(m)[k % 4]
        if all(abs(at - p) > 2 * m + 2 for p in plants):
            plants.append(at)
    # seeded places inside blocks
    for _ in range(6):
        at = int(r.integers(0, 10)) * BLOCK + int(r.integers(2000, BLOCK - 2000))
        if at > 270_000 and all(abs(at - p) > 2 * m + 2 for p in plants):
            plants.append(at)
    for at in plants:
        assert 0 <= at and at + m <= SIZE
        data[at:at + m] = needle
    return data.tobytes(), needle.tobytes(), sorted(plants)


@pytest.fixture(scope="module")
def corpus_a(native, tmp_path_factory):
    r = datagen.rng(0x5EA2C4)
    base = no_equal_neighbours(r, SIZE)
    master = no_equal_neighbours(r, 256)
    folder = tmp_path_factory.mktemp("search")
    boundaries = [k * BLOCK for k in range(1, 11)]
    out = {}
    for m in LENGTHS:
        raw, needle, plants = make_corpus_a(m, master, base)
        assert len(raw) == SIZE and len(needle) == m
        assert all(needle[i:i + 1] * 4 != needle[i:i + 4] for i in range(m))          # no run of 4
        path = folder / f"a{m}.bz2"
        path.write_bytes(bz2.compress(raw, 1))
        with native.open(str(path), parallelization=0) as f:
            blocks = f.block_offsets()
        starts = sorted(blocks.values())
        assert sorted(set(starts)) == [k * BLOCK for k in range(11)] + [SIZE], starts
        expected = matches_of(raw, needle)
        straddling = [p for p in expected if any(p < b < p + m for b in boundaries)]
        assert len(straddling) >= 8, (m, straddling)
        assert any(p + m == b for p in expected for b in boundaries)                  # ends exactly on a boundary
        assert set(plants) <= set(expected)
        out[m] = {"path": str(path), "raw": raw, "needle": needle, "plants": plants, "blocks": blocks,
                  "expected": expected, "straddling": straddling, "master": master.tobytes()}
    return out


def seeded_ranges(c, m, seed):
    """50 (start, end) pairs: start and end inside a planted needle, end - start in {0, m - 1, m}, start beyond the size,
    around the boundaries the needle straddles, and seeded ones from a few bytes to several blocks."""
    r = np.random.default_rng(seed)
    plant, other = c["straddling"][2], c["plants"][len(c["plants"]) // 2]
    ranges = [(plant + 1, plant + m + 5), (plant - 5, plant + m - 1), (plant, plant + m), (plant, plant + m - 1),
              (other + m // 2, other + 3 * m), (other - 3 * m, other + m // 2 + 1), (other, other + m), (other + 1, other + m),
              (1234, 1234), (1234, 1234 + m - 1), (1234, 1234 + m), (5000, 4000),
              (SIZE + 5, SIZE + 100), (SIZE, ALL), (SIZE - 3, 2**63), (SIZE - m, SIZE), (SIZE - 191, ALL), (0, ALL)]
    for p in c["straddling"][:8]:
        ranges.append((p - int(r.integers(0, 40)), p + m + int(r.integers(0, 40))))
    while len(ranges) < 50:
        kind = len(ranges) % 4
        start = int(r.integers(0, SIZE))
        size = int(r.integers(0, 300)) if kind == 0 else int(r.integers(300, BLOCK)) if kind == 1 \
            else int(r.integers(BLOCK, 3 * BLOCK)) if kind == 2 else int(r.integers(3 * BLOCK, 6 * BLOCK))
        ranges.append((start, start + size))
    return [(max(0, a), b) for a, b in ranges[:50]]


# ------------------------------------------------------------------------------------------------ corpus A

@pytest.mark.parametrize("parallelization", [1, 3, 0])
@pytest.mark.parametrize("m", LENGTHS)
def test_block_and_launch_seams(native, corpus_a, m, parallelization):
    c = corpus_a[m]
    raw, needle, expected = c["raw"], c["needle"], c["expected"]
    total = len(expected)
    with native.open(c["path"], parallelization=parallelization) as f:
        if parallelization != 3:
            f.set_block_offsets(c["blocks"])          # at 3 the file is indexed by the search itself
        f.seek(4321)
        # the full range
        assert f.count_matches(needle) == total
        got = f.find_all(needle)
        assert got.dtype == np.uint64 and got.tolist() == expected
        assert f.find(needle) == expected[0]
        for limit in (1, 2, total, total + 1):
            assert f.find_all(needle, limit=limit).tolist() == expected[:limit], limit
        assert f.find_all(needle, limit=0).tolist() == []
        # ranges
        for k, (start, end) in enumerate(seeded_ranges(c, m, 0x5EED + m)):
            want = matches_of(raw, needle, start, end)
            assert f.find_all(needle, start, end).tolist() == want, (start, end)
            if k < 20:
                assert f.count_matches(needle, start, end) == len(want), (start, end)
                assert f.find(needle, start, end) == (want[0] if want else -1), (start, end)
        # bytes-like patterns
        assert f.count_matches(bytearray(needle)) == total and f.count_matches(memoryview(needle)) == total
        assert f.tell() == 4321
        assert f.read(1000) == raw[4321:5321]


def test_every_needle_in_one_file(native, corpus_a):
    """The copy of m = 256 holds every shorter needle at every plant; and the single bytes of the text."""
    c = corpus_a[256]
    raw = c["raw"]
    for parallelization in (1, 0):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            for m in LENGTHS:
                needle = c["master"][:m]
                want = matches_of(raw, needle)
                assert len(want) >= len(c["plants"])
                assert f.count_matches(needle) == len(want)
                assert f.find_all(needle).tolist() == want
            for one in (b"a", b"~", b" ", b"\n"):
                want = matches_of(raw, one)
                assert f.count_matches(one) == len(want)
                assert f.find_all(one, 7, SIZE - 9).tolist() == [p for p in want if 7 <= p < SIZE - 9]


def test_each_block_once_and_the_limit_stops_launches(native, corpus_a):
    c = corpus_a[16]
    raw, needle = c["raw"], c["needle"]
    for parallelization, cap in ((1, 1), (3, 3), (0, 512)):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            before = f.statistics()
            assert f.count_matches(needle) == len(c["expected"])
            after = f.statistics()
            assert after["blocks_decoded"] - before["blocks_decoded"] == 11
            assert after["batches"] - before["batches"] == -(-11 // cap)
            # blocks 2 to 5 intersect this range
            start, end = 2 * BLOCK + 17, 5 * BLOCK + 1
            assert f.find_all(needle, start, end).tolist() == matches_of(raw, needle, start, end)
            assert f.statistics()["blocks_decoded"] - after["blocks_decoded"] == 4
            # the first match lies in the first block: launches behind the one that found it are not started
            before = f.statistics()
            assert f.find(needle) == c["expected"][0] < BLOCK - 256
            if parallelization == 1:
                assert f.statistics()["blocks_decoded"] - before["blocks_decoded"] < 11


def test_bounded_residency(native, corpus_a, monkeypatch):
    """The compressed file is not kept on the GPU: every launch brings the packed windows of its own blocks."""
    c = corpus_a[33]
    monkeypatch.setenv("MI355X_BZ2_INPUT_BUDGET", "65536")
    for parallelization in (1, 3, 0):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            assert f.statistics()["input_resident"] == 0
            assert f.find_all(c["needle"]).tolist() == c["expected"]
            assert f.count_matches(c["needle"], 123_456, 876_543) == len(matches_of(c["raw"], c["needle"], 123_456, 876_543))
            assert f.statistics()["input_resident"] == 0 and f.statistics()["input_bytes_uploaded"] > 0


def test_damaged_block(native, corpus_a, tmp_path):
    """One byte flipped inside block 7: a search whose range keeps clear of that block is served, one that needs it fails
    with the block's status and bit offset, and the reader works afterwards.  (The damaged block may share a launch with
    clean ones: only what the calls return or raise is asserted.)"""
    c = corpus_a[16]
    raw, needle = c["raw"], c["needle"]
    items = sorted(c["blocks"].items())
    bits, next_bits, start, stop = [(b, nb, s, e) for (b, s), (nb, e) in zip(items, items[1:]) if e > s][7]
    assert (start, stop) == (7 * BLOCK, 8 * BLOCK)
    damaged = bytearray(open(c["path"], "rb").read())
    damaged[(bits + next_bits) // 16] ^= 0xFF
    bad = tmp_path / "damaged.bz2"
    bad.write_bytes(bytes(damaged))
    clean = [(17, start), (stop, SIZE), (2 * BLOCK + 5, 5 * BLOCK), (stop, ALL)]
    needing = [(0, ALL), (start - 1000, start + 1000), (stop - 300, stop + 300), (start + 500, start + 600)]

    def check_clean(f):
        for a, b in clean:
            want = matches_of(raw, needle, a, b)
            assert len(want) >= 2
            assert f.count_matches(needle, a, b) == len(want), (a, b)
            assert f.find_all(needle, a, b).tolist() == want, (a, b)

    with native.open(str(bad), parallelization=4) as f:
        f.set_block_offsets(c["blocks"])
        check_clean(f)
        for a, b in needing:
            for call in (f.count_matches, f.find_all):
                with pytest.raises(native.Bz2Error) as failure:
                    call(needle, a, b)
                assert failure.value.status != 0
                assert f"bit offset {bits}" in str(failure.value)
        # the reader stays usable
        check_clean(f)


# ------------------------------------------------------------------------------------------------ corpus B

def test_extents_shorter_than_the_pattern(native, tmp_path):
    parts = [b"ab", b"c", b"", b"abc", b"a", b"bca"] * 10
    raw = b"".join(parts)
    enc = b"".join(bz2.compress(p, 9) for p in parts)
    assert len(parts) == 60 and len(enc) < 3000
    path = tmp_path / "b.bz2"
    path.write_bytes(enc)
    for parallelization in (1, 0):
        with native.open(str(path), parallelization=parallelization) as f:
            for pattern in (b"abc", b"cabca", b"abcabcabca", raw[13:77]):
                want = matches_of(raw, pattern)
                assert len(want) >= 1
                assert f.count_matches(pattern) == len(want), pattern
                assert f.find_all(pattern).tolist() == want, pattern
                assert f.find(pattern) == want[0]
                for start, end in ((1, len(raw) - 1), (5, 40), (14, 77), (13, 76), (13, 77), (len(raw) - 4, ALL)):
                    assert f.find_all(pattern, start, end).tolist() == matches_of(raw, pattern, start, end), (pattern, start, end)
                for limit in (1, 2, 3):
                    assert f.find_all(pattern, limit=limit).tolist() == want[:limit]
            assert f.read() == raw


# ------------------------------------------------------------------------------------------------ fixtures

@pytest.mark.parametrize("m", [1, 16, 256])
def test_self_overlap_and_worst_case_verify(native, m):
    _, raw = read_fixture("zeros")
    assert raw == b"\0" * len(raw) and len(raw) > 256
    path = os.path.join(ROOT, "tests", "golden", "fixtures", "zeros.bz2")
    for parallelization in (1, 0):
        with native.open(path, parallelization=parallelization) as f:
            pattern = b"\0" * m
            assert f.count_matches(pattern) == len(raw) - m + 1
            assert f.find_all(pattern).tolist() == list(range(len(raw) - m + 1))
            assert f.find_all(pattern, 3, len(raw) - 2, limit=5).tolist() == [3, 4, 5, 6, 7]
            assert f.find(pattern) == 0
            assert f.count_matches(b"\1" * m) == 0 and f.find(b"\0" * (m - 1) + b"\1") == -1


def test_empty_and_one_byte(native):
    for parallelization in (1, 0):
        with native.open(os.path.join(ROOT, "tests", "golden", "fixtures", "empty.bz2"), parallelization=parallelization) as f:
            assert f.count_matches(b"a") == 0 and f.find(b"a") == -1 and f.find_all(b"ab").tolist() == []
            assert f.read() == b""
        _, raw = read_fixture("1B")
        with native.open(os.path.join(ROOT, "tests", "golden", "fixtures", "1B.bz2"), parallelization=parallelization) as f:
            assert f.count_matches(raw) == 1 and f.find(raw) == 0 and f.find_all(raw).tolist() == [0]
            assert f.count_matches(raw + raw) == 0 and f.find(raw + raw) == -1
            assert f.count_matches(bytes([raw[0] ^ 1])) == 0
            assert f.count_matches(raw, 1) == 0 and f.count_matches(raw, 0, 0) == 0
            assert f.read() == raw


# ------------------------------------------------------------------------------------------------ agreement, position

@pytest.fixture(scope="module")
def with_newlines(corpus_a, tmp_path_factory):
    data = np.frombuffer(corpus_a[5]["raw"], dtype=np.uint8).copy()
    r = datagen.rng(0x0A0A)
    data[np.unique(r.integers(0, SIZE, 9000))] = 10
    data[BLOCK - 1] = data[BLOCK] = data[3 * BLOCK] = 10      # around block boundaries
    raw = data.tobytes()
    path = tmp_path_factory.mktemp("search-nl") / "nl.bz2"
    path.write_bytes(bz2.compress(raw, 1))
    return str(path), raw


def test_agrees_with_the_line_functions(native, with_newlines):
    path, raw = with_newlines
    newlines = np.flatnonzero(np.frombuffer(raw, dtype=np.uint8) == 10)
    for parallelization in (1, 0):
        with native.open(path, parallelization=parallelization) as f:
            n = f.count_lines()
            assert f.count_matches(b"\n") == n == len(newlines)
            found = f.find_all(b"\n")
            assert found.tolist() == newlines.tolist()
            assert (found + 1).tolist() == f.line_starts(range(1, n + 1)).tolist()


def read_raw(reader, n):
    """n bytes (fewer at the end) from the unbuffered reader, whose position is the native reader's own."""
    out = bytearray()
    while len(out) < n:
        piece = bytearray(n - len(out))
        got = reader.readinto(piece)
        if not got:
            break
        out += piece[:got]
    return bytes(out)


def test_positionless_and_independent_of_held_lines(native, with_newlines, corpus_a):
    """In the middle of a sequential read of the unbuffered reader (the buffered one would have read this file whole)."""
    path, raw = with_newlines
    needle = corpus_a[5]["needle"]
    everywhere = matches_of(raw, needle)
    lib = native.lib()
    for parallelization in (1, 3, 0):
        with native.open(path, parallelization=parallelization) as f:
            reader = f.bz2reader
            state = lambda: (reader.tell(), lib.mi355x_bz2_reader_eof(reader._h))
            assert read_raw(reader, 150_000) == raw[:150_000]
            assert state() == (150_000, 0)
            want = matches_of(raw, needle, 100_000, 700_000)
            assert f.find_all(needle, 100_000, 700_000).tolist() == want and len(want) > 3
            assert f.count_matches(needle) == len(everywhere)
            assert f.find(needle, 900_000) == [p for p in everywhere if p >= 900_000][0]
            assert state() == (150_000, 0)
            assert read_raw(reader, 200_000) == raw[150_000:350_000]
            # held line ranges survive a search, and held matches survive a line call
            ranges = [(3, 2), (1000, 40), (7, 1)]
            sizes, total = reader._read_line_ranges(ranges, b"\n", False)
            assert reader._search(needle, 0, None, ALL) == len(everywhere)
            dst = ctypes.create_string_buffer(max(1, total))
            reader._check(lib.mi355x_bz2_reader_take_line_ranges(reader._h, dst, 0))
            assert total > 0 and dst.raw[:total] == b"".join(f.read_line_ranges(ranges))
            assert reader._search(needle, 0, None, 3) == 3
            assert f.count_lines() == len(matches_of(raw, b"\n"))
            out = (ctypes.c_uint64 * 3)()
            reader._check(lib.mi355x_bz2_reader_take_matches(reader._h, out, 3))
            assert list(out) == everywhere[:3]
            with pytest.raises(ValueError):      # taken: nothing is held any more
                reader._check(lib.mi355x_bz2_reader_take_matches(reader._h, out, 3))
            assert state() == (350_000, 0)
            assert read_raw(reader, SIZE) == raw[350_000:]
            assert state() == (SIZE, 1)
            assert f.find(needle) == everywhere[0] and state() == (SIZE, 1)
            assert read_raw(reader, 10) == b""
    with pytest.raises(ValueError):
        f.count_matches(needle)


# ------------------------------------------------------------------------------------------------ the kernels

def test_count_and_find_kernels(native, corpus_a):
    """Decoder.count_bytes / find_bytes over spans of one batch's output: every start alignment 0 to 16, sizes around
    four tiles, a span given twice, spans of size 0 and shorter than the pattern, a capacity below the matches."""
    c = corpus_a[256]
    offsets = sorted(bits for bits, start in c["blocks"].items() if start < SIZE)
    dec = native.Decoder(device=0)
    dec.set_input(open(c["path"], "rb").read())
    results, total = dec.decode_batch(offsets)
    out = dec.copy_output(0, total)
    assert total == SIZE and out == c["raw"]
    for m in LENGTHS + [1]:
        needle = c["master"][:m]
        for alignment in range(17):
            base = 4096 * 5 + alignment
            spans = [(base, 65536 + d) for d in (-m, -1, 0, 1, m)]
            spans += [spans[2], (base, 0), (base + 3, m - 1), (base, m), (BLOCK - 100 + alignment, 3 * BLOCK)]
            want = [[p for p in matches_of(out, needle, o, o + n)] for o, n in spans]
            counts = [len(w) for w in want]
            assert counts[2] >= 4 and counts[6] == 0 and counts[7] == 0
            assert dec.count_bytes(needle, spans) == counts, (m, alignment)
            positions, found = dec.find_bytes(needle, spans)
            assert found == counts and positions == [p for w in want for p in w], (m, alignment)
            short = sum(counts) // 2
            positions, found = dec.find_bytes(needle, spans, capacity=short)
            assert found == counts and positions == [p for w in want for p in w][:short], (m, alignment)
    # the whole output as one span: dozens of tiles; and nothing to do
    needle = c["master"][:4]
    want = matches_of(out, needle)
    assert dec.count_bytes(needle, [(0, total), (1, total - 1)]) == [len(want), len([p for p in want if p >= 1])]
    assert dec.find_bytes(needle, [(0, total)]) == (want, [len(want)])
    assert dec.find_bytes(needle, [(0, total)], capacity=0) == ([], [len(want)])
    assert dec.count_bytes(needle, []) == [] and dec.find_bytes(needle, []) == ([], [])
    # spans outside the output and pattern sizes 0 and 257 are refused
    for bad in ([(total - 10, 11)], [(total + 1, 0)], [(0, 10), (2**63, 2**63)]):
        with pytest.raises(native.Bz2Error) as failure:
            dec.count_bytes(needle, bad)
        assert failure.value.status == 103
        with pytest.raises(native.Bz2Error):
            dec.find_bytes(needle, bad, capacity=4)
    for bad in (b"", b"x" * 257):
        with pytest.raises(native.Bz2Error) as failure:
            dec.count_bytes(bad, [(0, 100)])
        assert failure.value.status == 103
    assert dec.count_bytes(needle, [(0, total)]) == [len(want)]
    dec.close()


# ------------------------------------------------------------------------------------------------ the tool

def test_count_matches_tool(native, corpus_a):
    c = corpus_a[17]
    needle = c["needle"]
    args = os.fsencode(CLI), b"--count-matches", needle, os.fsencode(c["path"])
    run = subprocess.run(args, capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"%d\n" % len(c["expected"])
    run = subprocess.run([CLI, "-P", "1", "--count-matches=" + chr(needle[0]) + chr(needle[1]), c["path"]],
                         capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"%d\n" % len(matches_of(c["raw"], needle[:2]))
    run = subprocess.run([CLI, "--count-matches", "x" * 257, c["path"]], capture_output=True, timeout=600)
    assert run.returncode != 0 and b"1 to 256" in run.stderr
