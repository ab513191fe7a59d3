"""Grep and line numbers on the GPU: the k_rank_byte kernel (Decoder.rank_byte), line_numbers, grep /
count_matching_lines / grep_to_tensor of the reader, and `ibzip2-mi355x --grep [--line-number]`.

The text (grepgen.py) has the shape of the line tests' corpus -- about 9.5 MB, 30 000 newlines, one 3.5 MB line, dozens of
level-1 blocks without a newline, an unterminated tail -- with a needle written over it at a line's first bytes, just in
front of a newline, twice in one line, in consecutive lines, in line 0, in the tail, inside the long line and across
block boundaries of the level-1 and the level-9 file.  It is used at level 1, at level 9 and as two streams (cut inside a
needle), at parallelization 0, 1 and 3.

Every expected value comes from the raw bytes: numpy.cumsum for ranks, numpy.searchsorted over the newline positions for
line numbers, a plain split for the lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, read_fixture
import datagen
import grepgen
from grepgen import NEEDLE, NL

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
TILE = 65536
VARIANTS = ["level1", "level9", "two-streams"]


def data_block_starts(block_index):
    items = sorted(block_index.items())
    return [s for (_, s), (_, e) in zip(items, items[1:]) if e > s]


def block_index_of(native, path):
    with native.open(path, parallelization=0) as f:
        return f.block_offsets()


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("grep")
    text = grepgen.make_text()
    assert 9_000_000 < len(text) < 10_000_000 and 25_000 < text.count(NL) < 35_000 and not text.endswith(NL)
    # where the blocks of the level-1 and the level-9 file start: a needle goes across three boundaries of each (bytes are
    # overwritten, nothing is inserted, so the boundaries stay where they are -- which is checked below)
    boundaries = []
    for level in (1, 9):
        path = folder / f"plain{level}.bz2"
        path.write_bytes(datagen.compress(text, level))
        starts = data_block_starts(block_index_of(native, str(path)))
        boundaries += [starts[1], starts[len(starts) // 2], starts[-1]]
    raw, places = grepgen.plant(text, boundaries)
    cut = places["consecutive"][0] + 3            # the two streams part inside a needle
    variants = {
        "level1": datagen.compress(raw, 1),
        "level9": datagen.compress(raw, 9),
        "two-streams": datagen.compress(raw[:cut], 9) + datagen.compress(raw[cut:], 5),
    }
    out = {"raw": raw, "places": places, "newlines": grepgen.newline_positions(raw)}
    for name, enc in variants.items():
        path = folder / (name + ".bz2")
        path.write_bytes(enc)
        blocks = block_index_of(native, str(path))
        starts = data_block_starts(blocks)
        # a needle lies across a block boundary of every variant
        assert any(p < s < p + len(NEEDLE) for s in starts for p in grepgen.matches_of(raw, NEEDLE)), name
        out[name] = {"path": str(path), "enc": enc, "blocks": blocks, "starts": starts}
    assert 80 <= len(out["level1"]["starts"]) <= 110 and 9 <= len(out["level9"]["starts"]) <= 13
    # dozens of level-1 blocks without any newline
    counts = np.diff(np.searchsorted(out["newlines"], out["level1"]["starts"] + [len(raw)]))
    assert int((counts == 0).sum()) >= 25
    return out


# ------------------------------------------------------------------------------------------------ the kernel

def rank_positions(offset, size):
    """Positions of [offset, offset + size] at which k_rank_byte can go wrong."""
    base = offset & ~15
    end = offset + size
    wanted = {offset, end}
    wanted.update(offset + r for r in range(17))                         # every residue behind the span's start
    for k in range(0, size // TILE + 2):                                 # both sides of every tile boundary
        wanted.update(offset + k * TILE + d for d in (-1, 0, 1))
    for step in (1, 2, 64, 65):                                          # both sides of 1-KiB step boundaries
        wanted.update(base + 1024 * step + d for d in (-1, 0, 1))
    wanted.update(range(base + 3 * 1024, base + 4 * 1024))               # a whole step: 1 024 queries, 64 at a time
    return sorted(p for p in wanted if offset <= p <= end)


def check_ranks(dec, data, value, queries):
    sums = np.concatenate([[0], np.cumsum(np.frombuffer(data, dtype=np.uint8) == value)])
    want = [int(sums[p] - sums[o]) for o, n, p in queries]
    assert dec.rank_byte(queries, value) == want


def test_rank_kernel(native):
    """300 000 seeded bytes at level 1 (four blocks whose spans start at odd offsets): a sparse delimiter and a value that
    does not occur; then the fixture `zeros`, where every byte counts."""
    r = datagen.rng(0x4A2C)
    data = r.integers(0, 255, 300_000, dtype=np.uint8)       # 255 does not occur
    data[r.integers(0, len(data), 1200)] = 10                # a sparse delimiter beside the 1 in 255 that chance gives
    data = data.tobytes()
    enc = datagen.compress(data, 1)
    dec = native.Decoder(device=0)
    dec.set_input(enc)
    results, total = dec.decode_batch(native.find_magic(enc))
    assert total == len(data) and dec.copy_output(0, total) == data and len(results) >= 3
    block = (results[1]["data_offset"], results[1]["decoded_size"])
    assert block[1] > TILE + 16
    spans = [(0, total), block, (block[0] + 5, TILE + 11), (7, 3 * TILE + 1)]
    assert any(o % 16 not in (0, 7) for o, _ in spans)
    for value in (10, 255, ord("e")):
        for offset, size in spans:
            positions = rank_positions(offset, size)
            queries = [(offset, size, p) for p in positions]
            check_ranks(dec, data, value, queries)
            check_ranks(dec, data, value, queries[::-1])                       # descending
        # several spans in one call, one of them named twice, in seeded order
        mixed = [(o, n, p) for o, n in spans + [block] for p in rank_positions(o, n)[::7]]
        check_ranks(dec, data, value, [mixed[i] for i in r.permutation(len(mixed))])
        # a tile whose only query is its last byte; alone, and with neighbours in other tiles
        lonely = (block[0], block[1], block[0] + TILE)
        check_ranks(dec, data, value, [lonely])
        check_ranks(dec, data, value, [(block[0], block[1], block[0] + 3), lonely, (block[0], block[1], block[0] + TILE + 9)])
        # spans of 0, 1 and 15 bytes at every alignment
        small = [(at + sm, n, at + sm + k) for at in (0, 4096, block[0]) for sm in range(16) for n in (0, 1, 15)
                 for k in range(n + 1)]
        check_ranks(dec, data, value, small)
    assert dec.rank_byte([(0, total, total)], 255) == [0]
    assert dec.rank_byte([(0, total, total)], 10) == [data.count(b"\n")]
    assert dec.rank_byte([], 10) == []
    # spans outside the output and positions outside their span are refused
    for bad in ((total - 10, 11, total - 5), (0, 100, 101), (50, 100, 49), (total + 1, 0, total + 1)):
        with pytest.raises(native.Bz2Error):
            dec.rank_byte([(0, 10, 5), bad], 10)
    dec.close()

    enc, zeros = read_fixture("zeros")
    dec = native.Decoder(device=0)
    dec.set_input(enc)
    _, total = dec.decode_batch(native.find_magic(enc))
    assert total == len(zeros) and set(zeros) == {0}
    for offset, size in ((0, total), (3, total - 3), (17, 600)):
        queries = [(offset, size, p) for p in range(offset, offset + size + 1)]
        assert dec.rank_byte(queries, 0) == [p - offset for _, _, p in queries]
        assert dec.rank_byte(queries, 1) == [0] * len(queries)
    dec.close()


# ------------------------------------------------------------------------------------------------ line numbers

def offsets_for(c, v, seed):
    raw, newlines = c["raw"], c["newlines"]
    size = len(raw)
    rng = np.random.default_rng(seed)
    offsets = []
    for start in v["starts"]:
        offsets += [start, max(start - 1, 0), start + 1]
    offsets += [int(p) for p in newlines[::50]] + [int(p) + 1 for p in newlines[::50]]
    offsets += [0, size - 1, size, size + 5, 2**64 - 1]
    offsets += [int(p) for p in rng.integers(0, size, 500)]
    window = int(newlines[1234]) - 2000
    offsets += list(range(window, window + 4096))                       # dense: thousands of queries in one tile
    offsets += offsets[100:130]                                          # duplicates
    return [offsets[i] for i in rng.permutation(len(offsets))]          # unsorted


@pytest.mark.parametrize("parallelization", [0, 1, 3])
@pytest.mark.parametrize("variant", VARIANTS)
def test_line_numbers(native, corpus, variant, parallelization):
    c, v = corpus, corpus[variant]
    raw = c["raw"]
    offsets = offsets_for(c, v, 0x11 + parallelization)
    want = grepgen.line_numbers_of(raw, offsets)
    with native.open(v["path"], parallelization=parallelization) as f:
        f.set_block_offsets(v["blocks"])
        f.seek(4321)
        got = f.line_numbers(offsets)
        assert got.dtype == np.uint64 and got.shape == (len(offsets),)
        assert np.array_equal(got, want)
        # a numpy array goes in as it is; ascending order gives the same numbers
        ascending = np.sort(np.array(offsets, dtype=np.uint64))
        assert np.array_equal(f.line_numbers(ascending), grepgen.line_numbers_of(raw, ascending))
        # the inverse of line_starts: s(L(p)) <= p < s(L(p) + 1), with the size behind the last line
        inside = np.array([p for p in offsets[:1500] if p < len(raw)], dtype=np.uint64)
        numbers = f.line_numbers(inside)
        lower, upper = f.line_starts(numbers), f.line_starts(numbers + np.uint64(1))
        assert np.all(lower <= inside) and np.all(inside < upper)
        starts = f.line_starts([0, 1, 77, len(c["newlines"])])
        assert np.array_equal(f.line_numbers(starts), np.array([0, 1, 77, len(c["newlines"])], dtype=np.uint64))
        assert len(f.line_numbers([])) == 0
        # positionless
        assert f.tell() == 4321 and f.read(1000) == raw[4321:5321]


def test_line_numbers_decode_only_the_blocks_they_need(native, corpus):
    c, v = corpus, corpus["level1"]
    starts = v["starts"]
    with native.open(v["path"], parallelization=0) as f:
        f.set_block_offsets(v["blocks"])
        f.line_offsets()
        before = f.statistics()
        # block starts, the size and beyond: the index answers
        fixed = starts + [len(c["raw"]), len(c["raw"]) + 9]
        assert np.array_equal(f.line_numbers(fixed), grepgen.line_numbers_of(c["raw"], fixed))
        assert f.statistics()["blocks_decoded"] == before["blocks_decoded"]
        # thousands of offsets in three blocks: three blocks, one launch
        offsets = [starts[b] + k for b in (2, 3, 40) for k in range(1, 3000)]
        assert np.array_equal(f.line_numbers(offsets), grepgen.line_numbers_of(c["raw"], offsets))
        after = f.statistics()
        assert after["blocks_decoded"] - before["blocks_decoded"] == 3 and after["batches"] - before["batches"] == 1


def test_line_numbers_with_another_delimiter(native, corpus):
    c, v = corpus, corpus["level9"]
    offsets = offsets_for(c, v, 0x77)[:2000]
    with native.open(v["path"], parallelization=3) as f:
        for nl in (b"e", b"\x00", b"~"):
            assert np.array_equal(f.line_numbers(offsets, newline=nl), grepgen.line_numbers_of(c["raw"], offsets, nl))
        assert np.array_equal(f.line_numbers(offsets), grepgen.line_numbers_of(c["raw"], offsets))


def test_tiny_files(native):
    fixtures = os.path.join(ROOT, "tests", "golden", "fixtures")
    for name in ("empty", "1B"):
        _, raw = read_fixture(name)
        for nl in (NL, raw[:1] or b"x"):
            with native.open(os.path.join(fixtures, name + ".bz2"), parallelization=0) as f:
                offsets = [0, 1, 2, 7, 2**64 - 1]
                assert np.array_equal(f.line_numbers(offsets, newline=nl), grepgen.line_numbers_of(raw, offsets, nl))
                for pattern in (b"a", raw[:1] or b"b", nl):
                    numbers, lines = f.grep(pattern, newline=nl)
                    want_numbers, want_lines = grepgen.grep_of(raw, pattern, nl=nl)
                    assert np.array_equal(numbers, want_numbers) and lines == want_lines
                    assert f.count_matching_lines(pattern, newline=nl) == len(want_lines)


def test_lying_line_index(native, corpus):
    """An imported line index with one count raised by 1 fails line_numbers for an offset in that block; offsets in
    blocks the lie does not touch are served, and so is everything once the true index is back."""
    c, v = corpus, corpus["level9"]
    raw, starts = c["raw"], v["starts"]
    with native.open(v["path"], parallelization=4) as f:
        f.set_block_offsets(v["blocks"])
        true_index = f.line_offsets()
        b = 2
        lying = dict(true_index)
        lying[starts[b + 1]] += 1                      # block b gets one more, block b + 1 one fewer
        f.set_line_offsets(lying)
        with pytest.raises(native.Bz2Error) as failure:
            f.line_numbers([5, starts[b] + 10])
        assert failure.value.status == 106 and "line index" in str(failure.value)
        with pytest.raises(native.Bz2Error):
            f.grep(raw[starts[b] + 100:starts[b] + 110])
        untouched = [5, starts[1] - 1, starts[b], starts[5] + 7]
        assert np.array_equal(f.line_numbers(untouched), grepgen.line_numbers_of(raw, untouched))
        f.set_line_offsets(true_index)
        offsets = [5, starts[b] + 10, starts[b + 1] + 10]
        assert np.array_equal(f.line_numbers(offsets), grepgen.line_numbers_of(raw, offsets))
        assert f.read(1000) == raw[:1000]


def test_damaged_block(native, corpus, tmp_path):
    """One byte flipped inside block b, both true indexes imported: line_numbers of offsets that keep clear of the block
    is served, an offset in its middle fails with the block's status and bit offset; grep over the block fails the same
    way and holds nothing afterwards; a grep that keeps clear of the block is served before and after."""
    c, v = corpus, corpus["level9"]
    raw, starts, newlines = c["raw"], v["starts"], c["newlines"]
    b = len(starts) - 3
    items = sorted(v["blocks"].items())
    bits, next_bits, start, stop = [(x, nx, s, e) for (x, s), (nx, e) in zip(items, items[1:]) if e > s][b]
    assert (start, stop) == (starts[b], starts[b + 1])
    damaged = bytearray(v["enc"])
    damaged[(bits + next_bits) // 16] ^= 0xFF
    bad = tmp_path / "damaged.bz2"
    bad.write_bytes(bytes(damaged))
    line_index = {s: int(np.searchsorted(newlines, s)) for s in starts}
    line_index[len(raw)] = len(newlines)
    lib = native.lib()
    with native.open(str(bad), parallelization=4) as f:
        f.set_block_offsets(v["blocks"])
        f.set_line_offsets(line_index)
        # the damaged block's first byte is answered by the index, its neighbours' bytes by their own blocks
        avoiding = [5, starts[1] - 1, start, start - 1, stop, stop + 7, starts[2] + 10, len(raw) - 1, len(raw) + 3]
        assert np.array_equal(f.line_numbers(avoiding), grepgen.line_numbers_of(raw, avoiding))
        with pytest.raises(native.Bz2Error) as failure:
            f.line_numbers([5, (start + stop) // 2])
        assert failure.value.status != 0
        assert f"bit offset {bits}" in str(failure.value)
        assert np.array_equal(f.line_numbers(avoiding), grepgen.line_numbers_of(raw, avoiding))
        # a grep that keeps clear of the block is served (and its lines are taken)
        numbers, _ = assert_grep(f, raw, NEEDLE, 0, starts[1])
        assert len(numbers) >= 1
        reader = f.bz2reader
        for window in ((0, None), (start + 10, stop - 10)):
            with pytest.raises(native.Bz2Error) as failure:
                f.grep(NEEDLE, *window)
            assert failure.value.status != 0
            assert f"bit offset {bits}" in str(failure.value)
            with pytest.raises(ValueError, match="no line ranges are held"):
                reader._check(lib.mi355x_bz2_reader_take_line_ranges(reader._h, None, 0))
            assert lib.mi355x_bz2_reader_take_grep(reader._h, None, None, 0) == 103
        assert_grep(f, raw, NEEDLE, 0, starts[1])


# ------------------------------------------------------------------------------------------------ grep

def assert_grep(f, raw, pattern, start=0, end=None, limit=None):
    numbers, lines = f.grep(pattern, start, end, limit)
    want_numbers, want_lines = grepgen.grep_of(raw, pattern, start, end, limit)
    assert numbers.dtype == np.uint64 and np.array_equal(numbers, want_numbers)
    assert np.all(np.diff(numbers.astype(np.int64)) > 0)
    assert lines == want_lines
    return numbers, lines


@pytest.mark.parametrize("parallelization", [0, 1, 3])
@pytest.mark.parametrize("variant", VARIANTS)
def test_grep_planted_needle(native, corpus, variant, parallelization):
    c, v = corpus, corpus[variant]
    raw, places = c["raw"], c["places"]
    planted = sorted(p for offsets in places.values() for p in offsets)
    assert grepgen.matches_of(raw, NEEDLE) == planted
    with native.open(v["path"], parallelization=parallelization) as f:
        f.set_block_offsets(v["blocks"])
        f.seek(999)
        numbers, lines = assert_grep(f, raw, NEEDLE)
        # line 0, the tail, the long line, and one line for the two needles of "twice"
        assert numbers[0] == 0 and numbers[-1] == len(c["newlines"]) and not lines[-1].endswith(NL)
        assert max(len(line) for line in lines) == grepgen.LONG_LINE
        assert any(line.startswith(NEEDLE) for line in lines[1:]) and any(line.endswith(NEEDLE + NL) for line in lines)
        assert any(line.count(NEEDLE) == 2 for line in lines[:-2])                           # twice in one line, once reported
        assert any(b - a == 1 for a, b in zip(numbers.tolist(), numbers.tolist()[1:]))      # consecutive lines
        for limit in (1, 2):
            assert_grep(f, raw, NEEDLE, limit=limit)
        assert f.count_matching_lines(NEEDLE) == len(numbers)
        # start and end bound the matches, not the lines: windows that cut through matching lines and needles
        twice = places["twice"]
        for start, end in ((twice[0] + 1, None), (twice[1], twice[1] + len(NEEDLE)), (twice[1], twice[1] + len(NEEDLE) - 1),
                           (0, twice[0] + len(NEEDLE)), (places["long-line"][0] - 10, places["long-line"][0] + 100),
                           (places["tail"][0], 2**64 - 1), (places["tail"][0] + 1, None), (len(raw), None), (9, 3)):
            assert_grep(f, raw, NEEDLE, start, end)
            want = len(grepgen.grep_of(raw, NEEDLE, start, end)[0])
            assert f.count_matching_lines(NEEDLE, start, end) == want
        assert_grep(f, raw, b"no such string anywhere")
        assert f.count_matching_lines(b"no such string anywhere") == 0
        # positionless
        assert f.tell() == 999 and f.read(1000) == raw[999:1999]


def test_grep_needles_with_a_newline_and_frequent_ones(native, corpus):
    c, v = corpus, corpus["level1"]
    raw, newlines = c["raw"], c["newlines"]
    q = int(newlines[100])
    with native.open(v["path"], parallelization=0) as f:
        for pattern in (raw[q - 3:q + 3], raw[q:q + 4], raw[q - 4:q + 1], NL, b"\n\n"):
            numbers, _ = assert_grep(f, raw, pattern)
            assert len(numbers) >= 1
            assert f.count_matching_lines(pattern) == len(numbers)
        # a match belongs to the line of its first byte: the newline that ends line 100 belongs to line 100
        numbers, lines = f.grep(raw[q:q + 4])
        assert 100 in numbers.tolist()
        # thousands of matches per tile, most lines match, the result is most of the file
        numbers, lines = assert_grep(f, raw, b"e")
        assert len(numbers) > 20_000 and sum(map(len, lines)) > 8_000_000
        assert_grep(f, raw, b"e ", limit=100)
        assert f.count_matching_lines(b"e ") == len(grepgen.grep_of(raw, b"e ")[0])
        # another delimiter
        for nl in (b"e", b"~"):
            numbers, lines = f.grep(NEEDLE, newline=nl)
            want_numbers, want_lines = grepgen.grep_of(raw, NEEDLE, nl=nl)
            assert np.array_equal(numbers, want_numbers) and lines == want_lines


def test_grep_releases_what_earlier_calls_held(native, corpus):
    c, v = corpus, corpus["level9"]
    lib = native.lib()
    with native.open(v["path"], parallelization=0) as f:
        reader = f.bz2reader
        assert reader._search(NEEDLE, 0, None, 2**64 - 1) > 0            # matches are held ...
        reader._read_line_ranges([(0, 2)], NL, False)                    # ... and line ranges
        assert f.count_matching_lines(NEEDLE) > 0
        assert lib.mi355x_bz2_reader_take_matches(reader._h, None, 0) == 103
        assert lib.mi355x_bz2_reader_take_line_ranges(reader._h, None, 0) == 103
        assert lib.mi355x_bz2_reader_take_grep(reader._h, None, None, 0) == 103
        # the bytes of a grep are taken once
        assert_grep(f, c["raw"], NEEDLE, limit=3)
        assert lib.mi355x_bz2_reader_take_grep(reader._h, None, None, 0) == 103
        assert lib.mi355x_bz2_reader_take_line_ranges(reader._h, None, 0) == 103
        assert f.find_all(NEEDLE).tolist() == grepgen.matches_of(c["raw"], NEEDLE)


def test_grep_without_a_match_builds_no_line_index(native, corpus):
    """No match, or an empty window: the search pass alone -- every block once -- also on a reader that holds no line index
    yet; the empty result can be taken like any other."""
    v = corpus["level1"]
    lib = native.lib()
    with native.open(v["path"], parallelization=0) as f:
        f.set_block_offsets(v["blocks"])
        before = f.statistics()["blocks_decoded"]
        numbers, lines = f.grep(b"no such string anywhere")
        assert len(numbers) == 0 and lines == []
        assert f.count_matching_lines(b"no such string anywhere") == 0
        assert f.statistics()["blocks_decoded"] - before == 2 * len(v["starts"])
        numbers, lines = f.grep(NEEDLE, 500, 500)
        assert len(numbers) == 0 and lines == [] and f.count_matching_lines(NEEDLE, 9, 3) == 0
        assert f.statistics()["blocks_decoded"] - before == 2 * len(v["starts"])
        # held, empty; taken once
        reader = f.bz2reader
        assert reader._grep(b"no such string anywhere", 0, None, 5, NL, False)[2] == 0
        assert lib.mi355x_bz2_reader_take_line_ranges(reader._h, None, 0) == 0
        assert lib.mi355x_bz2_reader_take_grep(reader._h, None, None, 0) == 103


def test_grep_tool(native, corpus):
    raw = corpus["raw"]
    for name, pattern in (("level9", NEEDLE), ("two-streams", NEEDLE), ("level1", b"e ")):
        numbers, lines = grepgen.grep_of(raw, pattern)
        run = subprocess.run([CLI, "--grep", pattern.decode(), corpus[name]["path"]], capture_output=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        assert run.stdout == b"".join(lines)
        run = subprocess.run([CLI, "--grep=" + pattern.decode(), "--line-number", "-P", "3", corpus[name]["path"]],
                             capture_output=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        assert run.stdout == b"".join(b"%d:" % (k + 1) + line for k, line in zip(numbers.tolist(), lines))
    # no line matches: nothing is written, and the status is 0 all the same; a pattern that is too long is an error
    run = subprocess.run([CLI, "--grep", "no such string anywhere", corpus["level9"]["path"]], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b""
    run = subprocess.run([CLI, "--grep", "x" * 257, corpus["level9"]["path"]], capture_output=True, timeout=600)
    assert run.returncode == 1 and run.stdout == b""


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import indexed_bzip2_amd as m
import grepgen

path, raw = sys.argv[2], open(sys.argv[3], "rb").read()
for parallelization in (0, 3):
    with m.open(path, parallelization=parallelization) as f:
        for pattern, limit in ((grepgen.NEEDLE, None), (grepgen.NEEDLE, 2), (b"e ", 300), (b"no such string anywhere", None),
                               (grepgen.NEEDLE, 0)):
            numbers, data, offsets = f.grep_to_tensor(pattern, limit=limit)
            want_numbers, want_lines = f.grep(pattern, limit=limit)
            plain_numbers, plain_lines = grepgen.grep_of(raw, pattern, limit=limit)
            assert np.array_equal(want_numbers, plain_numbers) and want_lines == plain_lines
            assert numbers.dtype == np.uint64 and np.array_equal(numbers, want_numbers)
            assert data.dtype == torch.uint8 and data.is_cuda and data.dim() == 1
            assert offsets.dtype == torch.int64 and not offsets.is_cuda and offsets.numel() == len(want_lines) + 1
            bounds = [0]
            for line in want_lines:
                bounds.append(bounds[-1] + len(line))
            assert offsets.tolist() == bounds and data.numel() == bounds[-1]
            assert bytes(data.cpu().numpy()) == b"".join(want_lines)
        assert f.tell() == 0
        assert f.read(4096) == raw[:4096]
print("device grep ok")
"""


def test_grep_to_tensor(native, corpus, tmp_path):
    raw_path = tmp_path / "raw"
    raw_path.write_bytes(corpus["raw"])
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, corpus["level1"]["path"], str(raw_path)], capture_output=True,
                         text=True, timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "device grep ok" in run.stdout
