"""Search for a SET of byte strings on the GPU, one decode per call: count_matches_each / find_all_any / find_any / grep_any
of the reader, the k_count_set / k_emit_set kernels under them (Decoder.count_bytes_set, Decoder.find_bytes_set) and
`ibzip2-mi355x --grep-file / --count-matches-file`.

The corpora are those of test_gpu_search.py (its helpers are imported, not its fixtures): corpus A, 1 000 000 seeded
printable bytes without equal neighbours at bz2 level 1 -- 10 blocks of 99 981 bytes and one of 190 --, in the copy that
holds the 256-byte needle, whose prefixes of the lengths LENGTHS are the other needles: every plant gives up to ten pairs
at one position.  Corpus B: 60 streams of 0 to 3 bytes.

Every expected value comes from the raw bytes: matches_of per pattern (a raw.find(P, p + 1) loop), the union sorted by
(position, index in the set)."""
import bz2
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, read_fixture
import datagen
import grepgen
from test_gpu_search import ALL, BLOCK, LENGTHS, SIZE, make_corpus_a, matches_of, no_equal_neighbours

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")


def pairs_of(raw, patterns, start=0, end=None):
    """Every (p, i) with raw[p:p + m_i] == patterns[i], start <= p and p + m_i <= end (clipped), by (p, i)."""
    return sorted((p, i) for i, pattern in enumerate(patterns) for p in matches_of(raw, bytes(pattern), start, end))


def as_pairs(result):
    positions, ids = result
    assert positions.dtype == np.uint64 and ids.dtype == np.uint32 and len(positions) == len(ids)
    return list(zip(positions.tolist(), ids.tolist()))


def block_offsets_of(native, path):
    with native.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
    assert sorted(set(blocks.values())) == [k * BLOCK for k in range(11)] + [SIZE]
    return blocks


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    """The copy of corpus A for m = 256, the prefix chain as a set, and its expected pairs."""
    r = datagen.rng(0x5EA2C4)
    base = no_equal_neighbours(r, SIZE)
    master = no_equal_neighbours(r, 256)
    raw, needle, plants = make_corpus_a(256, master, base)
    path = tmp_path_factory.mktemp("search-set") / "a256.bz2"
    path.write_bytes(bz2.compress(raw, 1))
    chain = [needle[:m] for m in LENGTHS]
    expected = pairs_of(raw, chain)
    boundaries = [k * BLOCK for k in range(1, 11)]
    # up to ten pairs at one plant, in id order; straddled block boundaries; a pattern that ends exactly on one
    assert all([(p, i) for i in range(10)] == [pair for pair in expected if pair[0] == p] for p in plants[:5])
    assert sum(1 for p, i in expected if any(p < b < p + LENGTHS[i] for b in boundaries)) >= 30
    assert any(p + LENGTHS[i] == b for p, i in expected for b in boundaries)
    return {"path": str(path), "raw": raw, "master": needle, "plants": plants, "chain": chain, "expected": expected,
            "blocks": block_offsets_of(native, str(path)), "base": base}


def chain_ranges(c):
    """About 30 (start, end): ends that cut between p + m_min and p + m_max of a plant (at a block boundary and inside a
    block), starts inside a plant, empty and clipped ranges, and seeded ones from a few bytes to several blocks."""
    r = np.random.default_rng(0x5E7)
    straddling = [p for p in c["plants"] if any(p < b < p + 256 for b in (k * BLOCK for k in range(1, 11)))]
    ranges = [(0, ALL), (SIZE - 300, ALL), (SIZE, ALL), (5000, 4000), (1234, 1235), (1234, 1236)]
    for p in (straddling[0], straddling[3], c["plants"][-1]):
        ranges += [(p, p + 2), (p, p + 3), (p - 7, p + 16), (p, p + 17), (p - 1, p + 255), (p, p + 256), (p + 1, p + 300),
                   (0 if p < 2 * BLOCK else p - 2 * BLOCK, p + 100)]
    while len(ranges) < 34:
        start = int(r.integers(0, SIZE))
        size = int(r.integers(0, 300)) if len(ranges) % 2 else int(r.integers(BLOCK, 4 * BLOCK))
        ranges.append((start, start + size))
    return ranges


# ------------------------------------------------------------------------------------------------ 1: the prefix chain

@pytest.mark.parametrize("parallelization", [1, 3, 0])
def test_prefix_chain_at_seams(native, corpus, parallelization):
    c = corpus
    raw, chain, expected = c["raw"], c["chain"], c["expected"]
    with native.open(c["path"], parallelization=parallelization) as f:
        if parallelization != 3:
            f.set_block_offsets(c["blocks"])          # at 3 the file is indexed by the search itself
        f.seek(4321)
        each = f.count_matches_each(chain)
        assert each.dtype == np.uint64
        assert each.tolist() == [len(matches_of(raw, pattern)) for pattern in chain]
        assert as_pairs(f.find_all_any(chain)) == expected
        assert f.find_any(chain) == expected[0]
        for start, end in chain_ranges(c):
            want = pairs_of(raw, chain, start, end)
            assert as_pairs(f.find_all_any(chain, start, end)) == want, (start, end)
            assert f.find_any(chain, start, end) == (want[0] if want else (-1, -1)), (start, end)
        start, end = c["plants"][7] - 3, c["plants"][7] + 33
        want = pairs_of(raw, chain, start, end)
        assert [i for _, i in want if _ == c["plants"][7]] == list(range(8))      # the needles of up to 33 bytes fit
        assert f.count_matches_each(chain, start, end).tolist() == [sum(1 for _, i in want if i == k) for k in range(10)]
        assert as_pairs(f.find_all_any(chain, limit=0)) == []
        # bytes-like elements, any sequence
        assert f.count_matches_each(tuple(bytearray(p) for p in chain)).tolist() == each.tolist()
        assert f.tell() == 4321
        assert f.read(1000) == raw[4321:5321]


# ------------------------------------------------------------------------------------------------ 2: the limit

def test_limit_is_a_prefix(native, corpus, tmp_path):
    """A long pattern crosses a launch seam from BLOCK - 100 while a short one matches inside the front at BLOCK - 50: the
    pair of the long one sorts in front, and only the launch behind the seam shows it."""
    r = datagen.rng(0x11417)
    long = no_equal_neighbours(r, 200).tobytes()
    short = long[50:52]
    data = corpus["base"].copy()
    data[BLOCK - 100:BLOCK + 100] = np.frombuffer(long, dtype=np.uint8)
    raw = data.tobytes()
    path = tmp_path / "limit.bz2"
    path.write_bytes(bz2.compress(raw, 1))
    blocks = block_offsets_of(native, str(path))
    for patterns in ((long, short), (short, long)):
        everything = pairs_of(raw, patterns)                 # `short` also matches where chance puts it
        total = len(everything)
        crossing = (BLOCK - 100, patterns.index(long))
        rank = everything.index(crossing)
        assert everything[rank + 1] == (BLOCK - 50, patterns.index(short)) and 3 < rank and total > rank + 10
        limits = sorted(set(range(max(1, rank - 8), rank + 10)) | {1, 2, total - 1, total, total + 1}
                        | {int(k) for k in np.random.default_rng(7).integers(1, total + 1, 6)})
        with native.open(str(path), parallelization=1) as f:     # every block boundary is a launch seam
            f.set_block_offsets(blocks)
            assert as_pairs(f.find_all_any(patterns)) == everything
            for limit in limits:
                assert as_pairs(f.find_all_any(patterns, limit=limit)) == everything[:limit], limit
            assert f.find_any(patterns, BLOCK - 100) == crossing
            # with a start: the first pairs of the range
            assert as_pairs(f.find_all_any(patterns, BLOCK - 120, limit=2)) == pairs_of(raw, patterns, BLOCK - 120)[:2]


# ------------------------------------------------------------------------------------------------ 3: one decode

def test_one_decode_per_call_whatever_k(native, corpus):
    c = corpus
    raw = c["raw"]
    r = np.random.default_rng(0x64)
    patterns = [raw[p:p + 8] for p in r.integers(0, SIZE - 8, 64).tolist()]
    for parallelization, cap in ((1, 1), (0, 512)):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            before = f.statistics()
            assert f.count_matches_each(patterns).tolist() == [len(matches_of(raw, p)) for p in patterns]
            after = f.statistics()
            assert after["blocks_decoded"] - before["blocks_decoded"] == 11
            assert after["batches"] - before["batches"] == -(-11 // cap)
            # blocks 2 to 5 intersect this range
            start, end = 2 * BLOCK + 17, 5 * BLOCK + 1
            assert as_pairs(f.find_all_any(patterns, start, end)) == pairs_of(raw, patterns, start, end)
            assert f.statistics()["blocks_decoded"] - after["blocks_decoded"] == 4


# ------------------------------------------------------------------------------------------------ 4: short extents

def test_extents_shorter_than_the_patterns(native, tmp_path):
    parts = [b"ab", b"c", b"", b"abc", b"a", b"bca"] * 10
    raw = b"".join(parts)
    path = tmp_path / "b.bz2"
    path.write_bytes(b"".join(bz2.compress(p, 9) for p in parts))
    sets = ([b"a", b"abc", b"cabca", raw[13:77]], [raw[13:77], b"cabca", b"abc", b"a"], [b"abc"], [b"cabca", b"a", b"cabca"])
    for parallelization in (1, 0):
        with native.open(str(path), parallelization=parallelization) as f:
            for patterns in sets:
                want = pairs_of(raw, patterns)
                assert len(want) >= 10
                assert f.count_matches_each(patterns).tolist() == [len(matches_of(raw, p)) for p in patterns]
                assert as_pairs(f.find_all_any(patterns)) == want, patterns
                assert f.find_any(patterns) == want[0]
                for start, end in ((1, len(raw) - 1), (5, 40), (14, 77), (13, 76), (13, 77), (len(raw) - 4, ALL)):
                    assert as_pairs(f.find_all_any(patterns, start, end)) == pairs_of(raw, patterns, start, end), (patterns, start, end)
                for limit in (1, 2, 3, 7, len(want) - 1):
                    assert as_pairs(f.find_all_any(patterns, limit=limit)) == want[:limit], (patterns, limit)
            assert f.read() == raw


def test_self_overlap_and_equal_patterns(native):
    _, raw = read_fixture("zeros")
    assert raw == b"\0" * len(raw) and len(raw) > 256
    path = os.path.join(ROOT, "tests", "golden", "fixtures", "zeros.bz2")
    n = len(raw)
    patterns = (b"\0", b"\0" * 16, b"\0" * 256, b"\1")
    for parallelization in (1, 0):
        with native.open(path, parallelization=parallelization) as f:
            assert f.count_matches_each(patterns).tolist() == [n, n - 15, n - 255, 0]
            want = pairs_of(raw, patterns)
            assert want[:3] == [(0, 0), (0, 1), (0, 2)] and len(want) == 3 * n - 270
            assert as_pairs(f.find_all_any(patterns)) == want
            assert as_pairs(f.find_all_any(patterns, 3, n - 2, limit=5)) == [(3, 0), (3, 1), (3, 2), (4, 0), (4, 1)]
            assert as_pairs(f.find_all_any(patterns, n - 20, n - 2)) == pairs_of(raw, patterns, n - 20, n - 2)
            assert f.find_any(patterns) == (0, 0) and f.find_any([b"\1", b"\0\1"]) == (-1, -1)
            # equal patterns report twice
            twice = (b"\0" * 16, b"\0", b"\0" * 16)
            assert f.count_matches_each(twice).tolist() == [n - 15, n, n - 15]
            assert as_pairs(f.find_all_any(twice, 0, 40)) == pairs_of(raw, twice, 0, 40)


def test_empty_and_one_byte(native):
    for parallelization in (1, 0):
        with native.open(os.path.join(ROOT, "tests", "golden", "fixtures", "empty.bz2"), parallelization=parallelization) as f:
            assert f.count_matches_each([b"a", b"ab"]).tolist() == [0, 0] and f.find_any([b"a"]) == (-1, -1)
            assert as_pairs(f.find_all_any([b"ab", b"a"])) == []
            assert f.read() == b""
        _, raw = read_fixture("1B")
        with native.open(os.path.join(ROOT, "tests", "golden", "fixtures", "1B.bz2"), parallelization=parallelization) as f:
            patterns = [raw + raw, raw, bytes([raw[0] ^ 1]), raw]
            assert f.count_matches_each(patterns).tolist() == [0, 1, 0, 1]
            assert as_pairs(f.find_all_any(patterns)) == [(0, 1), (0, 3)] and f.find_any(patterns) == (0, 1)
            assert f.count_matches_each(patterns, 1).tolist() == [0, 0, 0, 0]
            assert f.count_matches_each(patterns, 0, 0).tolist() == [0, 0, 0, 0]
            assert f.read() == raw


# ------------------------------------------------------------------------------------------------ 5: the kernels

def test_count_and_emit_kernels(native, corpus):
    c = corpus
    chain = c["chain"]
    offsets = sorted(bits for bits, start in c["blocks"].items() if start < SIZE)
    dec = native.Decoder(device=0)
    dec.set_input(open(c["path"], "rb").read())
    results, total = dec.decode_batch(offsets)
    out = dec.copy_output(0, total)
    assert total == SIZE and out == c["raw"]

    def check(patterns, spans, capacities=()):
        want = [pairs_of(out, patterns, o, o + n) for o, n in spans]
        counts = [len(w) for w in want]
        flat = [pair for w in want for pair in w]
        each = [sum(1 for _, i in flat if i == k) for k in range(len(patterns))]
        assert dec.count_bytes_set(patterns, spans) == (counts, each)
        positions, ids, found = dec.find_bytes_set(patterns, spans)
        assert found == counts and list(zip(positions, ids)) == flat
        for capacity in capacities:
            positions, ids, found = dec.find_bytes_set(patterns, spans, capacity=capacity)
            assert found == counts and list(zip(positions, ids)) == flat[:capacity], capacity
        return counts

    # every start alignment; sizes around four tiles, -+ m_min and -+ m_max; the same span twice; size 0, shorter than
    # m_min, between m_min and m_max; across a block boundary
    plant = next(p for p in c["plants"] if p > 4096 * 6)
    for alignment in range(17):
        base = 4096 * 5 + alignment
        spans = [(base, 65536 + d) for d in (-256, -2, -1, 0, 1, 2, 256)]
        spans += [spans[3], (base, 0), (base + 3, 1), (base, 2), (plant - alignment % 3, 100), (BLOCK - 100 + alignment, 2 * BLOCK)]
        counts = check(chain, spans, capacities=(0, 5) if alignment % 4 else (0, 1, 37))
        assert counts[3] >= 40 and counts[8] == 0 and counts[9] == 0
        assert 0 < counts[11] < 10                     # only the needles of at most 100 bytes fit
    # the whole output as one span; nothing to do
    whole = check(chain, [(0, total), (1, total - 1)], capacities=(len(c["expected"]) // 2,))
    assert whole[0] == len(c["expected"])
    assert dec.count_bytes_set(chain, []) == ([], [0] * 10) and dec.find_bytes_set(chain, []) == ([], [], [])
    # k = 1: the positions of find_bytes
    for m in (1, 2, 17, 256):
        needle = c["master"][:m]
        spans = [(7, 300_000), (BLOCK - 5, 70_000)]
        positions, ids, found = dec.find_bytes_set([needle], spans)
        assert (positions, found) == dec.find_bytes(needle, spans) and ids == [0] * len(positions) and len(positions) > 10
    # k = 1 024 patterns of 16 bytes cut from the corpus: the limits of a set, both reached
    r = np.random.default_rng(0x400)
    cuts = [out[p:p + 16] for p in r.integers(0, 300_000, 1024).tolist()]
    counts = check(cuts, [(0, 300_016), (150_001, 33_333)])
    assert counts[0] >= 1024
    # all 256 first bytes occur in the set: the printable ones with a second byte from the text
    firsts = [out[out.index(bytes([b])):out.index(bytes([b])) + 2] if 32 <= b < 127 else bytes([b, 65]) for b in range(256)]
    assert sorted(p[0] for p in firsts) == list(range(256))
    counts = check(firsts[::-1], [(11, 200_000)], capacities=(1000,))
    assert counts[0] > 1000
    # refused: spans outside the output, a batch's limits of a set
    for bad in ([(total - 10, 11)], [(total + 1, 0)], [(0, 10), (2**63, 2**63)]):
        with pytest.raises(native.Bz2Error) as failure:
            dec.count_bytes_set(chain, bad)
        assert failure.value.status == 103
        with pytest.raises(native.Bz2Error) as failure:
            dec.find_bytes_set(chain, bad, capacity=4)
        assert failure.value.status == 103
    for bad in ([], [b"a"] * 1025, [b"ab", b""], [b"x" * 257], [b"x" * 256] * 64 + [b"y"]):
        for call in (dec.count_bytes_set, lambda patterns, spans: dec.find_bytes_set(patterns, spans, capacity=4)):
            with pytest.raises(native.Bz2Error) as failure:
                call(bad, [(0, 100)])
            assert failure.value.status == 103
    assert dec.count_bytes_set(chain, [(0, total)])[0] == [len(c["expected"])]
    dec.close()


# ------------------------------------------------------------------------------------------------ 6 and 7: grep, the tool

@pytest.fixture(scope="module")
def with_newlines(corpus, tmp_path_factory):
    data = np.frombuffer(corpus["raw"], dtype=np.uint8).copy()
    r = datagen.rng(0x0A0A)
    data[np.unique(r.integers(0, SIZE, 9000))] = 10
    data[BLOCK - 1] = data[BLOCK] = data[3 * BLOCK] = 10      # around block boundaries
    raw = data.tobytes()
    path = tmp_path_factory.mktemp("search-set-nl") / "nl.bz2"
    path.write_bytes(bz2.compress(raw, 1))
    master = corpus["master"]
    at = raw.index(b"\n", 500_000)
    patterns = [master[:5], raw[at - 1:at + 2], master[:17], raw[7000:7003], master[:4]]     # one holds the delimiter
    assert patterns[1][1] == 10 and all(10 not in p for k, p in enumerate(patterns) if k != 1)
    return str(path), raw, patterns


def lines_of(raw, patterns, start=0, end=None, limit=None):
    """(numbers, lines): the distinct lines that hold the first byte of a pair, by a plain split."""
    pieces = raw.split(b"\n")
    lines = [piece + b"\n" for piece in pieces[:-1]] + [pieces[-1]]
    positions = sorted({p for p, _ in pairs_of(raw, patterns, start, end)})
    numbers = sorted({int(k) for k in grepgen.line_numbers_of(raw, positions)})[:limit]
    return numbers, [lines[k] for k in numbers]


def test_grep_any(native, with_newlines):
    path, raw, patterns = with_newlines
    numbers, lines = lines_of(raw, patterns)
    # a line that holds matches of several patterns (every plant of the 17-byte needle) is reported once
    assert len(numbers) > 30 and len(numbers) < len(pairs_of(raw, patterns))
    for parallelization in (1, 0):
        with native.open(path, parallelization=parallelization) as f:
            got, text = f.grep_any(patterns)
            assert got.dtype == np.uint64 and got.tolist() == numbers and text == lines
            assert f.count_matching_lines_any(patterns) == len(numbers)
            for start, end, limit in ((0, None, 7), (123_456, 654_321, None), (2 * BLOCK - 9, 2 * BLOCK + 9, None), (5, 4, None)):
                want = lines_of(raw, patterns, start, end, limit)
                got, text = f.grep_any(patterns, start, end, limit)
                assert (got.tolist(), text) == want, (start, end, limit)
                if limit is None:
                    assert f.count_matching_lines_any(patterns, start, end) == len(want[0])
            assert f.grep_any(patterns, limit=0)[1] == []
            # one pattern as a set is grep
            single = f.grep(patterns[2])
            got, text = f.grep_any([patterns[2]])
            assert got.tolist() == single[0].tolist() and text == single[1]


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import indexed_bzip2_amd as m
from test_gpu_search_set import lines_of

path, raw = sys.argv[2], open(sys.argv[3], "rb").read()
patterns = [bytes.fromhex(word) for word in sys.argv[4:]]
for parallelization in (0, 3):
    with m.open(path, parallelization=parallelization) as f:
        for start, end, limit in ((0, None, None), (0, 400_000, 9), (123_456, 123_457, None), (0, None, 0)):
            numbers, data, offsets = f.grep_any_to_tensor(patterns, start, end, limit)
            want_numbers, want_lines = lines_of(raw, patterns, start, end, limit)
            assert numbers.dtype == np.uint64 and numbers.tolist() == want_numbers
            assert data.dtype == torch.uint8 and data.is_cuda and data.dim() == 1
            assert offsets.dtype == torch.int64 and not offsets.is_cuda
            assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(line) for line in want_lines])]).astype(int).tolist()
            assert bytes(data.cpu().numpy()) == b"".join(want_lines)
        assert f.tell() == 0
print("device grep of a set ok")
"""


def test_grep_any_to_tensor(native, with_newlines, tmp_path):
    path, raw, patterns = with_newlines
    raw_path = tmp_path / "raw"
    raw_path.write_bytes(raw)
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, str(raw_path)] + [p.hex() for p in patterns],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "device grep of a set ok" in run.stdout


def test_file_options_of_the_tool(native, with_newlines, tmp_path):
    path, raw, patterns = with_newlines
    patterns = [p for p in patterns if 10 not in p]
    listed = tmp_path / "patterns.txt"
    listed.write_bytes(b"\n".join(patterns) + b"\n")
    numbers, lines = lines_of(raw, patterns)
    run = subprocess.run([CLI, "--grep-file", str(listed), path], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"".join(lines)
    listed.write_bytes(b"\n".join(patterns))                  # no trailing LF
    run = subprocess.run([CLI, "-P", "1", "--grep-file=" + str(listed), "--line-number", path], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"".join(b"%d:" % (k + 1) + line for k, line in zip(numbers, lines))
    run = subprocess.run([CLI, "--count-matches-file", str(listed), path], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"".join(b"%d\n" % len(matches_of(raw, p)) for p in patterns)
    # refused combinations, and a set beyond the limits
    for options in (["--grep-file", str(listed), "--grep", "x"], ["--count-matches-file", str(listed), "--count-matches", "x"],
                    ["--count-matches-file", str(listed), "--grep-file", str(listed)]):
        run = subprocess.run([CLI] + options + [path], capture_output=True, timeout=600)
        assert run.returncode != 0 and run.stdout == b"", options
    listed.write_bytes(b"x" * 257 + b"\n")
    run = subprocess.run([CLI, "--count-matches-file", str(listed), path], capture_output=True, timeout=600)
    assert run.returncode != 0 and b"1 to 256" in run.stderr


# ------------------------------------------------------------------------------------------------ 8: residency, damage

def test_bounded_residency(native, corpus, monkeypatch):
    """The compressed file is not kept on the GPU: every launch brings the packed windows of its own blocks."""
    c = corpus
    monkeypatch.setenv("MI355X_BZ2_INPUT_BUDGET", "65536")
    with native.open(c["path"], parallelization=3) as f:
        f.set_block_offsets(c["blocks"])
        assert f.statistics()["input_resident"] == 0
        assert as_pairs(f.find_all_any(c["chain"])) == c["expected"]
        want = pairs_of(c["raw"], c["chain"], 123_456, 876_543)
        assert f.count_matches_each(c["chain"], 123_456, 876_543).tolist() == [sum(1 for _, i in want if i == k) for k in range(10)]
        assert f.statistics()["input_resident"] == 0 and f.statistics()["input_bytes_uploaded"] > 0


def test_damaged_block(native, corpus, tmp_path):
    """One byte flipped inside block 7: a set search whose range keeps clear of that block is served, one that needs it
    fails with the block's status and bit offset, and the reader works afterwards."""
    c = corpus
    raw, chain = c["raw"], c["chain"]
    items = sorted(c["blocks"].items())
    bits, next_bits, start, stop = [(b, nb, s, e) for (b, s), (nb, e) in zip(items, items[1:]) if e > s][7]
    assert (start, stop) == (7 * BLOCK, 8 * BLOCK)
    damaged = bytearray(open(c["path"], "rb").read())
    damaged[(bits + next_bits) // 16] ^= 0xFF
    bad = tmp_path / "damaged.bz2"
    bad.write_bytes(bytes(damaged))

    def check_clean(f):
        for a, b in ((17, start), (stop, ALL), (2 * BLOCK + 5, 5 * BLOCK)):
            want = pairs_of(raw, chain, a, b)
            assert len(want) >= 10
            assert as_pairs(f.find_all_any(chain, a, b)) == want, (a, b)
            assert int(f.count_matches_each(chain, a, b).sum()) == len(want), (a, b)

    with native.open(str(bad), parallelization=4) as f:
        f.set_block_offsets(c["blocks"])
        check_clean(f)
        for a, b in ((0, ALL), (start - 1000, start + 1000), (start + 500, start + 600)):
            for call in (f.count_matches_each, f.find_all_any, f.grep_any):
                with pytest.raises(native.Bz2Error) as failure:
                    call(chain, a, b)
                assert failure.value.status != 0
                assert f"bit offset {bits}" in str(failure.value)
        check_clean(f)
