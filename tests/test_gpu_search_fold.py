"""ignore_case on the GPU: the folding instantiations of k_count_bytes / k_emit_bytes / k_count_set / k_emit_set under
Decoder.count_bytes(..., ignore_case=True) and its kin, the reader's search and grep methods with ignore_case, and
`ibzip2-mi355x --ignore-case`.

The rule: fold(b) = b | 0x20 for 'A' <= b <= 'Z', every other byte -- '@', '[', '`', '{' and 0x80 .. 0xFF among them -- as
it is; a match of P at p is fold(D[p + j]) == fold(P[j]) for all j.  That is bytes.lower(), so the model is a
raw.lower().find(P.lower(), p + 1) loop over the raw bytes: never bytes.count (which skips overlapping matches), never the
code under test.

Corpus A is the one of test_gpu_search.py rebuilt here: 1 000 000 seeded printable bytes without equal neighbours at level
1, ten blocks of 99 981 bytes and one of 190 (asserted from block_offsets()).  The needles are prefixes of one seeded
256-byte string whose neighbours differ under the fold too (so no case variant of it holds a run, and the blocks stay
where they are) and that holds at least 60 letters.  One copy of the corpus per needle; at each plant a seeded case variant
of the needle is written, every letter flipped with probability 1/2.  The plants straddle nine of the ten block
boundaries at j bytes in front of them, j taking several values inside the needle, and end exactly on the tenth.

The grep text is grepgen's (9.5 MB, imported, not edited: its size is grepgen's, not this file's choice) at level 9."""
import bz2
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import datagen
import grepgen

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
SIZE = 1_000_000
BLOCK = 99_981
LENGTHS = [1, 2, 3, 16, 17, 33, 256]
ALL = 2**64 - 1
BOUNDARIES = [k * BLOCK for k in range(1, 11)]


def is_letter(b):
    return 65 <= b <= 90 or 97 <= b <= 122


def matches_of(raw, pattern, start=0, end=None):
    """Every p with raw[p:p + m] == pattern, start <= p and p + m <= end (clipped), overlapping ones included."""
    end = len(raw) if end is None else min(end, len(raw))
    start = min(start, end)
    found = []
    p = raw.find(pattern, start, end)
    while p != -1:
        found.append(p)
        p = raw.find(pattern, p + 1, end)
    return found


def fold_matches_of(lowered, pattern, start=0, end=None):
    """The model: `lowered` is raw.lower(), computed once per corpus and never changed."""
    return matches_of(lowered, pattern.lower(), start, end)


def fold_pairs_of(lowered, patterns, start=0, end=None):
    return sorted((p, i) for i, pattern in enumerate(patterns) for p in fold_matches_of(lowered, pattern, start, end))


def as_pairs(result):
    positions, ids = result
    assert positions.dtype == np.uint64 and ids.dtype == np.uint32 and len(positions) == len(ids)
    return list(zip(positions.tolist(), ids.tolist()))


def no_equal_neighbours(r, n):
    """n printable bytes, each different from the one in front of it."""
    steps = r.integers(1, 95, n)
    steps[0] = r.integers(0, 95)
    return (32 + np.cumsum(steps) % 95).astype(np.uint8)


def make_master(r):
    """256 printable bytes, the first a letter, whose neighbours differ also under the fold."""
    out = [int(r.choice(np.frombuffer(b"ghkmqrtwGHKMQRTW", dtype=np.uint8)))]
    while len(out) < 256:
        b = int(r.integers(32, 127))
        if bytes([b]).lower() != bytes([out[-1]]).lower():
            out.append(b)
    return np.array(out, dtype=np.uint8)


def case_variant(needle, r):
    """Every letter flipped with probability 1/2."""
    flips = r.integers(0, 2, len(needle)).astype(bool)
    letters = np.array([is_letter(int(b)) for b in needle])
    return np.where(flips & letters, needle ^ 0x20, needle).astype(np.uint8)


def js_of(m):
    """Bytes of the needle in front of a boundary, for the ten boundaries in turn: all inside the needle but the fourth,
    which the needle ends on."""
    inside = [1, m // 2, m - 1, None, m // 3, m // 2 + 1, (2 * m) // 3, m // 4, m // 2, (3 * m) // 4]
    return [m if j is None else min(max(j, 1), max(m - 1, 1)) for j in inside]


def make_corpus_a(m, master, base):
    """The copy of corpus A for the needle of length m: (raw, needle, plants)."""
    data = base.copy()
    needle = master[:m]
    r = datagen.rng(0xF01D00 + m)
    plants = [k * BLOCK - j for k, j in zip(range(1, 11), js_of(m))]
    for k in range(1, 64):                     # the multiples of 4 096 in the first 256 KiB that no plant is near
        at = k * 4096 - [1, max(1, m // 2), max(m - 1, 1), m][k % 4]
        if all(abs(at - p) > 2 * m + 2 for p in plants):
            plants.append(at)
    for _ in range(6):                         # seeded places inside blocks
        at = int(r.integers(0, 10)) * BLOCK + int(r.integers(2000, BLOCK - 2000))
        if at > 270_000 and all(abs(at - p) > 2 * m + 2 for p in plants):
            plants.append(at)
    for at in plants:
        assert 0 <= at and at + m <= SIZE
        data[at:at + m] = case_variant(needle, r)
    return data.tobytes(), needle.tobytes(), sorted(plants)


def block_offsets_of(native, path):
    with native.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
    assert sorted(set(blocks.values())) == [k * BLOCK for k in range(11)] + [SIZE], sorted(set(blocks.values()))
    return blocks


@pytest.fixture(scope="module")
def corpus_a(native, tmp_path_factory):
    r = datagen.rng(0xF01DCA5E)
    base = no_equal_neighbours(r, SIZE)
    master = make_master(r)
    assert sum(is_letter(int(b)) for b in master) >= 60
    folder = tmp_path_factory.mktemp("search-fold")
    out = {"master": master.tobytes()}
    for m in LENGTHS:
        raw, needle, plants = make_corpus_a(m, master, base)
        assert len(raw) == SIZE and len(needle) == m
        path = folder / f"a{m}.bz2"
        path.write_bytes(bz2.compress(raw, 1))
        blocks = block_offsets_of(native, str(path))
        lowered = raw.lower()
        expected = fold_matches_of(lowered, needle)
        exact = matches_of(raw, needle)
        assert set(plants) <= set(expected) and set(exact) <= set(expected)
        if m >= 16:
            assert len(expected) > len(exact)                                          # folding finds more
            straddling = [(p, b) for p in expected for b in BOUNDARIES if p < b < p + m]
            assert len(straddling) >= 8, (m, straddling)
            # a letter on each side of the boundary whose case is not the needle's
            differs = lambda p, a, b: any(is_letter(needle[j]) and raw[p + j] != needle[j] for j in range(a - p, b - p))
            assert sum(differs(p, p, b) and differs(p, b, p + m) for p, b in straddling) >= 4, m
            assert any(p + m == b for p in expected for b in BOUNDARIES)               # ends exactly on a boundary
        out[m] = {"path": str(path), "raw": raw, "lowered": lowered, "needle": needle, "plants": plants, "blocks": blocks,
                  "expected": expected, "exact": exact}
    return out


def seeded_ranges(c, m, seed):
    """About 30 (start, end) pairs whose edges lie inside planted needles (or on their first and last bytes, for the
    shortest), and a few around them: beyond the size, empty, the whole file."""
    r = np.random.default_rng(seed)
    plants = c["plants"]
    ranges = [(0, ALL), (SIZE - 3, 2**63), (1234, 1234), (5000, 4000), (plants[3], plants[3] + m), (plants[3], plants[3] + m - 1),
              (plants[3] + 1, plants[3] + m + 5)]
    while len(ranges) < 31:
        a, b = sorted(int(p) for p in r.choice(plants, 2))
        ranges.append((a + int(r.integers(0, m)), b + int(r.integers(0, m)) + int(r.integers(0, 2))))
    return ranges


# ------------------------------------------------------------------------------------------------ 1. the rule

@pytest.fixture(scope="module")
def every_byte(native, tmp_path_factory):
    """bytes(range(256)) 256 times over, shuffled: every byte next to every kind of neighbour.  Then every two-byte string
    of `TWO` in its four case forms, and with the byte that a wrong fold would confuse it with, written over seeded places."""
    r = datagen.rng(0xB17E5)
    data = np.frombuffer(bytes(range(256)) * 256, dtype=np.uint8).copy()
    r.shuffle(data)
    forms = set()
    for pattern in TWO:
        for a in (pattern[0], pattern[0] ^ 0x20):
            for b in (pattern[1], pattern[1] ^ 0x20):
                forms.add(bytes([a, b]))
    for k, form in enumerate(sorted(forms) * 3):
        at = 1000 + 523 * k
        data[at:at + 2] = np.frombuffer(form, dtype=np.uint8)
    raw = data.tobytes()
    assert len(raw) == 65536
    path = tmp_path_factory.mktemp("fold-rule") / "bytes.bz2"
    path.write_bytes(bz2.compress(raw, 1))
    return str(path), raw, raw.lower()


TWO = [b"@A", b"Z[", b"`a", b"z{", b"\xC1a", b"A\xE1"]


def test_the_fold_rule_on_the_device(native, every_byte):
    path, raw, lowered = every_byte
    with native.open(path, parallelization=0) as f:
        for b in range(256):
            want = len(fold_matches_of(lowered, bytes([b])))
            assert want >= (500 if is_letter(b) else 240)
            assert f.count_matches(bytes([b]), ignore_case=True) == want, b
        # the neighbours of the letters, and their counterparts above 0x80, do not fold
        for b in b"@[`{\xC1\xDA\xE1\xFA":
            assert f.count_matches(bytes([b]), ignore_case=True) == len(matches_of(raw, bytes([b]))) == f.count_matches(bytes([b]))
        for pattern in TWO:
            for given in (pattern, pattern.lower(), pattern.upper()):
                want = fold_matches_of(lowered, given)
                assert len(want) >= 6
                assert f.find_all(given, ignore_case=True).tolist() == want, given
                assert f.count_matches(given, ignore_case=True) == len(want), given
            # and fewer without the flag
            assert f.find_all(pattern).tolist() == matches_of(raw, pattern)
            assert len(matches_of(raw, pattern)) < len(fold_matches_of(lowered, pattern))
    with native.open(path, parallelization=1) as f:
        assert f.find_all(b"a\xC1", ignore_case=True).tolist() == fold_matches_of(lowered, b"a\xC1")
        assert f.count_matches(b"Q", ignore_case=True) == len(fold_matches_of(lowered, b"q"))


# ------------------------------------------------------------------------------------------------ 2. seams

@pytest.mark.parametrize("parallelization", [1, 3, 0])
@pytest.mark.parametrize("m", LENGTHS)
def test_block_and_launch_seams(native, corpus_a, m, parallelization):
    c = corpus_a[m]
    lowered, needle, expected = c["lowered"], c["needle"], c["expected"]
    total = len(expected)
    mixed = case_variant(np.frombuffer(needle, dtype=np.uint8), datagen.rng(m)).tobytes()
    with native.open(c["path"], parallelization=parallelization) as f:
        if parallelization != 3:
            f.set_block_offsets(c["blocks"])          # at 3 the file is indexed by the search itself
        f.seek(4321)
        for given in (needle.lower(), needle.upper(), mixed):
            assert f.count_matches(given, ignore_case=True) == total
            got = f.find_all(given, ignore_case=True)
            assert got.dtype == np.uint64 and got.tolist() == expected
            assert f.find(given, ignore_case=True) == expected[0]
        for limit in (1, 2, total, total + 1):
            assert f.find_all(mixed, limit=limit, ignore_case=True).tolist() == expected[:limit], limit
        assert f.find_all(mixed, limit=0, ignore_case=True).tolist() == []
        for k, (start, end) in enumerate(seeded_ranges(c, m, 0xF01D + m)):
            given = (needle, needle.lower(), needle.upper(), mixed)[k % 4]
            want = fold_matches_of(lowered, needle, start, end)
            assert f.find_all(given, start, end, ignore_case=True).tolist() == want, (start, end)
            if k < 12:
                assert f.count_matches(given, start, end, ignore_case=True) == len(want), (start, end)
                assert f.find(given, start, end, ignore_case=True) == (want[0] if want else -1), (start, end)
        assert f.tell() == 4321
        assert f.read(1000) == c["raw"][4321:5321]


# ------------------------------------------------------------------------------------------------ 3. not sticky

def test_the_flag_is_not_sticky(native, corpus_a):
    c = corpus_a[17]
    raw, needle = c["raw"], c["needle"]
    exact = matches_of(raw, needle)
    for parallelization in (1, 0):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            assert f.find_all(needle).tolist() == exact and f.count_matches(needle) == len(exact)
            assert f.find_all(needle, ignore_case=True).tolist() == c["expected"] != exact
            assert f.find_all(needle).tolist() == exact and f.count_matches(needle) == len(exact)
            assert f.find_all(needle, ignore_case=False).tolist() == exact
            patterns = [needle, needle.lower()]
            assert as_pairs(f.find_all_any(patterns)) == sorted((p, i) for i, q in enumerate(patterns) for p in matches_of(raw, q))
            assert as_pairs(f.find_all_any(patterns, ignore_case=True)) == fold_pairs_of(c["lowered"], patterns)
            assert as_pairs(f.find_all_any(patterns)) == sorted((p, i) for i, q in enumerate(patterns) for p in matches_of(raw, q))


# ------------------------------------------------------------------------------------------------ 4. the kernels

def decoded(native, c):
    offsets = sorted(bits for bits, start in c["blocks"].items() if start < SIZE)
    dec = native.Decoder(device=0)
    dec.set_input(open(c["path"], "rb").read())
    results, total = dec.decode_batch(offsets)
    out = dec.copy_output(0, total)
    assert total == SIZE and out == c["raw"]
    return dec, out


def test_count_and_find_kernels(native, corpus_a):
    """Decoder.count_bytes / find_bytes with ignore_case over spans of one batch's output: every start alignment 0 to 16,
    sizes around four tiles, a span given twice, spans of size 0 and shorter than the pattern, a capacity at half the
    matches.  The copy of m = 256 holds a case variant of every shorter needle at every plant."""
    c = corpus_a[256]
    dec, out = decoded(native, c)
    lowered = c["lowered"]
    for m in LENGTHS:
        needle = corpus_a["master"][:m]
        given = (needle, needle.lower(), needle.upper())[m % 3]
        for alignment in range(17):
            base = 4096 * 5 + alignment
            spans = [(base, 65536 + d) for d in (-m, -1, 0, 1, m)]
            spans += [spans[2], (base, 0), (base + 3, m - 1), (base, m), (BLOCK - 100 + alignment, 3 * BLOCK)]
            want = [fold_matches_of(lowered, needle, o, o + n) for o, n in spans]
            counts = [len(w) for w in want]
            assert counts[2] >= 4 and counts[6] == 0 and counts[7] == 0
            assert dec.count_bytes(given, spans, ignore_case=True) == counts, (m, alignment)
            positions, found = dec.find_bytes(given, spans, ignore_case=True)
            assert found == counts and positions == [p for w in want for p in w], (m, alignment)
            short = sum(counts) // 2
            positions, found = dec.find_bytes(given, spans, capacity=short, ignore_case=True)
            assert found == counts and positions == [p for w in want for p in w][:short], (m, alignment)
    # the whole output as one span, and the exact instantiation beside it on the same context
    needle = corpus_a["master"][:3]
    want = fold_matches_of(lowered, needle)
    assert dec.count_bytes(needle.upper(), [(0, SIZE), (1, SIZE - 1)], ignore_case=True) == [len(want), len([p for p in want if p >= 1])]
    assert dec.find_bytes(needle, [(0, SIZE)], ignore_case=True) == (want, [len(want)])
    assert dec.find_bytes(needle, [(0, SIZE)]) == (matches_of(out, needle), [len(matches_of(out, needle))])
    assert dec.find_bytes(needle, [(0, SIZE)], ignore_case=False) == (matches_of(out, needle), [len(matches_of(out, needle))])
    assert len(matches_of(out, needle)) < len(want)
    assert dec.count_bytes(needle, [], ignore_case=True) == [] and dec.find_bytes(needle, [], ignore_case=True) == ([], [])
    # an unknown flag bit is refused by the context as well, and says so
    lib = native.lib()
    span = (native._native.ByteSpan * 1)(native._native.ByteSpan(0, 100))
    counts = (ctypes.c_uint64 * 1)()
    sizes = (ctypes.c_uint32 * 1)(3)
    for flags in (2, 3, 0x80000000):
        assert lib.mi355x_bz2_count_bytes_ex(dec._h, span, 1, needle, 3, flags, counts) == 103
        assert b"unknown flag bits" in lib.mi355x_bz2_last_error(dec._h)
        assert lib.mi355x_bz2_find_bytes_ex(dec._h, span, 1, needle, 3, flags, None, 0, counts) == 103
        assert lib.mi355x_bz2_count_bytes_set_ex(dec._h, span, 1, needle, sizes, 1, flags, counts, None) == 103
        assert b"unknown flag bits" in lib.mi355x_bz2_last_error(dec._h)
        assert lib.mi355x_bz2_find_bytes_set_ex(dec._h, span, 1, needle, sizes, 1, flags, None, None, 0, counts, None) == 103
    assert dec.count_bytes(needle, [(0, SIZE)], ignore_case=True) == [len(want)]
    dec.close()


# ------------------------------------------------------------------------------------------------ 5. sets

@pytest.fixture(scope="module")
def set_corpus(native, corpus_a, tmp_path_factory):
    """The copy of m = 33 with two more strings planted in several cases, across two block boundaries too: one that starts
    with '[' (whose | 0x20 is '{') and one that starts with 0xC5 (whose | 0x20 is 0xE5).  The set: the needle in three
    cases -- three ids at every position --, a prefix of it, the two strings, and 40 seeded words cut from the text with
    their case changed."""
    c = corpus_a[33]
    r = datagen.rng(0x5E7F01D)
    data = np.frombuffer(c["raw"], dtype=np.uint8).copy()
    bracket, angstrom = b"[Tag]", b"\xC5ngStrom"
    forms = [bracket, bracket.lower(), bracket.upper(), b"{Tag]", b"{tag]", angstrom, angstrom.upper(), angstrom.lower(),
             b"\xE5ngstrom", b"\xE5NGSTROM"]
    taken = list(c["plants"])
    # the first two go across a block boundary, over the needle that is planted there
    places = [7 * BLOCK - 2, 9 * BLOCK - 3] + [int(p) for p in r.integers(300_000, SIZE - 100, 28)]
    for k, at in enumerate(places):
        if k >= 2 and any(abs(at - p) < 80 for p in taken):
            continue
        form = forms[k % len(forms)]
        data[at:at + len(form)] = np.frombuffer(form, dtype=np.uint8)
        taken.append(at)
    raw = data.tobytes()
    needle = c["needle"]
    words = []
    while len(words) < 40:
        at, size = int(r.integers(0, SIZE - 10)), int(r.integers(3, 9))
        word = raw[at:at + size]
        if sum(is_letter(b) for b in word) >= 2:
            words.append(word.swapcase() if len(words) % 2 else word.lower())
    patterns = [needle.lower(), needle.upper(), needle, needle[:7].upper(), bracket, angstrom] + words
    path = tmp_path_factory.mktemp("search-fold-set") / "set.bz2"
    path.write_bytes(bz2.compress(raw, 1))
    blocks = block_offsets_of(native, str(path))
    lowered = raw.lower()
    pairs = fold_pairs_of(lowered, patterns)
    each = [sum(1 for _, i in pairs if i == k) for k in range(len(patterns))]
    assert each[0] == each[1] == each[2] >= len(c["plants"]) - 2 and each[3] >= each[0]
    assert each[4] >= 2 and each[5] >= 2 and all(n >= 1 for n in each)
    assert len(fold_matches_of(lowered, b"{tag]")) >= 1 and len(fold_matches_of(lowered, b"\xE5ngstrom")) >= 1
    assert any(p < b < p + len(patterns[i]) for p, i in pairs if i >= 4 for b in BOUNDARIES)
    return {"path": str(path), "raw": raw, "lowered": lowered, "blocks": blocks, "patterns": patterns, "pairs": pairs, "each": each}


@pytest.mark.parametrize("parallelization", [1, 0])
def test_sets(native, set_corpus, parallelization):
    c = set_corpus
    patterns, pairs, lowered = c["patterns"], c["pairs"], c["lowered"]
    with native.open(c["path"], parallelization=parallelization) as f:
        f.set_block_offsets(c["blocks"])
        each = f.count_matches_each(patterns, ignore_case=True)
        assert each.dtype == np.uint64 and each.tolist() == c["each"]
        for i in (0, 1, 2, 3, 4, 5, 6, 17, 45):
            assert f.count_matches(patterns[i], ignore_case=True) == c["each"][i], i
        assert as_pairs(f.find_all_any(patterns, ignore_case=True)) == pairs
        assert f.find_any(patterns, ignore_case=True) == pairs[0]
        # with a limit: a prefix, for limits around the first seam
        front = sum(1 for p, _ in pairs if p < BLOCK - 300)
        assert 3 < front < len(pairs) - 12
        for limit in [1, 2, 3] + list(range(front - 2, front + 12, 2)) + [len(pairs), len(pairs) + 1]:
            assert as_pairs(f.find_all_any(patterns, limit=limit, ignore_case=True)) == pairs[:limit], limit
        # ranges whose edges cut planted strings
        first = pairs[len(pairs) // 2][0]
        for start, end in ((first + 1, None), (first, first + 33), (first, first + 32), (BLOCK - 40, BLOCK + 40), (3 * BLOCK - 2, 3 * BLOCK + 2)):
            want = fold_pairs_of(lowered, patterns, start, end)
            assert as_pairs(f.find_all_any(patterns, start, end, ignore_case=True)) == want, (start, end)
            assert f.find_any(patterns, start, end, ignore_case=True) == (want[0] if want else (-1, -1))
        # and the exact set beside it
        exact = sorted((p, i) for i, q in enumerate(patterns) for p in matches_of(c["raw"], q))
        assert as_pairs(f.find_all_any(patterns)) == exact and len(exact) < len(pairs)


def test_count_and_emit_set_kernels(native, set_corpus):
    c = set_corpus
    dec, out = decoded(native, c)
    patterns, lowered = c["patterns"], c["lowered"]
    for alignment in range(17):
        base = 4096 * 5 + alignment                       # sixteen plants of the needle inside, three ids each and a prefix
        spans = [(base, 65536 + d) for d in (-1, 0, 1)] + [(base, 0), (base + 3, 2), (base, 33), (BLOCK - 100 + alignment, 2 * BLOCK)]
        spans.append(spans[1])
        want = [fold_pairs_of(lowered, patterns, o, o + n) for o, n in spans]
        counts = [len(w) for w in want]
        assert counts[1] >= 8 and counts[3] == 0
        got_counts, each = dec.count_bytes_set(patterns, spans, ignore_case=True)
        assert got_counts == counts, alignment
        assert each == [sum(1 for w in want for _, i in w if i == k) for k in range(len(patterns))]
        positions, ids, found = dec.find_bytes_set(patterns, spans, ignore_case=True)
        assert found == counts and list(zip(positions, ids)) == [pair for w in want for pair in w], alignment
        short = sum(counts) // 2
        positions, ids, found = dec.find_bytes_set(patterns, spans, capacity=short, ignore_case=True)
        assert found == counts and list(zip(positions, ids)) == [pair for w in want for pair in w][:short], alignment
    positions, ids, found = dec.find_bytes_set(patterns, [(0, SIZE)], ignore_case=True)
    assert list(zip(positions, ids)) == c["pairs"] and found == [len(c["pairs"])]
    dec.close()


# ------------------------------------------------------------------------------------------------ 6. grep

GREP_NEEDLE = b"N33dLe#7q"


def as_lines(raw):
    """The lines with their delimiters, the unterminated tail as it is."""
    pieces = raw.split(grepgen.NL)
    return [piece + grepgen.NL for piece in pieces[:-1]] + [pieces[-1]]


def fold_grep_of(raw, lowered, patterns, start=0, end=None, limit=None):
    """grepgen.grep_of with the folded matches: the lines themselves come from the raw bytes."""
    lines = as_lines(raw)
    positions = [p for pattern in patterns for p in fold_matches_of(lowered, pattern, start, end)]
    numbers = sorted({int(k) for k in grepgen.line_numbers_of(raw, positions)})
    if limit is not None:
        numbers = numbers[:limit]
    return np.array(numbers, dtype=np.uint64), [lines[k] for k in numbers]


@pytest.fixture(scope="module")
def grep_corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("grep-fold")
    text = grepgen.make_text()
    plain = folder / "plain.bz2"
    plain.write_bytes(datagen.compress(text, 9))
    with native.open(str(plain), parallelization=0) as f:
        items = sorted(f.block_offsets().items())
    starts = [s for (_, s), (_, e) in zip(items, items[1:]) if e > s]
    planted, places = grepgen.plant(text, [starts[1], starts[len(starts) // 2], starts[-1]], GREP_NEEDLE)
    # every second copy gets the other case: the needle occurs in two mixed forms
    data = bytearray(planted)
    offsets = sorted(p for found in places.values() for p in found)
    for p in offsets[1::2]:
        data[p:p + len(GREP_NEEDLE)] = GREP_NEEDLE.swapcase()
    raw = bytes(data)
    path = folder / "planted.bz2"
    path.write_bytes(datagen.compress(raw, 9))
    with native.open(str(path), parallelization=0) as f:
        blocks = f.block_offsets()
    lowered = raw.lower()
    assert fold_matches_of(lowered, GREP_NEEDLE) == offsets and len(matches_of(raw, GREP_NEEDLE)) == (len(offsets) + 1) // 2
    assert any(p < s < p + len(GREP_NEEDLE) for s in sorted(set(blocks.values())) for p in offsets)
    return {"path": str(path), "raw": raw, "lowered": lowered, "blocks": blocks, "offsets": offsets}


@pytest.mark.parametrize("parallelization", [0, 3])
def test_grep(native, grep_corpus, parallelization):
    c = grep_corpus
    raw, lowered = c["raw"], c["lowered"]
    others = [b"no such string", b"#7Q", GREP_NEEDLE.lower()]

    def same(got, want):
        assert got[0].dtype == np.uint64 and np.array_equal(got[0], want[0]) and got[1] == want[1]

    with native.open(c["path"], parallelization=parallelization) as f:
        f.set_block_offsets(c["blocks"])
        f.seek(999)
        for given in (GREP_NEEDLE, GREP_NEEDLE.lower(), GREP_NEEDLE.upper()):
            want = fold_grep_of(raw, lowered, [given])
            assert len(want[1]) >= 8
            same(f.grep(given, ignore_case=True), want)
            assert f.count_matching_lines(given, ignore_case=True) == len(want[1])
            # without the flag: the exact model's, which is less (nothing at all for the lower and the upper form)
            exact = grepgen.grep_of(raw, given)
            same(f.grep(given), exact)
            same(f.grep(given, ignore_case=False), exact)
            assert f.count_matching_lines(given) == len(exact[1]) < len(want[1])
        for limit in (1, 3):
            same(f.grep(GREP_NEEDLE.upper(), limit=limit, ignore_case=True), fold_grep_of(raw, lowered, [GREP_NEEDLE], limit=limit))
        # start and end bound the matches, not the lines
        p = c["offsets"][4]
        for start, end in ((p + 1, None), (p, p + len(GREP_NEEDLE)), (p, p + len(GREP_NEEDLE) - 1), (0, p + len(GREP_NEEDLE))):
            same(f.grep(GREP_NEEDLE.lower(), start, end, ignore_case=True), fold_grep_of(raw, lowered, [GREP_NEEDLE], start, end))
        # sets
        same(f.grep_any(others, ignore_case=True), fold_grep_of(raw, lowered, others))
        assert f.count_matching_lines_any(others, ignore_case=True) == len(fold_grep_of(raw, lowered, others)[1])
        exact_numbers = sorted({int(k) for q in others for k in grepgen.grep_of(raw, q)[0]})
        got = f.grep_any(others)
        assert got[0].tolist() == exact_numbers and len(exact_numbers) < len(fold_grep_of(raw, lowered, others)[1])
        assert f.count_matching_lines_any(others, ignore_case=False) == len(exact_numbers)
        assert f.tell() == 999 and f.read(1000) == raw[999:1999]


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import indexed_bzip2_amd as m
import grepgen
from test_gpu_search_fold import GREP_NEEDLE, fold_grep_of, as_lines

path, raw = sys.argv[2], open(sys.argv[3], "rb").read()
lowered = raw.lower()
others = [b"no such string", b"#7Q", GREP_NEEDLE.lower()]
with m.open(path, parallelization=0) as f:
    for patterns, limit, fold in (([GREP_NEEDLE.upper()], None, True), ([GREP_NEEDLE.lower()], 2, True), ([GREP_NEEDLE], None, False),
                                  (others, None, True), (others, 3, True), (others, None, False), ([GREP_NEEDLE], 0, True)):
        if len(patterns) == 1:
            numbers, data, offsets = f.grep_to_tensor(patterns[0], limit=limit, ignore_case=fold)
        else:
            numbers, data, offsets = f.grep_any_to_tensor(patterns, limit=limit, ignore_case=fold)
        if fold:
            want_numbers, want_lines = fold_grep_of(raw, lowered, patterns, limit=limit)
        else:
            all_numbers = sorted({int(k) for q in patterns for k in grepgen.grep_of(raw, q)[0]})[:limit]
            want_numbers, want_lines = np.array(all_numbers, dtype=np.uint64), [as_lines(raw)[k] for k in all_numbers]
        assert numbers.dtype == np.uint64 and np.array_equal(numbers, want_numbers), (patterns, limit, fold)
        assert data.dtype == torch.uint8 and data.is_cuda and data.dim() == 1
        bounds = [0]
        for line in want_lines:
            bounds.append(bounds[-1] + len(line))
        assert offsets.tolist() == bounds and data.numel() == bounds[-1]
        assert bytes(data.cpu().numpy()) == b"".join(want_lines)
    assert f.tell() == 0
print("device fold grep ok")
"""


def test_grep_to_tensor(native, grep_corpus, tmp_path):
    raw_path = tmp_path / "raw"
    raw_path.write_bytes(grep_corpus["raw"])
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, grep_corpus["path"], str(raw_path)], capture_output=True,
                         text=True, timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "device fold grep ok" in run.stdout


# ------------------------------------------------------------------------------------------------ 7. the tool

def test_the_tool(native, corpus_a, grep_corpus, tmp_path):
    c = corpus_a[17]
    needle = c["needle"]
    run = subprocess.run([os.fsencode(CLI), b"--count-matches", needle.upper(), b"--ignore-case", os.fsencode(c["path"])],
                         capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"%d\n" % len(c["expected"])
    run = subprocess.run([os.fsencode(CLI), b"--count-matches", needle.upper(), os.fsencode(c["path"])], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b"%d\n" % len(matches_of(c["raw"], needle.upper()))

    g = grep_corpus
    raw, lowered = g["raw"], g["lowered"]
    numbers, lines = fold_grep_of(raw, lowered, [GREP_NEEDLE])
    given = GREP_NEEDLE.lower().decode()
    run = subprocess.run([CLI, "--grep", given, "--ignore-case", "--line-number", g["path"]], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"".join(b"%d:" % (k + 1) + line for k, line in zip(numbers.tolist(), lines))
    run = subprocess.run([CLI, "--ignore-case", "-P", "3", "--grep=" + given, g["path"]], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b"".join(lines)
    # without the option the lower-case form is nowhere: nothing is written, and the status is 0 all the same
    run = subprocess.run([CLI, "--grep", given, g["path"]], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b""
    run = subprocess.run([CLI, "--grep", "no such string anywhere", "--ignore-case", g["path"]], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b""
    # a set from a file
    others = [b"no such string", b"#7Q", GREP_NEEDLE.lower()]
    listed = tmp_path / "patterns.txt"
    listed.write_bytes(b"\n".join(others) + b"\n")
    want_numbers, want_lines = fold_grep_of(raw, lowered, others)
    run = subprocess.run([CLI, "--grep-file", str(listed), "--ignore-case", g["path"]], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"".join(want_lines)
    run = subprocess.run([CLI, "--grep-file", str(listed), "--ignore-case", "--line-number", g["path"]], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b"".join(b"%d:" % (k + 1) + line for k, line in zip(want_numbers.tolist(), want_lines))
    run = subprocess.run([CLI, "--count-matches-file", str(listed), "--ignore-case", g["path"]], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"".join(b"%d\n" % len(fold_matches_of(lowered, q)) for q in others)
    listed.write_bytes(b"no such string\nnor this one\n")
    run = subprocess.run([CLI, "--grep-file", str(listed), "--ignore-case", g["path"]], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b""


# ------------------------------------------------------------------------------------------------ 8. bounded residency

def test_bounded_residency(native, corpus_a, set_corpus, monkeypatch):
    """The compressed file is not kept on the GPU: every launch brings the packed windows of its own blocks."""
    c = corpus_a[33]
    monkeypatch.setenv("MI355X_BZ2_INPUT_BUDGET", "65536")
    for parallelization in (1, 3, 0):
        with native.open(c["path"], parallelization=parallelization) as f:
            f.set_block_offsets(c["blocks"])
            assert f.statistics()["input_resident"] == 0
            assert f.find_all(c["needle"].upper(), ignore_case=True).tolist() == c["expected"]
            want = fold_matches_of(c["lowered"], c["needle"], 123_456, 876_543)
            assert f.count_matches(c["needle"].lower(), 123_456, 876_543, ignore_case=True) == len(want)
            assert f.statistics()["input_resident"] == 0 and f.statistics()["input_bytes_uploaded"] > 0
    with native.open(set_corpus["path"], parallelization=3) as f:
        f.set_block_offsets(set_corpus["blocks"])
        assert as_pairs(f.find_all_any(set_corpus["patterns"], ignore_case=True)) == set_corpus["pairs"]
        assert f.statistics()["input_resident"] == 0
