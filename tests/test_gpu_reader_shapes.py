"""Every reader call in every launch shape: the layer of bz2_reader.cpp that cuts a call into launches of at most
`parallelization` blocks, spreads them over one to four decoder contexts, stitches the per-launch summaries on the host and
patches seam lines into device memory -- over the corpus of readershapes.py, whose hundreds of tiny blocks give 1, 8, 94,
156 or 466 launches per whole-file call and whose planted cases lie on the launch boundaries of every cap
(test_readershapes_corpus.py checks that on the CPU).

A shape is (parallelization, MI355X_BZ2_READER_CONTEXTS or none, bounded residency or not).  The contexts a shape runs on
follow BatchScheduler::contextCount -- 1 at parallelization 1, 2 below 64, 3 from 64 on, or the forced number -- and are not
visible through the API; what is asserted is the number of launches (statistics()["batches"]) and the residency.

Every expected value comes from readershapes.expected: the models fields.py, linehash.py, grepgen.py, regexgen.py and the
standard library, computed once per corpus variant, shared, never changed; and from the oracle's block map."""
import io
import random

import numpy as np
import pytest

import grepgen
import readershapes as R
from readershapes import NEEDLE, TAB

pytestmark = pytest.mark.gpu

DEFAULT_BATCH = 512
#         parallelization, MI355X_BZ2_READER_CONTEXTS, contexts that follow
ROWS = ((1, None, 1), (3, None, 2), (5, 4, 4), (64, None, 3), (64, 1, 1), (0, None, "default"))
SHAPES = [(p, forced, bounded) for bounded in (False, True) for p, forced, _ in ROWS]


def shape_id(shape):
    p, forced, bounded = shape
    return "P%d-%s-%s" % (p, "contexts%d" % forced if forced else "unforced", "bounded" if bounded else "resident")


# ------------------------------------------------------------------------------------------------ the expected values

@pytest.fixture(scope="module")
def world(native, oracle, tmp_path_factory):
    """One entry per corpus variant: readershapes.expected (shared, never changed), the file, and the oracle's map."""
    folder = tmp_path_factory.mktemp("shapes")
    out = {"folder": folder}
    for variant in R.VARIANTS:
        e = dict(R.expected(variant))
        path = folder / (variant + ".bz2")
        path.write_bytes(e["enc"])
        status, decoded, block_map, garbage = oracle.decode_file(e["enc"])
        assert status == 0 and decoded == e["raw"] and not garbage
        raw, starts = e["raw"], e["block_starts"]
        e.update(path=str(path), block_map=block_map, size=len(raw), N=len(e["newlines"]), n=len(e["lines"]),
                 starts_ext=e["line_starts"].tolist() + [len(raw)],
                 line_index={**{s: int(np.searchsorted(e["newlines"], s)) for s in starts}, len(raw): len(e["newlines"])})
        assert sorted({b for b in block_map.values()}) == starts + [len(raw)]
        out[variant] = e
    return out


def open_shape(native, monkeypatch, path, shape):
    parallelization, forced, bounded = shape
    if forced is None:
        monkeypatch.delenv("MI355X_BZ2_READER_CONTEXTS", raising=False)
    else:
        monkeypatch.setenv("MI355X_BZ2_READER_CONTEXTS", str(forced))
    if bounded:
        monkeypatch.setenv("MI355X_BZ2_INPUT_BUDGET", "65536")
    else:
        monkeypatch.delenv("MI355X_BZ2_INPUT_BUDGET", raising=False)
    return native.open(path, parallelization=parallelization)


def cap_of(shape):
    return shape[0] or DEFAULT_BATCH


def seams_of(e, shape):
    """The launch boundaries of a whole-file call in this shape that the tests look at: the planted ones and a spread of
    the others (for one launch there is none: those of cap 64 stand in, as places like any other)."""
    boundaries = R.boundaries_of(e["block_starts"], min(cap_of(shape), 64))
    planted = [b for b in boundaries if b in R.planted()[0]]
    return sorted(set(planted + boundaries[::max(1, len(boundaries) // 8)]))


def line_of(e, offset):
    """L(offset): the number of the line that holds it."""
    return int(np.searchsorted(e["newlines"], offset, "left"))


def range_of(e, first, count):
    """The bytes of lines [first, first + count), delimiters included, as read_line_ranges returns them."""
    ext, last = e["starts_ext"], e["N"] + 1
    return e["raw"][ext[min(first, last)]:ext[min(first + count, last)]]


def pairs(spans):
    starts, sizes = spans
    assert starts.dtype == np.uint64 and sizes.dtype == np.int64 and len(starts) == len(sizes)
    return list(zip(starts.tolist(), sizes.tolist()))


def windows_of(e, shape):
    """(first, count) over the numbering of line_hashes: starting and ending on seam lines, one line behind a seam, inside
    the launches of the long line around the run of one-byte streams, at and past the end, and empty."""
    n = e["n"]
    lines = [line_of(e, b) for b in seams_of(e, shape)]
    long_line = line_of(e, R.planted()[1])
    windows = [(lines[0], 1), (lines[1], lines[2] - lines[1] + 1), (lines[0] + 1, 5), (lines[-1] + 1, 1), (lines[-1] - 2, 4)]
    windows += [(k, 1) for k in lines[2:6]] + [(k - 1, 3) for k in lines[3:5]]
    windows += [(long_line, 1), (long_line - 1, 3), (long_line + 1, 2)]
    return windows + [(n - 1, 5), (n, 1), (7, 0), (0, 3), (n - 3, 10**12)]


# ------------------------------------------------------------------------------------------------ the call families

def check_lines_and_ranges(f, e, shape):
    raw, size, N = e["raw"], e["size"], e["N"]
    seams = seams_of(e, shape)
    assert f.count_lines() == N, "count_lines()"
    seam_lines = [line_of(e, b) for b in seams]
    lines = sorted(set(seam_lines + [k + 1 for k in seam_lines] + [0, 1, N, N + 1, N + 5] + list(range(0, N, 997))))
    want = [e["starts_ext"][min(k, N + 1)] for k in lines]
    assert f.line_starts(lines).tolist() == want, "line_starts(%r)" % (lines[:8],)
    ranges = [r for k in seam_lines[:3] for r in ((k - 1, 3), (k, 1), (k + 1, 2))] + [(N - 1, 5), (N + 3, 2), (5, 0)]
    assert f.read_line_ranges(ranges) == [range_of(e, first, count) for first, count in ranges], "read_line_ranges(%r)" % (ranges,)
    offsets = [p for b in seams for p in (b - 1, b, b + 1)] + [0, size - 1, size, size + 5]
    assert f.line_numbers(offsets).tolist() == grepgen.line_numbers_of(raw, offsets).tolist(), "line_numbers(%r)" % (offsets[:9],)
    rng = random.Random(0x4A6E)
    ranges = [(rng.randrange(size), rng.choice([0, 1, 7, 700, 5_000, 50_000])) for _ in range(34)]
    ranges += [(seams[0] - 3, 6), (seams[-1] - 1, 2), (size - 10, 100), (size - 1, 1), (size, 5), (size + 100, 5)]
    assert len(ranges) == 40
    assert f.read_ranges(ranges) == [raw[o:o + s] for o, s in ranges], "read_ranges(40 seeded ranges)"


def check_search(f, e, shape):
    raw = e["raw"]
    seams = seams_of(e, shape)
    window = (seams[1] - 2, seams[-1] + 3)
    for fold in (False, True):
        text, needle = (raw.lower(), NEEDLE.lower()) if fold else (raw, NEEDLE)
        for start, end in ((0, None), window):
            want = grepgen.matches_of(text, needle, start, end)
            label = "(%r, %r, %r, ignore_case=%r)" % (NEEDLE, start, end, fold)
            assert f.count_matches(NEEDLE, start, end, ignore_case=fold) == len(want), "count_matches" + label
            assert f.find_all(NEEDLE, start, end, ignore_case=fold).tolist() == want, "find_all" + label
            assert f.find(NEEDLE, start, end, ignore_case=fold) == (want[0] if want else -1), "find" + label
    assert f.find_all(NEEDLE, limit=7).tolist() == grepgen.matches_of(raw, NEEDLE)[:7], "find_all(limit=7)"
    patterns = list(R.SET_PATTERNS)
    for start, end in ((0, None), window):
        found = [grepgen.matches_of(raw, p, start, end) for p in patterns]
        label = "(%r, %r, %r)" % (patterns, start, end)
        assert f.count_matches_each(patterns, start, end).tolist() == [len(x) for x in found], "count_matches_each" + label
        want = sorted((p, i) for i, x in enumerate(found) for p in x)
        positions, ids = f.find_all_any(patterns, start, end)
        assert list(zip(positions.tolist(), ids.tolist())) == want, "find_all_any" + label
    everything = sorted((p, i) for i, x in enumerate(patterns) for p in grepgen.matches_of(raw, x))
    positions, ids = f.find_all_any(patterns, limit=50)
    assert list(zip(positions.tolist(), ids.tolist())) == everything[:50], "find_all_any(%r, limit=50)" % (patterns,)


def grep_any_of(e, patterns, limit=None):
    raw = e["raw"]
    matches = sorted({p for pattern in patterns for p in grepgen.matches_of(raw, pattern)})
    numbers = sorted({int(k) for k in grepgen.line_numbers_of(raw, matches)})[:limit]
    return numbers, [range_of(e, k, 1) for k in numbers]


def check_grep(f, e, shape):
    raw = e["raw"]
    for fold in (False, True):
        text, needle = (raw.lower(), NEEDLE.lower()) if fold else (raw, NEEDLE)
        for limit in (None, 3):
            want_numbers, _ = grepgen.grep_of(text, needle, limit=limit)
            numbers, lines = f.grep(NEEDLE, limit=limit, ignore_case=fold)
            label = "grep(%r, limit=%r, ignore_case=%r)" % (NEEDLE, limit, fold)
            assert numbers.tolist() == want_numbers.tolist(), label
            assert lines == [range_of(e, int(k), 1) for k in want_numbers], label
        assert f.count_matching_lines(NEEDLE, ignore_case=fold) == len(grepgen.grep_of(text, needle)[0]), \
            "count_matching_lines(%r, ignore_case=%r)" % (NEEDLE, fold)
    seams = seams_of(e, shape)
    start, end = seams[0] - 2, seams[-1] + 3
    want_numbers, want_lines = grepgen.grep_of(raw, NEEDLE, start, end)
    numbers, lines = f.grep(NEEDLE, start, end)
    assert numbers.tolist() == want_numbers.tolist() and lines == want_lines, "grep(%r, %d, %d)" % (NEEDLE, start, end)
    patterns = [NEEDLE, b"err", b"ab,"]
    for limit in (None, 4):
        want_numbers, want_lines = grep_any_of(e, patterns, limit)
        numbers, lines = f.grep_any(patterns, limit=limit)
        assert numbers.tolist() == want_numbers and lines == want_lines, "grep_any(%r, limit=%r)" % (patterns, limit)


def check_regex(f, e, shape):
    for (pattern, fold), (want_numbers, want_lines) in e["regex"].items():
        label = "(%r, ignore_case=%r)" % (pattern, fold)
        numbers, lines = f.grep_regex(pattern, ignore_case=fold)
        assert numbers.dtype == np.uint64 and numbers.tolist() == want_numbers, "grep_regex" + label
        assert lines == want_lines, "grep_regex" + label
        assert f.count_matching_lines_regex(pattern, ignore_case=fold) == len(want_numbers), "count_matching_lines_regex" + label
    for pattern in (R.REGEX_PATTERNS[0], R.REGEX_PATTERNS[4]):
        want_numbers, want_lines = e["regex"][(pattern, False)]
        for limit in (1, len(want_numbers) - 1):
            numbers, lines = f.grep_regex(pattern, limit=limit)
            assert numbers.tolist() == want_numbers[:limit] and lines == want_lines[:limit], "grep_regex(%r, limit=%d)" % (pattern, limit)


def check_hashes(f, e, shape):
    for seed in R.SEEDS:
        got = f.line_hashes(seed=seed)
        assert got.dtype == np.uint64 and got.tolist() == e["hashes"][seed], "line_hashes(seed=%d)" % seed
    for first, count in windows_of(e, shape):
        assert f.line_hashes(first, count).tolist() == e["hashes"][0][first:first + count], "line_hashes(%d, %d)" % (first, count)
    first, count = windows_of(e, shape)[1]
    assert f.line_hashes(first, count, seed=1).tolist() == e["hashes"][1][first:first + count], "line_hashes(%d, %d, seed=1)" % (first, count)
    for seed in R.SEEDS:
        assert f.count_distinct_lines(seed=seed) == len(e["first_occurrences"]), "count_distinct_lines(seed=%d)" % seed
        assert f.first_occurrences(seed=seed).tolist() == e["first_occurrences"], "first_occurrences(seed=%d)" % seed


def check_fields(f, e, shape):
    windows = windows_of(e, shape)
    for (j, dl), want in e["spans"].items():
        delimiter = bytes([dl])
        assert pairs(f.field_spans(j, delimiter=delimiter)) == want, "field_spans(%d, delimiter=%r)" % (j, delimiter)
        for first, count in windows:
            assert pairs(f.field_spans(j, first, count, delimiter)) == want[first:first + count], \
                "field_spans(%d, %d, %d, %r)" % (j, first, count, delimiter)
    assert f.read_fields(3) == e["field3"], "read_fields(3)"
    for first, count in windows[:-1]:
        assert f.read_fields(3, first, count) == e["field3"][first:first + count], "read_fields(3, %d, %d)" % (first, count)
    assert f.field_spans(0)[0].tolist() == f.line_starts(range(e["n"])).tolist(), "field_spans(0) against line_starts"


def groups_of(e, j, dl, first=0, count=None):
    return e["groups"][(j, dl)] if (first, count) == (0, None) else R.groups_of(e["values"][(j, dl)], first, count)


def grouped(got):
    lines, counts, missing = got
    assert lines.dtype == counts.dtype == np.uint64 and isinstance(missing, int)
    return lines.tolist(), counts.tolist(), missing


def check_field_hashes(f, e, shape):
    windows = windows_of(e, shape)
    for j, dl in R.FIELDS:
        delimiter = bytes([dl])
        for seed in R.SEEDS:
            got = f.field_hashes(j, delimiter=delimiter, seed=seed)
            assert got.dtype == np.uint64 and got.tolist() == e["keys"][(j, dl, seed)], "field_hashes(%d, delimiter=%r, seed=%d)" % (j, delimiter, seed)
        for first, count in windows:
            assert f.field_hashes(j, first, count, delimiter).tolist() == e["keys"][(j, dl, 0)][first:first + count], \
                "field_hashes(%d, %d, %d, %r)" % (j, first, count, delimiter)
        lines, counts, missing, ranked = groups_of(e, j, dl)
        # (a whole-file call is one pass, hundreds of launches at parallelization 1: the second seed and the unlimited
        # value_counts go to two of the six fields)
        for seed in R.SEEDS if j in (1, 3) else R.SEEDS[:1]:
            assert grouped(f.count_by_field(j, delimiter=delimiter, seed=seed)) == (lines, counts, missing), \
                "count_by_field(%d, delimiter=%r, seed=%d)" % (j, delimiter, seed)
        if j in (1, 3):
            assert f.value_counts(j, delimiter=delimiter) == ranked, "value_counts(%d, delimiter=%r)" % (j, delimiter)
        assert f.value_counts(j, 5, delimiter=delimiter, seed=1) == ranked[:5], "value_counts(%d, 5, delimiter=%r, seed=1)" % (j, delimiter)
    first, count = windows[1]
    assert f.field_hashes(3, first, count, seed=1).tolist() == e["keys"][(3, TAB, 1)][first:first + count], "field_hashes(3, %d, %d, seed=1)" % (first, count)
    for first, count in windows[:9] + windows[-3:]:
        for j, dl in ((3, TAB), (1, ord(","))):
            lines, counts, missing, ranked = groups_of(e, j, dl, first, count)
            label = "(%d, %d, %d, %r)" % (j, first, count, bytes([dl]))
            assert grouped(f.count_by_field(j, first, count, bytes([dl]))) == (lines, counts, missing), "count_by_field" + label
            assert f.value_counts(j, 3, first, count, bytes([dl])) == ranked[:3], "value_counts limit 3 " + label


def launches_by_call(f, e):
    """{call: launches it made}, from statistics()["batches"] before and after: whole-file calls of one pass each."""
    counts = {}
    for name, call in (("count_matches", lambda: f.count_matches(NEEDLE)),
                       ("count_matching_lines_regex", lambda: f.count_matching_lines_regex(R.FIELD_REGEX)),
                       ("line_hashes", lambda: f.line_hashes()), ("field_spans", lambda: f.field_spans(3)),
                       ("field_hashes", lambda: f.field_hashes(3)), ("count_by_field", lambda: f.count_by_field(3)),
                       ("grep_regex", lambda: f.grep_regex(R.REGEX_PATTERNS[0])), ("read_fields", lambda: f.read_fields(3)),
                       ("value_counts", lambda: f.value_counts(3))):
        before = f.statistics()["batches"]
        call()
        counts[name] = f.statistics()["batches"] - before
    return counts


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_call(native, world, monkeypatch, shape, variant):
    """The time follows the launches: about 47 000 of one block each at parallelization 1 (34 s on an MI355X, 0.7 ms per
    launch on one context), 16 000 at 3 (7.5 s), 9 400 at 5 on four contexts (3.5 s), under 1 000 from 64 on (1 s).
    With field_hashes, count_by_field and value_counts -- about 30 more whole-file calls -- the measured times are 50 s, 12 to
    15 s, 6 s and 1 s."""
    e = world[variant]
    with open_shape(native, monkeypatch, e["path"], shape) as f:
        check_lines_and_ranges(f, e, shape)
        # the shape is what it claims to be: so many launches per pass over the file, and the residency asked for
        counts = launches_by_call(f, e)
        print("launches %s %s: %r" % (shape_id(shape), variant, counts))
        launches = len(R.launches_of(e["block_starts"], e["size"], cap_of(shape)))
        for name in ("count_matches", "count_matching_lines_regex", "line_hashes", "field_spans", "field_hashes", "count_by_field"):
            assert counts[name] == launches, (name, counts, launches)
        assert counts["grep_regex"] > launches and counts["read_fields"] > launches and counts["value_counts"] > launches
        statistics = f.statistics()
        if shape[2]:
            assert statistics["input_resident"] == 0 and statistics["input_bytes_uploaded"] > 0
        else:
            assert statistics["input_resident"] == 1
        check_search(f, e, shape)
        check_grep(f, e, shape)
        check_regex(f, e, shape)
        check_hashes(f, e, shape)
        check_fields(f, e, shape)
        check_field_hashes(f, e, shape)
        assert f.tell() == 0, "a query moved the position"
        assert f.read() == e["raw"], "read()"
        assert f.block_offsets() == e["block_map"], "block_offsets()"


# ------------------------------------------------------------------------------------------------ call orders

ORDER_SHAPES = [(3, None, False), (64, None, False), (5, 4, True)]
ORDER_SEED = 0x0DE5
OPERATIONS = 80


def query_operations(f, e, shape, rng):
    """One seeded query of every kind of test_every_call: [(label, call, wanted)] with results as plain lists."""
    raw, size, n, N = e["raw"], e["size"], e["n"], e["N"]
    seams = seams_of(e, shape)

    def window():
        return rng.choice(windows_of(e, shape)[:-1] + [(rng.randrange(n), rng.choice([0, 1, 5, 300]))])

    def byte_range():
        start = rng.choice(seams + [0, rng.randrange(size)]) - rng.randrange(3)
        return max(start, 0), rng.choice([None, start + rng.choice([4, 5, 3_000, 200_000])])

    first, count = window()
    start, end = byte_range()
    seed = rng.choice(R.SEEDS)
    (j, dl), fold = rng.choice(R.FIELDS), rng.choice([False, True])
    pattern = rng.choice(R.REGEX_PATTERNS)
    regex_limit = rng.choice([None, 3])
    text, needle = (raw.lower(), NEEDLE.lower()) if fold else (raw, NEEDLE)
    offsets = [rng.choice(seams) + rng.randrange(-2, 3) for _ in range(20)] + [rng.randrange(size + 10) for _ in range(20)]
    lines = [rng.randrange(N + 4) for _ in range(30)] + [line_of(e, b) for b in seams[:4]]
    line_ranges = [(rng.randrange(N + 2), rng.choice([0, 1, 2, 40])) for _ in range(6)]
    byte_ranges = [(rng.randrange(size + 5), rng.choice([0, 1, 700, 50_000])) for _ in range(8)]
    patterns = list(R.SET_PATTERNS)
    want_regex = e["regex"][(pattern, fold)]
    return [
        ("line_hashes(%d, %d, seed=%d)" % (first, count, seed), lambda: f.line_hashes(first, count, seed=seed).tolist(),
         e["hashes"][seed][first:first + count]),
        ("field_spans(%d, %d, %d, %r)" % (j, first, count, bytes([dl])), lambda: pairs(f.field_spans(j, first, count, bytes([dl]))),
         e["spans"][(j, dl)][first:first + count]),
        ("read_fields(3, %d, %d)" % (first, count), lambda: f.read_fields(3, first, count), e["field3"][first:first + count]),
        ("field_hashes(%d, %d, %d, %r, seed=%d)" % (j, first, count, bytes([dl]), seed),
         lambda: f.field_hashes(j, first, count, bytes([dl]), seed=seed).tolist(), e["keys"][(j, dl, seed)][first:first + count]),
        ("field_hashes(%d, delimiter=%r, seed=%d)" % (j, bytes([dl]), seed),
         lambda: f.field_hashes(j, delimiter=bytes([dl]), seed=seed).tolist(), e["keys"][(j, dl, seed)]),
        ("count_by_field(%d, %d, %d, %r, seed=%d)" % (j, first, count, bytes([dl]), seed),
         lambda: grouped(f.count_by_field(j, first, count, bytes([dl]), seed=seed)), groups_of(e, j, dl, first, count)[:3]),
        ("count_by_field(%d, delimiter=%r, seed=%d)" % (j, bytes([dl]), seed),
         lambda: grouped(f.count_by_field(j, delimiter=bytes([dl]), seed=seed)), groups_of(e, j, dl)[:3]),
        ("value_counts(%d, %r, %d, %d, %r)" % (j, regex_limit, first, count, bytes([dl])),
         lambda: f.value_counts(j, regex_limit, first, count, bytes([dl])), groups_of(e, j, dl, first, count)[3][:regex_limit]),
        ("value_counts(%d, %r, delimiter=%r, seed=%d)" % (j, regex_limit, bytes([dl]), seed),
         lambda: f.value_counts(j, regex_limit, delimiter=bytes([dl]), seed=seed), groups_of(e, j, dl)[3][:regex_limit]),
        ("grep_regex(%r, limit=%r, ignore_case=%r)" % (pattern, regex_limit, fold),
         lambda: (lambda got: (got[0].tolist(), got[1]))(f.grep_regex(pattern, limit=regex_limit, ignore_case=fold)),
         (want_regex[0][:regex_limit], want_regex[1][:regex_limit])),
        ("count_matching_lines_regex(%r, ignore_case=%r)" % (pattern, fold),
         lambda: f.count_matching_lines_regex(pattern, ignore_case=fold), len(want_regex[0])),
        ("grep(%r, %r, %r, ignore_case=%r)" % (NEEDLE, start, end, fold),
         lambda: (lambda got: (got[0].tolist(), got[1]))(f.grep(NEEDLE, start, end, ignore_case=fold)),
         (lambda want: (want[0].tolist(), [range_of(e, int(k), 1) for k in want[0]]))(grepgen.grep_of(text, needle, start, end))),
        ("find_all(%r, %r, %r, ignore_case=%r)" % (NEEDLE, start, end, fold),
         lambda: f.find_all(NEEDLE, start, end, ignore_case=fold).tolist(), grepgen.matches_of(text, needle, start, end)),
        ("count_matches_each(%r, %r, %r)" % (patterns, start, end), lambda: f.count_matches_each(patterns, start, end).tolist(),
         [len(grepgen.matches_of(raw, p, start, end)) for p in patterns]),
        ("find_all_any(%r, %r, %r, limit=50)" % (patterns, start, end),
         lambda: (lambda got: list(zip(got[0].tolist(), got[1].tolist())))(f.find_all_any(patterns, start, end, limit=50)),
         sorted((p, i) for i, x in enumerate(patterns) for p in grepgen.matches_of(raw, x, start, end))[:50]),
        ("line_numbers(%r)" % (offsets,), lambda: f.line_numbers(offsets).tolist(), grepgen.line_numbers_of(raw, offsets).tolist()),
        ("line_starts(%r)" % (lines,), lambda: f.line_starts(lines).tolist(), [e["starts_ext"][min(k, N + 1)] for k in lines]),
        ("read_line_ranges(%r)" % (line_ranges,), lambda: f.read_line_ranges(line_ranges), [range_of(e, a, b) for a, b in line_ranges]),
        ("read_ranges(%r)" % (byte_ranges,), lambda: f.read_ranges(byte_ranges), [raw[o:o + s] for o, s in byte_ranges]),
        ("count_distinct_lines(seed=%d)" % seed, lambda: f.count_distinct_lines(seed=seed), len(e["first_occurrences"])),
        ("first_occurrences(seed=%d)" % seed, lambda: f.first_occurrences(seed=seed).tolist(), e["first_occurrences"]),
        ("count_lines()", lambda: f.count_lines(), N),
    ]


@pytest.mark.parametrize("shape", ORDER_SHAPES, ids=shape_id)
def test_call_orders(native, world, monkeypatch, shape):
    """80 operations from a fixed seed on one reader: seeks and reads, which move the position; queries of every kind, which
    do not, although they go to the front of the job queue that the reads' look-ahead stands in; and the import of maps
    that the same reader exported.  The first three are a read of one byte at offset 0 -- its look-ahead is then in flight
    --, a whole-file grep_regex and a read of 300 000 bytes."""
    e = world["tail"]
    raw, size = e["raw"], e["size"]
    rng = random.Random(ORDER_SEED)
    exported, position = None, 0
    with open_shape(native, monkeypatch, e["path"], shape) as f:
        for index in range(OPERATIONS):
            where = "seed %#x, operation %d: " % (ORDER_SEED, index)
            kind = ("read", "regex", "read")[index] if index < 3 else rng.choice(["seek", "read", "query", "query", "query", "maps"])
            if kind == "seek":
                whence = rng.choice([io.SEEK_SET, io.SEEK_CUR, io.SEEK_END])
                if whence == io.SEEK_SET:
                    offset = rng.randrange(size + 1_000)
                    target = offset
                elif whence == io.SEEK_CUR:
                    offset = rng.randrange(-min(position, 200_000), 200_000)
                    target = position + offset
                else:
                    offset = -rng.randrange(size)
                    target = size + offset
                got = f.seek(offset, whence)
                position = min(target, size)
                assert got == position, where + "seek(%d, %d)" % (offset, whence)
                kind = "read"                                   # as dev_fuzz_seek.py: every seek is followed by a read
            if kind == "read":
                n = (1, None, 300_000)[index] if index < 3 else rng.choice([0, 1, 7, 1_000, 65_536, 300_000])
                data = f.read(n)
                assert data == raw[position:position + n], where + "read(%d) at %d" % (n, position)
                position += len(data)
            elif kind == "regex":
                numbers, lines = f.grep_regex(R.FIELD_REGEX)
                assert (numbers.tolist(), lines) == e["regex"][(R.FIELD_REGEX, False)], where + "grep_regex behind read(1)"
            elif kind == "query":
                label, call, want = rng.choice(query_operations(f, e, shape, rng))
                assert call() == want, where + label
            elif exported is None:
                exported = (f.line_offsets(), f.block_offsets())                # the line index first: it completes the
                assert exported[0] == e["line_index"], where + "line_offsets()"  # block map without moving the position
                assert exported[1] == e["block_map"], where + "block_offsets()"
            else:
                f.set_block_offsets(exported[1])                                 # each used once
                f.set_line_offsets(exported[0])
                exported = None
            assert f.tell() == position, where + "tell() after " + kind
        assert index == OPERATIONS - 1


# ------------------------------------------------------------------------------------------------ failures

def data_blocks_of(e):
    """[(bit offset, bit offset of what follows, decoded start, decoded end, newlines inside)] of the data blocks."""
    items = sorted(e["block_map"].items())
    return [(bits, next_bits, start, stop, line_of(e, stop) - line_of(e, start))
            for (bits, start), (next_bits, stop) in zip(items, items[1:]) if stop > start]


def block_for_damage(e):
    """A 6 000-byte block near the middle of the file with many lines, its neighbours likewise."""
    blocks = data_blocks_of(e)
    good = [b for b in range(2, len(blocks) - 2) if blocks[b][3] - blocks[b][2] == 6_000
            and all(blocks[k][4] >= 10 and blocks[k][3] - blocks[k][2] >= 2_000 for k in (b - 1, b, b + 1))]
    return min(good, key=lambda b: abs(blocks[b][2] - e["size"] // 2))


FAILURE_SHAPES = [(1, None, False), (3, None, False), (64, None, False)]


@pytest.mark.parametrize("shape", FAILURE_SHAPES, ids=shape_id)
def test_damaged_block(native, world, monkeypatch, tmp_path, shape):
    """One byte flipped in the middle of a block, both true indexes imported: grep_regex, line_hashes, the distinct lines,
    field_spans, read_fields, field_hashes, count_by_field and value_counts serve what keeps clear of the block and fail,
    with the status and the bit offset of a plain read, for what needs it -- and go on serving afterwards."""
    e = world["tail"]
    blocks = data_blocks_of(e)
    bits, next_bits, start, stop, _ = blocks[block_for_damage(e)]
    damaged = bytearray(e["enc"])
    damaged[(bits + next_bits) // 16] ^= 0xFF
    bad = tmp_path / "damaged.bz2"
    bad.write_bytes(bytes(damaged))
    with open_shape(native, monkeypatch, str(bad), shape) as f:
        with pytest.raises(native.Bz2Error) as failure:
            f.read()
        status = failure.value.status
        assert status != 0
    in_front, behind = line_of(e, start) - 15, line_of(e, stop) + 2          # windows of 10 lines clear of the block
    inside = line_of(e, start) + 2
    hashes, spans, field3, keys = e["hashes"][0], e["spans"][(3, TAB)], e["field3"], e["keys"][(3, TAB, 0)]

    def served(f):
        return [(f.line_hashes(first, 10).tolist(), pairs(f.field_spans(3, first, 10)), f.read_fields(3, first, 10),
                 f.field_hashes(3, first, 10).tolist(), grouped(f.count_by_field(3, first, 10)), f.value_counts(3, None, first, 10))
                for first in (in_front, behind)]

    with open_shape(native, monkeypatch, str(bad), shape) as f:
        f.set_block_offsets(e["block_map"])
        f.set_line_offsets(e["line_index"])
        before = served(f)
        assert before == [(hashes[k:k + 10], spans[k:k + 10], field3[k:k + 10], keys[k:k + 10], groups_of(e, 3, TAB, k, 10)[:3],
                           groups_of(e, 3, TAB, k, 10)[3]) for k in (in_front, behind)]
        failing = [("grep_regex", lambda: f.grep_regex(R.REGEX_PATTERNS[0])),
                   ("count_matching_lines_regex", lambda: f.count_matching_lines_regex(R.FIELD_REGEX)),
                   ("line_hashes()", lambda: f.line_hashes()), ("line_hashes(seed=1)", lambda: f.line_hashes(seed=1)),
                   ("count_distinct_lines", lambda: f.count_distinct_lines()), ("first_occurrences", lambda: f.first_occurrences()),
                   ("field_spans(3)", lambda: f.field_spans(3)), ("field_spans(1, ',')", lambda: f.field_spans(1, delimiter=b",")),
                   ("read_fields(3)", lambda: f.read_fields(3)),
                   ("line_hashes(inside, 2)", lambda: f.line_hashes(inside, 2)),
                   ("field_spans(3, inside, 2)", lambda: f.field_spans(3, inside, 2)),
                   ("read_fields(3, inside, 2)", lambda: f.read_fields(3, inside, 2)),
                   ("line_hashes(across)", lambda: f.line_hashes(in_front, behind - in_front)),
                   ("field_spans(across)", lambda: f.field_spans(0, in_front, behind - in_front)),
                   ("field_hashes(3)", lambda: f.field_hashes(3)), ("field_hashes(1, ',', seed=1)", lambda: f.field_hashes(1, delimiter=b",", seed=1)),
                   ("count_by_field(3)", lambda: f.count_by_field(3)), ("value_counts(3)", lambda: f.value_counts(3)),
                   ("value_counts(3, 2)", lambda: f.value_counts(3, 2)),
                   ("field_hashes(3, inside, 2)", lambda: f.field_hashes(3, inside, 2)),
                   ("count_by_field(3, inside, 2)", lambda: f.count_by_field(3, inside, 2)),
                   ("value_counts(3, inside, 2)", lambda: f.value_counts(3, None, inside, 2)),
                   ("field_hashes(across)", lambda: f.field_hashes(0, in_front, behind - in_front)),
                   ("count_by_field(across)", lambda: f.count_by_field(0, in_front, behind - in_front))]
        for k, (name, call) in enumerate(failing):
            with pytest.raises(native.Bz2Error) as failure:
                call()
            assert failure.value.status == status, name
            assert f"bit offset {bits}" in str(failure.value), name
            # after each failure a clean call is answered correctly
            first = (in_front, behind)[k % 2]
            assert f.line_hashes(first, 10).tolist() == hashes[first:first + 10], "line_hashes behind the failure of " + name
            assert pairs(f.field_spans(3, first, 10)) == spans[first:first + 10], "field_spans behind the failure of " + name
            assert f.field_hashes(3, first, 10).tolist() == keys[first:first + 10], "field_hashes behind the failure of " + name
        assert served(f) == before
        # (a read() fills a buffer of 1 MiB, more than the file: it would ask for the damaged block)
        assert f.tell() == 0 and f.read_ranges([(0, 1000), (stop, 700)]) == [e["raw"][:1000], e["raw"][stop:stop + 700]]


def block_for_lie(e):
    """b with blocks b - 1, b and b + 1 each of at least 2 000 bytes and 10 lines, in the first half of the file."""
    blocks = data_blocks_of(e)
    return next(b for b in range(len(blocks) // 4, len(blocks) - 2)
                if all(blocks[k][4] >= 10 and blocks[k][3] - blocks[k][2] >= 2_000 for k in (b - 1, b, b + 1)))


@pytest.mark.parametrize("shape", FAILURE_SHAPES, ids=shape_id)
def test_lying_line_index(native, world, monkeypatch, shape):
    """The imported line index gives block b one delimiter more and block b + 1 one fewer: line_hashes, field_spans,
    read_fields, field_hashes, count_by_field and value_counts of a
    window that needs block b fail with status 106 and say which block, what was promised and what was counted; a window
    clear of both blocks is served, and so is everything once the true index is back."""
    e = world["tail"]
    blocks = data_blocks_of(e)
    b = block_for_lie(e)
    start, following, held = blocks[b][2], blocks[b + 1][2], blocks[b][4]
    true_index = e["line_index"]
    lying = dict(true_index)
    lying[following] += 1
    failing = (true_index[start] + 3, 4)                                       # lines that lie inside block b
    clear = (true_index[blocks[b - 1][2]] + 2, 3)                              # ... inside block b - 1
    assert true_index[following] - true_index[start] == held and failing[0] + failing[1] < true_index[following] - 2
    hashes, spans, keys = e["hashes"][0], e["spans"][(3, TAB)], e["keys"][(3, TAB, 0)]
    message = "decoded offset %d %d delimiters, it holds %d" % (start, held + 1, held)
    with open_shape(native, monkeypatch, e["path"], shape) as f:
        f.set_block_offsets(e["block_map"])
        f.set_line_offsets(lying)
        for name, call in (("line_hashes", lambda: f.line_hashes(*failing)), ("field_spans", lambda: f.field_spans(3, *failing)),
                           ("read_fields", lambda: f.read_fields(3, *failing)), ("field_hashes", lambda: f.field_hashes(3, *failing)),
                           ("count_by_field", lambda: f.count_by_field(3, *failing)),
                           ("value_counts", lambda: f.value_counts(3, None, *failing))):
            with pytest.raises(native.Bz2Error) as failure:
                call()
            assert failure.value.status == 106 and "line index" in str(failure.value), name
            assert message in str(failure.value), (name, str(failure.value))
            assert f.line_hashes(*clear).tolist() == hashes[clear[0]:clear[0] + clear[1]], "line_hashes clear of the lie"
            assert pairs(f.field_spans(3, *clear)) == spans[clear[0]:clear[0] + clear[1]], "field_spans clear of the lie"
            assert f.field_hashes(3, *clear).tolist() == keys[clear[0]:clear[0] + clear[1]], "field_hashes clear of the lie"
            assert grouped(f.count_by_field(3, *clear)) == groups_of(e, 3, TAB, *clear)[:3], "count_by_field clear of the lie"
        f.set_line_offsets(true_index)
        assert f.line_hashes(*failing).tolist() == hashes[failing[0]:failing[0] + failing[1]]
        assert pairs(f.field_spans(3, *failing)) == spans[failing[0]:failing[0] + failing[1]]
        assert f.read_fields(3, *failing) == e["field3"][failing[0]:failing[0] + failing[1]]
        assert f.field_hashes(3, *failing).tolist() == keys[failing[0]:failing[0] + failing[1]]
        assert grouped(f.count_by_field(3, *failing)) == groups_of(e, 3, TAB, *failing)[:3]
        assert f.value_counts(3, None, *failing) == groups_of(e, 3, TAB, *failing)[3]
        assert f.tell() == 0 and f.read(1000) == e["raw"][:1000]
