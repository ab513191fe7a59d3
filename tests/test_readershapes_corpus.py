"""The conditions on the corpus of readershapes.py that make test_gpu_reader_shapes.py meaningful, checked on the CPU from
the raw bytes, the parts and the models alone: enough tiny blocks and empty streams, every case a stitch can get wrong on
a launch boundary of every cap, hashes without collisions, and counts that are not trivial."""
import bz2
import re

import numpy as np
import pytest

import fields as F
import grepgen
import linehash as H
import readershapes as R
import regexgen as G
from readershapes import NEEDLE, NL, TAB


@pytest.fixture(scope="module", params=R.VARIANTS)
def c(request):
    return R.expected(request.param)


def line_of(c, offset):
    """(start, end) of the line that holds `offset`: end is its delimiter's offset, or the size."""
    raw = c["raw"]
    start = raw.rfind(b"\n", 0, offset) + 1
    end = raw.find(b"\n", offset)
    return start, len(raw) if end < 0 else end


def launch_of(launches, offset):
    return next(k for k, (lo, hi) in enumerate(launches) if lo <= offset < hi)


def test_deterministic_and_well_formed():
    raw, enc, parts = R.corpus("tail")
    R.corpus.cache_clear()
    again = R.corpus("tail")
    assert again == (raw, enc, parts)
    closed = R.corpus("closed")[0]
    assert not raw.endswith(b"\n") and closed.endswith(b"\n") and closed[:-1] == raw[:-1]
    assert 850_000 < len(raw) < 950_000 and len(enc) < 500_000
    assert b"".join(parts) == raw and bz2.decompress(enc) == raw
    assert {len(p) for p in parts} == set(R.SIZES)


def test_blocks_and_streams(c):
    parts = c["parts"]
    assert 300 <= len(c["block_starts"]) <= 512          # at most the default batch: parallelization 0 is one launch
    assert sum(1 for p in parts if len(p) == 0) >= 20
    ones = [p for p in parts if len(p) == 1]
    assert len(ones) >= 20 and ones.count(b"\n") >= 3
    # what the launch caps of the GPU tests give: 1, about 6, about 70 and about 120 launches
    counts = {cap: len(R.launches_of(c["block_starts"], len(c["raw"]), cap)) for cap in (512, 64, 5, 3)}
    assert counts[512] == 1 and 5 <= counts[64] <= 8 and 60 <= counts[5] <= 105 and 100 <= counts[3] <= 175, counts


def test_kinds_of_lines(c):
    raw, lines = c["raw"], c["lines"]
    sizes = sorted(len(content) for content in lines)
    assert sizes.count(40_000) == 6 and sizes.count(9_000) == 4 and sizes[-1] == 40_000
    assert b"\n\n\n" in raw and any(b"\0" in content and b"\xff" in content for content in lines)
    assert any(b"," in content.split(b"\t")[1] for content in lines if content.count(b"\t") >= 1)
    for content in lines:
        if len(content) >= 9_000:
            tabs = [k for k, byte in enumerate(content) if byte == TAB]
            assert len(tabs) == 4 and tabs[-1] - tabs[-2] > 3_000
    # whole-line duplicates: directly adjacent, and at least a few hundred lines apart
    last, adjacent, far = {}, 0, 0
    for k, content in enumerate(lines):
        if content and content in last:
            adjacent += last[content] == k - 1
            far += k - last[content] >= 300
        last[content] = k
    assert adjacent >= 50 and far >= 50


@pytest.mark.parametrize("cap", R.CAPS)
def test_launch_boundaries(c, cap):
    """With launches taken as consecutive groups of `cap` data blocks."""
    raw, starts = c["raw"], c["block_starts"]
    launches = R.launches_of(starts, len(raw), cap)
    boundaries = [lo for lo, _ in launches[1:]]
    assert boundaries == R.boundaries_of(starts, cap) and len(boundaries) >= 4

    def field_number(b):
        return raw.count(b"\t", line_of(c, b)[0], b)

    assert any(raw[b - 1] == NL for b in boundaries), "no boundary exactly behind a newline"
    assert any(raw[b] == NL for b in boundaries), "no boundary exactly in front of a newline"
    assert any(NL not in raw[b - 1:b + 1] and TAB not in raw[b - 1:b + 1] and field_number(b) >= 1 for b in boundaries), \
        "no boundary inside a field other than field 0"
    assert any(raw[b - 1] == TAB for b in boundaries), "no boundary directly behind a tab"
    if cap in (2, 3, 5):
        assert any(NL not in raw[lo:hi] for lo, hi in launches), "no launch without a newline"
    # a line that starts in one launch and ends three or more launches later
    spans = [(launch_of(launches, start), launch_of(launches, min(end, len(raw) - 1)))
             for start, end in (line_of(c, b) for b in boundaries)]
    assert any(last - first >= 3 for first, last in spans), "no line through three launch boundaries"
    # a needle occurrence and a regex match that straddle a launch boundary
    needles = grepgen.matches_of(raw, NEEDLE)
    assert any(p < b < p + len(NEEDLE) for b in boundaries for p in needles), "no needle across a boundary"
    pattern = re.compile(R.FIELD_REGEX, G.reference_flags(False))
    straddling = 0
    for b in boundaries:
        start, end = line_of(c, b)
        match = pattern.search(raw[start:end])
        straddling += match is not None and start + match.start() < b < start + match.end()
    assert straddling >= 1, "no regex match across a boundary"
    # a matching line whose match lies wholly in a later launch than its start
    later = 0
    for p in needles:
        start, end = line_of(c, p)
        later += launch_of(launches, p) > launch_of(launches, start) and raw.find(NEEDLE, start, end) == p
    assert later >= 1, "no match wholly in a later launch than its line's start"


@pytest.mark.parametrize("cap", R.CAPS)
def test_field_3_across_a_launch_boundary(c, cap):
    """field_hashes patches the one line per seam on the host from P(end) - P(start) * x^(end - start): for every cap at
    least one line has its field 3 start in one launch and end in a later one, so P(start) and P(end) come from different
    launches."""
    boundaries = R.boundaries_of(c["block_starts"], cap)
    for j in (3,):
        across = [(start, size) for start, size in c["spans"][(j, TAB)] if size > 0 and any(start < b < start + size for b in boundaries)]
        assert len(across) >= 1, "no field %d across a launch boundary at cap %d" % (j, cap)
    # ... and, but for the few launches of cap 64, one whose line starts in a launch of its own: three launches in one key
    launches = R.launches_of(c["block_starts"], len(c["raw"]), cap)
    three = 0
    for (start, size), line_start in zip(c["spans"][(3, TAB)], c["line_starts"].tolist()):
        if size > 0:
            three += launch_of(launches, line_start) < launch_of(launches, start) < launch_of(launches, start + size - 1)
    assert three >= 1 or cap == 64, "no line whose start, field 3's start and field 3's end lie in three launches at cap %d" % cap


def test_field_keys_do_not_collide(c):
    """Distinct values have distinct keys under every seed, none is MISSING's: grouping by key is grouping by value."""
    import fieldhash as FH
    for (j, dl), values in c["values"].items():
        distinct = {value for value in values if value is not None}
        for seed in R.SEEDS:
            keys = c["keys"][(j, dl, seed)]
            assert len(keys) == len(values) == len(c["lines"])
            assert [key == FH.MISSING for key in keys] == [value is None for value in values]
            assert len({key for key in keys if key != FH.MISSING}) == len(distinct), (j, dl, seed)
        lines, counts, missing, ranked = c["groups"][(j, dl)]
        assert lines == sorted(lines) and len(lines) == len(distinct) and sum(counts) + missing == len(values)
        assert [count for _, count in ranked] == sorted(counts, reverse=True)
    lines, counts, missing, ranked = c["groups"][(1, TAB)]
    assert len(lines) > 100 and max(counts) > 20 and missing > 100                      # not trivial
    assert c["groups"][(1023, TAB)] == ([], [], len(c["lines"]), [])


def test_hashes_do_not_collide(c):
    """Distinct contents have distinct model hashes under every seed the GPU tests use, so a collision can neither hide a
    failure nor cause one."""
    lines = c["lines"]
    for seed in R.SEEDS:
        hashes = c["hashes"][seed]
        assert len(hashes) == len(lines) and len(set(hashes)) == len(set(lines))
    assert c["hashes"][0][:50] == H.Prefix(c["raw"], H.base(0)).lines(NL)[:50]
    assert c["hashes"][0] != c["hashes"][1]


def test_counts_are_not_trivial(c):
    raw, lines = c["raw"], c["lines"]
    n = len(lines)
    assert n == raw.count(b"\n") + (not raw.endswith(b"\n")) and n > 10_000
    assert len(c["line_starts"]) == raw.count(b"\n") + 1
    for pattern in R.SET_PATTERNS:
        assert len(grepgen.matches_of(raw, pattern)) > 5, pattern
        assert len(grepgen.grep_of(raw, pattern)[0]) > 5, pattern
    folded = len(grepgen.matches_of(raw.lower(), NEEDLE.lower()))
    assert folded > len(grepgen.matches_of(raw, NEEDLE)) + 5
    for (pattern, fold), (numbers, _) in c["regex"].items():
        if pattern == R.REGEX_PATTERNS[-1]:
            assert numbers == [], "the pattern that never matches"
        else:
            assert 5 < len(numbers) < n, (pattern, fold)
    # the pattern of the long lines matches those and nothing else
    for fold in (False, True):
        numbers, matching = c["regex"][(R.REGEX_PATTERNS[4], fold)]
        assert len(numbers) == 6 and all(len(line) == 40_001 for line in matching)
    assert c["regex"][(R.FIELD_REGEX, True)][0] != c["regex"][(R.FIELD_REGEX, False)][0]
    assert 100 < len(c["first_occurrences"]) < n - 100
    sizes = [size for _, size in c["spans"][(3, TAB)]]
    assert sum(1 for size in sizes if size >= 0) > 1000 and sum(1 for size in sizes if size < 0) > 1000
    assert c["field3"].count(None) == sizes.count(-1) and F.fields_of(raw, NL, TAB, 3) == c["field3"]
    assert all(size == -1 for _, size in c["spans"][(1023, TAB)])
