"""A corpus of hundreds of tiny blocks, shared by test_readershapes_corpus.py (its conditions, on the CPU) and
test_gpu_reader_shapes.py (every reader call in every launch shape).  Nothing here touches the code under test.

About 900 kB of records, cut into consecutive parts of 0, 1, 700, 2 000, 3 000, 4 096 or 6 000 bytes, each part a bzip2
stream of its own: every data block is that small, so that a launch cap of 3, 5 or 64 blocks gives dozens of launches
from a file that decodes in milliseconds.  The part sizes are drawn first; the text is then written line by line around
the launch boundaries they give (launches of a whole-file call are consecutive groups of `cap` data blocks), so that the
cases a stitch can get wrong lie exactly on boundaries of every cap in CAPS -- planted by construction, as grepgen.plant
does, not left to the seed:

  behind-nl     the boundary directly behind a "\\n"
  before-nl     the boundary directly in front of a "\\n" (both-nl: both at once, an empty line that starts on it)
  needle        NEEDLE across the boundary, inside field 2
  regex         a match of FIELD_REGEX across the boundary, inside its [a-e]* run in field 1
  behind-tab    the boundary directly behind a tab, NEEDLE right behind it: a match wholly in a later launch than its line

and a run of one-byte streams inside a 40 000-byte line, which therefore runs through whole launches without any
delimiter at every cap and ends three launches behind its start even at cap 64.

The lines are records: a counter, a tab, up to eleven more tab-separated fields over "abcdeABCDE," (some of them hold
ERROR in some case); runs of empty lines; lines of "\\0", "\\xff", commas and tabs; copies of lines hundreds of lines
back and of the line just in front; lines of 9 000 and 40 000 bytes with tabs far apart and MARK in the long ones; an
unterminated tail ("tail"), or the same bytes with a final "\\n" ("closed")."""
import functools
import random
import re

import numpy as np

import datagen
import fieldhash as FH
import fields as F
import grepgen
import linehash as H
import regexgen as G

NL, TAB = 10, 9
NEEDLE = b"ERROR"
MARK = b"xyzzy7"
SIZES = (0, 1, 700, 2_000, 3_000, 4_096, 6_000)
CAPS = (2, 3, 5, 64)
TOTAL = 880_000
RUN_FIRST, RUN_BLOCKS = 3 * 64 - 1, 2 * 64 + 2       # one-byte data blocks 191 .. 320: all of launches 3 and 4 at cap 64
LONG_LINES = ((60_000, 40_000), (130_000, 9_000), (180_000, 40_000), (250_000, 9_000), (300_000, 40_000), (640_000, 40_000),
              (720_000, 9_000), (760_000, 40_000), (840_000, 9_000))     # (due at, bytes); one more lies around the run
ALPHABET = b"abcdeABCDE,"
SEEDS = (0, 1)
VARIANTS = ("tail", "closed")

FIELD_REGEX = rb"^[0-9]+\t[a-e]*,"
REGEX_PATTERNS = (rb"ERROR", rb"^$", rb"\t$", FIELD_REGEX, rb"xyzzy[0-9]", rb"never[0-9]there")
SET_PATTERNS = (NEEDLE, b"err", b"\t\t", b"ab,", b"\xff\x00")
FIELDS = ((0, TAB), (1, TAB), (3, TAB), (7, TAB), (1023, TAB), (1, ord(",")))


def part_sizes(rng):
    """(sizes of the parts, offset of the run of one-byte parts)."""
    sizes, data, at, run_at = [], 0, 0, None
    while at < TOTAL:
        if data == RUN_FIRST and run_at is None:
            run_at = at
            sizes += [1] * RUN_BLOCKS
            data += RUN_BLOCKS
            at += RUN_BLOCKS
        size = rng.choice(SIZES)
        sizes.append(size)
        data += size > 0
        at += size
    return sizes + [700], run_at


def data_block_starts(parts):
    """The decoded offset of every data block: a part of no bytes is a stream without one."""
    starts, at = [], 0
    for part in parts:
        if len(part) > 0:
            starts.append(at)
        at += len(part)
    return starts


def boundaries_of(starts, cap):
    """Where the launches of a whole-file call meet: consecutive groups of `cap` data blocks."""
    return [starts[i] for i in range(cap, len(starts), cap)]


def launches_of(starts, size, cap):
    """[(offset, end)] of those launches."""
    edges = [0] + boundaries_of(starts, cap) + [size]
    return list(zip(edges, edges[1:]))


def choose_targets(sizes, run_at):
    """{offset: kind}: the boundaries that get a planted case, clear of the long lines and of one another; and the long
    lines as [(offset at which one is due, length)]."""
    starts, at = [], 0
    for size in sizes:
        if size > 0:
            starts.append(at)
        at += size
    longs = [(run_at - 20_000, 40_000)]
    reserved = [(run_at - 21_000, run_at + 22_000), (0, 3_000), (at - 3_000, at)]
    targets = {}

    def take(candidates, kind):
        for b in candidates:
            if all(not lo <= b <= hi for lo, hi in reserved):
                targets[b] = kind
                reserved.append((b - 1_000, b + 1_000))
                return
        raise AssertionError("no boundary left for %s" % kind)

    def take_all(cap, kinds):
        candidates = boundaries_of(starts, cap)
        for i, kind in enumerate(kinds):
            # spread over the file: each kind looks from its own share of the boundaries on
            take(candidates[i * len(candidates) // len(kinds):] + candidates, kind)

    # cap 64 has few boundaries, and the run holds three of them: they come first, and the long lines give way
    take_all(64, ("needle", "regex", "behind-tab", "both-nl"))
    for due, length in LONG_LINES:
        while any(lo <= due + length + 2_000 and due - 1_000 <= hi for lo, hi in reserved):
            due += 1_000
        longs.append((due, length))
        reserved.append((due - 1_000, due + length + 2_000))
    for cap in (5, 3, 2):
        take_all(cap, ("behind-nl", "before-nl", "needle", "regex", "behind-tab"))
    # streams that are exactly b"\n"
    ones = [start for start, size in zip(np.cumsum([0] + sizes[:-1]).tolist(), sizes) if size == 1]
    for i in range(6):
        take(ones[i * len(ones) // 6:] + ones, "before-nl")
    return targets, sorted(longs)


@functools.lru_cache(maxsize=None)
def corpus(variant="tail", seed=0x5AFE):
    """(raw, enc, parts)."""
    assert variant in VARIANTS
    rng = random.Random(seed)
    sizes, run_at = part_sizes(rng)
    total = sum(sizes)
    targets, longs = choose_targets(sizes, run_at)
    targets = sorted(targets.items())
    out, lines = bytearray(), []                 # lines: the content of every line so far, None for those too long to copy

    def emit(content):
        out.extend(content + b"\n")
        lines.append(content if len(content) <= 600 else None)

    def fill(n, alphabet=ALPHABET):
        return bytes(rng.choices(alphabet, k=n))

    def head():
        return b"%d\t" % len(lines)

    def field():
        if rng.random() < 0.03:
            return rng.choice([NEEDLE, b"error", b"Error", b"an " + NEEDLE + b",x"])
        return fill(rng.randrange(12))

    def long_line(n):
        line = bytearray(fill(n, b"fghijklm \0\xff"))
        for k in (5, n // 3, n // 3 + 1, n - 2_000):
            line[k] = TAB
        if n > 10_000:
            line[n - 9_000:n - 9_000 + len(MARK)] = MARK
        return bytes(line)

    def random_lines(limit):
        """Lines of at most `limit` bytes together, delimiters included (limit >= 60)."""
        kind = rng.randrange(12)
        if kind == 0:
            return [b""] * rng.randrange(1, 5)
        if kind == 1:
            return [fill(rng.randrange(1, 600), b"ab\0\xff,\t")[:limit - 1]]
        if kind == 2 and len(lines) > 400:
            copy = lines[-rng.randrange(300, min(len(lines), 3_000))]
            if copy is not None and len(copy) < limit:
                return [copy]
        if kind == 3 and lines and lines[-1] is not None and len(lines[-1]) < limit:
            return [lines[-1]]
        return [(head() + b"\t".join(field() for _ in range(rng.randrange(12))))[:limit - 1]]

    def craft(b, kind):
        """The line(s) that put `kind` on offset b, from a line start 60 to 300 bytes in front of it."""
        room, h = b - len(out), head()
        if kind == "behind-nl":
            emit(h + fill(room - 1 - len(h)))
        elif kind == "before-nl":
            emit(h + fill(room - len(h)))
        elif kind == "both-nl":
            emit(h + fill(room - 1 - len(h)))
            emit(b"")
        elif kind == "needle":
            emit(h + b"ab\t" + fill(room - 2 - len(h) - 3) + NEEDLE + b"x\tend")
        elif kind == "regex":
            emit(h + fill(room - len(h) + 7, b"abcde") + b",x\tend")
        elif kind == "behind-tab":
            emit(h + fill(room - len(h) - 1) + b"\t" + NEEDLE + b"\tend")

    while True:
        at = len(out)
        if longs and at >= longs[0][0]:
            emit(long_line(longs.pop(0)[1]))
            continue
        room = (targets[0][0] if targets else total) - at
        if room <= 300:
            if not targets:
                break
            craft(*targets.pop(0))
            continue
        for content in random_lines(min(600, room - 60)):
            emit(content)
    room = total - len(out)
    assert 60 <= room <= 300 and not longs
    out.extend((b"the\ttail has\tno newline,\tbut an " + NEEDLE + b" " + fill(room))[:room - 1] + (b"e" if variant == "tail" else b"\n"))
    raw = bytes(out)
    parts, at = [], 0
    for size in sizes:
        parts.append(raw[at:at + size])
        at += size
    assert at == len(raw) == total
    assert raw.find(b"\n", run_at - 10_000) - raw.rfind(b"\n", 0, run_at - 10_000) == 40_001       # the run lies in a long line
    assert b"\n" not in raw[run_at - 10_000:run_at + RUN_BLOCKS + 10_000]
    return raw, datagen.multistream(parts, 1), tuple(parts)


@functools.lru_cache(maxsize=None)
def planted(seed=0x5AFE):
    """({offset: kind} of the planted cases, offset of the run of one-byte streams): the same for both variants."""
    sizes, run_at = part_sizes(random.Random(seed))
    return choose_targets(sizes, run_at)[0], run_at


def reference_regex(raw, pattern, ignore_case=False):
    """(numbers, lines) of the lines Python's re finds a match in, as test_gpu_regex.reference."""
    compiled = re.compile(pattern, G.reference_flags(ignore_case))
    numbers, lines = [], []
    for k, (at, content) in enumerate(G.split_lines(raw)):
        if compiled.search(content):
            numbers.append(k)
            lines.append(raw[at:at + len(content) + 1])
    return numbers, lines


def first_occurrences_of(lines):
    seen, numbers = {}, []
    for k, content in enumerate(lines):
        if content not in seen:
            seen[content] = k
            numbers.append(k)
    return numbers


def groups_of(values, first=0, count=None):
    """Lines [first, first + count) of `values` (one field per line, None where it is missing) grouped by value, as
    count_by_field and value_counts return them -> (lines, counts, missing, ranked): the number of the first line of every
    distinct value in first-occurrence order, how many lines of the range hold it, the number of lines without the field,
    and [(value, count)] by descending count, then by first occurrence."""
    last = len(values) if count is None else min(len(values), first + count)
    firsts, tally, missing = {}, {}, 0
    for k in range(min(first, last), last):
        value = values[k]
        if value is None:
            missing += 1
        else:
            firsts.setdefault(value, k)
            tally[value] = tally.get(value, 0) + 1
    order = sorted(firsts, key=firsts.get)
    ranked = sorted(((value, tally[value]) for value in order), key=lambda item: (-item[1], firsts[item[0]]))
    return [firsts[value] for value in order], [tally[value] for value in order], missing, ranked


@functools.lru_cache(maxsize=None)
def expected(variant="tail"):
    """What the reader must answer for a variant, from the models and the standard library alone; computed once per
    process, shared, never changed by a test."""
    raw, enc, parts = corpus(variant)
    lines = F.lines_of(raw, NL)
    newlines = grepgen.newline_positions(raw)
    return {
        "raw": raw, "enc": enc, "parts": parts,
        "block_starts": data_block_starts(parts),
        "newlines": newlines,
        "line_starts": grepgen.line_starts_of(raw),                 # s(0) .. s(N): N + 1 offsets, the tail's included
        "lines": lines,                                             # as line_hashes and field_spans number them
        "hashes": {seed: H.direct(raw, NL, seed) for seed in SEEDS},
        "first_occurrences": first_occurrences_of(lines),
        "spans": {(j, dl): F.direct(raw, NL, dl, j) for j, dl in FIELDS},
        "field3": F.fields_of(raw, NL, TAB, 3),
        "values": {(j, dl): F.fields_of(raw, NL, dl, j) for j, dl in FIELDS},
        "keys": {(j, dl, seed): FH.keys_of(raw, NL, dl, j, seed) for j, dl in FIELDS for seed in SEEDS},
        "groups": {(j, dl): groups_of(F.fields_of(raw, NL, dl, j)) for j, dl in FIELDS},
        "regex": {(pattern, fold): reference_regex(raw, pattern, fold) for pattern in REGEX_PATTERNS for fold in (False, True)},
    }
