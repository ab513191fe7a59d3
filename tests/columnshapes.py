"""A corpus of hundreds of tiny blocks with numeric and keyed seams planted, shared by test_columnshapes_corpus.py (its
conditions, on the CPU) and test_gpu_column_shapes.py (field_ints, sum_by_field, read_columns, where_field and
select_lines in every launch shape).  Nothing here touches the code under test.

About 250 kB of records, cut into consecutive parts of 0, 1, 300, 700, 1 500 or 2 500 bytes, each part a bzip2 stream of its
own, as readershapes.py does it: the part sizes are drawn first, and the text is then written line by line around the
launch boundaries they give (launches of a whole-file call are consecutive groups of `cap` data blocks).  A line is a record

    counter TAB key TAB value TAB filler TAB end<counter>

-- the key from a vocabulary of about 40 values with heavy repeats (b"", GE, GET, GETS, bytes of 0x80 and above, one key
of exactly 256 bytes), the value a number of 1 to 18 digits with or without a sign, or something that is none (empty, "-",
"+", "1.5", "12 ", 19 digits), 0 to 200 bytes of filler --, among them lines cut short, lines of filler alone, empty lines,
twelve values of 10^18 - 1 under the key BIG and twelve of its negative under NEG (both sums leave int64), and one line
with a filler of 9 000 bytes.  `counter` is the number of the line, so field 0 and field 4 are unique to their line.

Planted exactly on launch boundaries (`|`), each kind once for each cap in PLANT_CAPS and some of them on boundaries of
cap 64 (KINDS_AT_64):

  digits-18     ...TAB 123456789|012345678 TAB...   18 digits, both sides at least 2: the 18-digit number
  digits-19     19 digits, each side at most 18: NOT_A_NUMBER, though each half alone is a number
  sign          -|18 digits: the negative number, a text of 19 bytes
  sign-20       - and 19 digits, cut inside: NOT_A_NUMBER, the text saturates at 20
  value-begins  the boundary directly behind the tab in front of the value: the head text begins the field
  value-ends    the boundary directly in front of the tab behind the value: the carried text is the whole field
  garbage       123|x4: NOT_A_NUMBER, though the front half alone is a number
  key           GE|T as key
  key-miss      GET|S as key
  key-empty     the boundary between the two tabs around an empty key
  last-value    a line `counter TAB key TAB value` with the boundary directly in front of its "\\n"
  last-value-behind   ... with the boundary directly behind its "\\n": the next line starts on it

and one line of about 20 000 bytes around a run of RUN_BLOCKS one-byte streams that starts at data block RUN_FIRST: inside
the run lie the last 4 bytes of the 256-byte key, a tab, a value of 19 bytes ("-" and 18 digits), a tab and filler to the
end of the run.  At parallelization 1 every byte of that number is a launch of its own, the boundaries of caps 2, 3, 5 and
64 all cut it, and at caps 2, 3 and 5 several launches behind it hold no delimiter at all.

The last-value lines have no field 4: field 0, the counter, names them."""
import functools
import random

import numpy as np

import datagen
import fieldcols as FC
import fieldhash as FH
import fieldmatch as FM
import fieldnum as FN
import fields as F
import grepgen
import linehash as H
from readershapes import boundaries_of, data_block_starts, groups_of, launches_of           # noqa: F401 (shared with the tests)

NL, TAB = 10, 9
SIZES = (0, 1, 300, 700, 1_500, 2_500)
TOTAL = 250_000
PLANT_CAPS = (2, 3, 5)
CAPS = PLANT_CAPS + (64,)
RUN_FIRST, RUN_BLOCKS = 2 * 64 - 10, 80
RUN_LINE = 20_000                                    # bytes of the line around the run, about
LONG_FILLER = (30_000, 9_000)                        # (due at, bytes of filler)
VARIANTS = ("tail", "closed")
KINDS = ("digits-18", "digits-19", "sign", "sign-20", "value-begins", "value-ends", "garbage", "key", "key-miss", "key-empty",
         "last-value", "last-value-behind")
KINDS_AT_64 = ("digits-18", "key", "sign")           # the third only where a third boundary of cap 64 is free
ALPHABET = b"abcdefgh ,.;"
KEY256 = bytes(65 + (7 * i + i // 26) % 26 for i in range(252)) + b"Zq9!"
HIGH = b"\x80\xfe\xff"
BIG, NEG = b"BIG", b"NEG"
NUMBER_MAX = 10**18 - 1
VOCABULARY = (b"", b"GE", b"GET", b"GETS", HIGH, KEY256, b"PUT", b"POST", b"DELETE", b"HEAD") + tuple(b"k%02d" % i for i in range(30))
WEIGHTS = (30, 25, 200, 25, 25, 12, 90, 50, 20, 10) + tuple(40 // (i + 1) + 1 for i in range(30))
FIELDS = (0, 1, 2, 3, 4)
NUMBER_FIELDS = (0, 2, 4, 1023)
SUMS = ((1, 2), (1, 0))

# the predicates of the GPU tests: {name: (field, values, between)}
SET_30 = tuple(b"k%02d" % i for i in range(26)) + (b"PUT", b"POST", b"DELETE", HIGH)
PREDICATES = {
    "get": (1, (b"GET",), None),
    "ge-get-empty": (1, (b"GE", b"GET", b""), None),
    "key256": (1, (KEY256,), None),
    "set30": (1, SET_30, None),
    "never": (1, (b"never",), None),
    "small": (2, None, (-5, 10**17)),
    "negative": (2, None, (None, -1)),
    "largest": (2, None, (NUMBER_MAX, None)),
    "empty-range": (2, None, (5, 4)),
}


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


def run_line_bounds(run_at):
    """(offset of the line around the run, offset of its "\\n"): the key's last 4 bytes are the run's first."""
    start = run_at - 252 - 1 - 6                     # a counter of 6 bytes at the most, a tab, 252 bytes of the key
    return start, start + RUN_LINE


def choose_targets(sizes, run_at):
    """{offset: kind}: the boundaries that get a planted case, clear of the long lines and of one another."""
    starts, at = [], 0
    for size in sizes:
        if size > 0:
            starts.append(at)
        at += size
    run_start, run_end = run_line_bounds(run_at)
    reserved = [(run_start - 700, run_end + 700), (0, 1_500), (at - 1_500, at), (LONG_FILLER[0] - 700, sum(LONG_FILLER) + 1_500)]
    targets = {}

    def take(candidates, kind):
        for b in candidates:
            if all(not lo <= b <= hi for lo, hi in reserved):
                targets[b] = kind
                reserved.append((b - 700, b + 700))
                return True
        return False

    def take_all(cap, kinds, required):
        candidates = boundaries_of(starts, cap)
        for i, kind in enumerate(kinds):
            # spread over the file: each kind looks from its own share of the boundaries on
            found = take(candidates[i * len(candidates) // len(kinds):] + candidates, kind)
            assert found or i >= required, "no boundary of cap %d left for %s" % (cap, kind)

    take_all(64, KINDS_AT_64, 2)                     # cap 64 has few boundaries, and the run holds two of them: they come first
    for cap in (5, 3, 2):
        take_all(cap, KINDS, len(KINDS))
    return targets


@functools.lru_cache(maxsize=None)
def corpus(variant="tail", seed=0xC0157):
    """(raw, enc, parts)."""
    assert variant in VARIANTS
    rng = random.Random(seed)
    sizes, run_at = part_sizes(rng)
    total = sum(sizes)
    targets = sorted(choose_targets(sizes, run_at).items())
    run_start, run_end = run_line_bounds(run_at)
    specials = sorted([(run_start, "run"), (LONG_FILLER[0], "long")])
    out, count = bytearray(), [0]
    big = [BIG] * 12 + [NEG] * 12

    def emit(content):
        out.extend(content + b"\n")
        count[0] += 1

    def fill(n):
        return bytes(rng.choices(ALPHABET, k=n))

    def digits(n):
        return b"%d" % rng.randrange(1, 10) + b"".join(b"%d" % rng.randrange(10) for _ in range(n - 1))

    def head():
        return b"%d\t" % count[0]

    def end():
        return b"\tend%d" % count[0]

    def value():
        kind = rng.randrange(10)
        if kind == 0:
            return rng.choice([b"", b"-", b"+", b"1.5", b"12 ", digits(19), b"-" + digits(19)])
        return rng.choice([b"", b"", b"-", b"+"]) + b"%d" % rng.randrange(10 ** rng.randrange(1, 19))

    def record(limit):
        """One or more lines of at most `limit` bytes together, delimiters included (limit >= 60)."""
        kind = rng.randrange(40)
        if kind == 0:
            return [b""] * rng.randrange(1, 4)
        if kind == 1:
            return [fill(rng.randrange(1, 120))[:limit - 1]]
        if kind == 2:
            return [(head() + rng.choice(VOCABULARY[:5]))[:limit - 1]]
        if kind == 3:
            return [(head() + rng.choice(VOCABULARY[:5]) + b"\t" + value())[:limit - 1]]
        if kind in (4, 5) and big:
            key = big.pop()
            return [head() + key + b"\t" + (b"-" if key == NEG else rng.choice([b"", b"+"])) + b"%d" % NUMBER_MAX + b"\t\t" + end()[1:]]
        key = rng.choices(VOCABULARY, WEIGHTS)[0]
        return [(head() + key + b"\t" + value() + b"\t" + fill(rng.randrange(201)) + end())[:limit - 1]]

    def craft(b, kind):
        """A line of filler that ends where the crafted line must start, then the line(s) that put `kind` on offset b."""
        at, n = len(out), count[0] + 1               # the crafted line's number: one line of padding comes first
        h = b"%d\t" % n
        key = rng.choice([b"PUT", b"k03", b"", b"GET"])
        rest = b"\t" + fill(rng.randrange(4, 120)) + b"\tend%d" % n
        a, c = rng.randrange(2, 17), rng.randrange(1, 19)
        front, behind = {
            "digits-18": (h + key + b"\t" + digits(a), digits(18 - a) + rest),
            "digits-19": (h + key + b"\t" + digits(c), digits(19 - c) + rest),
            "sign": (h + key + b"\t-", digits(18) + rest),
            "sign-20": (h + key + b"\t-" + digits(a), digits(19 - a) + rest),
            "value-begins": (h + key + b"\t", rng.choice([b"-", b"+", b""]) + digits(rng.randrange(2, 19)) + rest),
            "value-ends": (h + key + b"\t" + rng.choice([b"-", b""]) + digits(rng.randrange(2, 19)), rest),
            "garbage": (h + key + b"\t123", b"x4" + rest),
            "key": (h + b"GE", b"T\t" + digits(3) + rest),
            "key-miss": (h + b"GET", b"S\t" + digits(3) + rest),
            "key-empty": (h, b"\t" + digits(3) + rest),
            "last-value": (h + key + b"\t" + digits(rng.randrange(1, 19)), b""),
            "last-value-behind": (h + key + b"\t-" + digits(rng.randrange(1, 19)) + b"\n", None),
        }[kind]
        emit(fill(b - at - len(front) - 1))
        assert count[0] == n
        if behind is None:                           # the line's own "\n" is the byte in front of the boundary
            emit(front[:-1])
        else:
            emit(front + behind)

    def special(kind):
        if kind == "long":
            emit(head() + b"GET\t77\t" + fill(LONG_FILLER[1]) + end())
            return
        h = b"%d\t" % (count[0] + 1)                 # one line of padding comes first
        assert len(h) <= 7 and len(out) <= run_start, "the line around the run starts too late"
        emit(fill(run_at - 252 - len(h) - len(out) - 1))           # ... so that the key's last 4 bytes are the run's first
        assert h == head() and len(out) + len(h) + 252 == run_at
        line = h + KEY256 + b"\t-" + digits(18) + b"\t"
        tail = end()
        emit(line + fill(run_end - len(out) - len(line) - len(tail)) + tail)
        assert len(out) == run_end + 1

    while True:
        at = len(out)
        room = min([targets[0][0] if targets else total] + [due for due, _ in specials[:1]]) - at
        if specials and specials[0][0] - at <= 300 and (not targets or specials[0][0] <= targets[0][0]):
            special(specials.pop(0)[1])
            continue
        if room <= 300:
            if not targets:
                break
            craft(*targets.pop(0))
            continue
        for content in record(min(600, room - 60)):
            emit(content)
    room = total - len(out)
    assert 60 <= room <= 300 and not specials and not big
    last = b"%d\tGET\t-42\t" % count[0]
    out.extend(last + fill(room - len(last) - 8 - 1) + b"\tendtail" + (b"e" if variant == "tail" else b"\n"))
    raw = bytes(out)
    parts, at = [], 0
    for size in sizes:
        parts.append(raw[at:at + size])
        at += size
    assert at == len(raw) == total
    return raw, datagen.multistream(parts, 1), tuple(parts)


@functools.lru_cache(maxsize=None)
def planted(seed=0xC0157):
    """({offset: kind} of the planted cases, offset of the run of one-byte streams): the same for both variants."""
    sizes, run_at = part_sizes(random.Random(seed))
    return choose_targets(sizes, run_at), run_at


def flags_of(raw, name):
    j, values, between = PREDICATES[name]
    return FM.flags_of(raw, NL, TAB, j, values, between, number=FN.number)


@functools.lru_cache(maxsize=None)
def expected(variant="tail"):
    """What the reader must answer for a variant, from the models and the standard library alone; computed once per
    process, shared, never changed by a test."""
    raw, enc, parts = corpus(variant)
    return {
        "raw": raw, "enc": enc, "parts": parts,
        "block_starts": data_block_starts(parts),
        "newlines": grepgen.newline_positions(raw),
        "line_starts": grepgen.line_starts_of(raw),                 # s(0) .. s(N): N + 1 offsets, the tail's included
        "lines": F.lines_of(raw, NL),                               # as field_ints and read_columns number them
        "whole_lines": FM.lines_with_delimiters(raw, NL),           # as select_lines returns them
        "words": {j: FN.words_of(raw, NL, TAB, j) for j in NUMBER_FIELDS},
        "fields": {j: F.fields_of(raw, NL, TAB, j) for j in FIELDS},
        "sums": {pair: FN.group_sums(raw, NL, TAB, *pair) for pair in SUMS},
        "columns": {j: FC.column(raw, NL, TAB, j) for j in FIELDS},
        "flags": {name: flags_of(raw, name) for name in PREDICATES},
        "hashes": H.direct(raw, NL, 0),                             # of the old calls the call orders mix in
        "keys": FH.keys_of(raw, NL, TAB, 1, 0),
    }


# ------------------------------------------------------------------------------------------------ blocks for the failures

def data_blocks(e):
    """[(decoded start, decoded end, newlines inside)] of the data blocks of expected(...)."""
    edges, newlines = e["block_starts"] + [len(e["raw"])], e["newlines"]
    return [(a, b, int(np.searchsorted(newlines, b) - np.searchsorted(newlines, a))) for a, b in zip(edges, edges[1:])]


def block_for_damage(e):
    """d, nearest the middle of the file: blocks d - 1, d and d + 1 have at least 1 500 bytes and 6 lines, d + 2 ends at
    least one line, and the boundaries in front of d - 1 and d + 2 lie inside lines -- the one across the latter begins
    behind block d."""
    raw, blocks = e["raw"], data_blocks(e)

    def fits(d):
        if not all(blocks[k][1] - blocks[k][0] >= 1_500 and blocks[k][2] >= 6 for k in (d - 1, d, d + 1)):
            return False
        if blocks[d + 2][2] < 1:
            return False
        front, behind = blocks[d - 1][0], blocks[d + 2][0]
        return raw[front - 1] != NL and raw[behind - 1] != NL and raw.rfind(b"\n", 0, behind) >= blocks[d][1]

    good = [d for d in range(3, len(blocks) - 3) if fits(d)]
    return min(good, key=lambda d: abs(blocks[d][0] - len(raw) // 2))


def block_for_lie(e):
    """b with blocks b - 1, b and b + 1 each of at least 1 500 bytes and 8 lines, behind the first quarter of the file."""
    blocks = data_blocks(e)
    return next(b for b in range(len(blocks) // 4, len(blocks) - 2)
                if all(blocks[k][2] >= 8 and blocks[k][1] - blocks[k][0] >= 1_500 for k in (b - 1, b, b + 1)))
