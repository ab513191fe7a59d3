"""The texts of the quoted-field tests, shared by test_fieldsquoted_plan.py (the corpus' conditions, on the CPU) and
test_gpu_fields_quoted.py.  Nothing here touches the code under test.

record() is one line of comma-separated cells, some quoted, with delimiters and doubled quotes inside, some with lone and
unbalanced quotes.  reader_corpus() is about 90 kB of such lines cut into tiny bzip2 streams as readershapes.py cuts its
corpus, written around the launch boundaries the cut gives so that, for every cap of CAPS, a boundary lies directly behind
an opening quote, directly in front of a closing quote, between the two quotes of a doubled quote and on a delimiter inside
quotes; a run of one-byte streams lies inside a quoted field of 6 000 bytes; and the last line is open inside a quote."""
import functools
import random

import datagen
import readershapes as R

NL, DL, QT = 10, ord(","), ord('"')


def quoted_cell(rng, n):
    """A quoted field of n bytes between its quotes: commas, doubled quotes and letters."""
    out = bytearray()
    while len(out) < n:
        token = rng.choice([b",", b",", b'""', b"a", b"bc", b" "])
        out += token if len(out) + len(token) <= n else b"a"
    return b'"' + bytes(out) + b'"'


def record(rng):
    cells = []
    for _ in range(rng.choice([0, 1, 1, 2, 3, 5, 8])):
        kind = rng.randrange(10)
        if kind < 4:
            cells.append(bytes(rng.choice(b"abcxyz \0\xff") for _ in range(rng.randrange(9))))
        elif kind < 7:
            cells.append(quoted_cell(rng, rng.randrange(12)))
        elif kind == 7:
            cells.append(b'""')
        elif kind == 8:
            cells.append(quoted_cell(rng, rng.randrange(40, 400)))
        else:
            cells.append(rng.choice([b'"', b'a"', b'"a', b'"a"b', b'a"b"', b'""""']))     # lone and unbalanced quotes too
    return b",".join(cells)


CAPS = (2, 3, 5)
KINDS = ("behind-open", "before-close", "in-doubled", "dl-inside")
PART_SIZES = (0, 1, 400, 1_000, 2_500)
TOTAL, RUN, LONG = 90_000, 13, 6_000
FIELDS = (0, 1, 2, 5)


def reader_parts(rng):
    """(sizes of the parts, offset of the run of one-byte parts): readershapes' cutting, smaller."""
    sizes, at, run_at = [], 0, None
    while at < TOTAL:
        if at >= 30_000 and run_at is None:
            run_at = at
            sizes += [1] * RUN
            at += RUN
        size = rng.choice(PART_SIZES)
        sizes.append(size)
        at += size
    return sizes + [700], run_at


def reader_targets(sizes, run_at):
    """{offset: kind}: for every cap of CAPS and every kind a launch boundary of that cap, clear of the others, of the long
    quoted field around the run and of both ends."""
    starts = R.data_block_starts([b"x" * size for size in sizes])
    reserved = [(run_at - LONG, run_at + LONG), (0, 2_000), (sum(sizes) - 2_000, sum(sizes))]
    targets = {}
    for cap in CAPS:
        candidates = R.boundaries_of(starts, cap)
        for i, kind in enumerate(KINDS):
            for b in candidates[i * len(candidates) // len(KINDS):] + candidates:
                if all(not lo <= b <= hi for lo, hi in reserved):
                    targets[b] = kind
                    reserved.append((b - 700, b + 700))
                    break
            else:
                raise AssertionError("no boundary left for %s at cap %d" % (kind, cap))
    return targets


@functools.lru_cache(maxsize=None)
def reader_corpus(variant):
    """(raw, enc, {offset: kind}, run_at, parts)."""
    rng = random.Random(0x0C5F)
    sizes, run_at = reader_parts(rng)
    total = sum(sizes)
    planted = reader_targets(sizes, run_at)
    targets = sorted(planted.items())
    out, count = bytearray(), 0

    def emit(content):
        nonlocal count
        out.extend(content + b"\n")
        count += 1

    def fill(n):
        return bytes(rng.choices(b"abcdeABCDE ", k=n))

    def inner(n):
        return bytes(rng.choices(b"abc,,, ", k=n))

    def craft(b, kind):
        room, h = b - len(out), b"%d," % count
        if kind == "behind-open":                                   # the opening quote is the last byte in front of b
            emit(h + fill(room - len(h) - 2) + b',"' + inner(40) + b'",end')
        elif kind == "before-close":                                # the closing quote is the byte at b
            emit(h + fill(5) + b',"' + inner(room - len(h) - 7) + b'",end')
        elif kind == "in-doubled":                                  # b lies between the two quotes of a ""
            emit(h + fill(5) + b',"' + inner(room - len(h) - 8) + b'""' + inner(30) + b'",end')
        elif kind == "dl-inside":                                   # the byte at b is a delimiter inside quotes
            emit(h + fill(5) + b',"' + inner(room - len(h) - 7) + b"," + inner(30) + b'",end')

    long_due = run_at - LONG // 2
    while True:
        at = len(out)
        if long_due is not None and at >= long_due - 300:
            emit(b"%d,%s," % (count, fill(3)) + b'"' + inner(LONG) + b'"' + b",behind,the run")
            long_due = None
            continue
        room = (targets[0][0] if targets else total) - at
        if room <= 300:
            if not targets:
                break
            craft(*targets.pop(0))
            continue
        line = b"%d," % count + record(rng)
        emit(line[:room - 61] if len(line) > room - 61 else line)
    room = total - len(out)
    assert 60 <= room <= 300 and long_due is None
    tail = (b'the,tail,"is open, inside, a quote, ' + inner(room))[:room - 1]
    out.extend(tail + (b"e" if variant == "tail" else b"\n"))
    raw = bytes(out)
    assert len(raw) == total
    parts, at = [], 0
    for size in sizes:
        parts.append(raw[at:at + size])
        at += size
    return raw, datagen.multistream(parts, 1), planted, run_at, parts
