"""Seeded text and plain-Python expectations shared by the grep / line-number tests (test_gpu_grep.py and its child
process).  Nothing here touches the code under test: every expected value comes from the raw bytes with numpy or plain
Python.

The text has the shape of the line tests' corpus: lines of random length 0-400 up to 6 MB, ONE 3.5 MB line of random
printable bytes in the middle (dozens of level-1 blocks hold no newline), and an unterminated tail: about 9.5 MB and
30 000 newlines.  plant() then overwrites bytes with a needle -- the line structure stays -- at the places the tests are
about."""
import numpy as np

NL = b"\n"
NEEDLE = b"N33DLE#7"
LINES_BYTES = 6_000_000
LONG_LINE = 3_500_000
TAIL = 173


def make_text(seed=0x62E9):
    r = np.random.default_rng(seed)
    lengths = r.integers(0, 401, LINES_BYTES // 150)
    ends = np.cumsum(lengths + 1)                       # position behind every line's newline
    ends = ends[ends <= LINES_BYTES]
    text = r.integers(32, 127, int(ends[-1]), dtype=np.uint8)
    text[ends - 1] = 10
    half = int(ends[len(ends) // 2])                     # a line start in the middle
    long_line = r.integers(32, 127, LONG_LINE, dtype=np.uint8)
    long_line[-1] = 10
    tail = r.integers(32, 127, TAIL, dtype=np.uint8)     # an unterminated last line
    return np.concatenate([text[:half], long_line, text[half:], tail]).tobytes()


def newline_positions(raw, nl=NL):
    return np.flatnonzero(np.frombuffer(raw, dtype=np.uint8) == nl[0]).astype(np.int64)


def line_starts_of(raw, nl=NL):
    """s(k) for k = 0..N as a numpy array of N + 1 offsets."""
    return np.concatenate([[0], newline_positions(raw, nl) + 1]).astype(np.int64)


def plant(raw, boundaries=(), needle=NEEDLE):
    """The text with the needle written over its bytes: at a line's first bytes, ending just in front of a newline, twice
    in one line, in two consecutive lines, in line 0, in the unterminated tail, inside the longest line, and across every
    offset of `boundaries` (block starts), three bytes in front of it and the rest behind.  Returns (bytes, {place:
    [offsets of the needle]})."""
    out = bytearray(raw)
    s = line_starts_of(raw)
    sizes = np.diff(np.concatenate([s, [len(raw)]]))
    m = len(needle)
    roomy = [int(k) for k in np.flatnonzero(sizes[:-1] >= 6 * m) if k > 0]      # lines with room, not line 0, not the tail
    longest = int(np.argmax(sizes))
    pick = [k for k in roomy if k != longest]
    k_first, k_last, k_twice = pick[10], pick[200], pick[3000]
    roomy_set = set(pick)
    k_pair = next(k for k in pick[5000:] if k + 1 in roomy_set)
    places = {
        "line-start": [int(s[k_first])],
        "before-newline": [int(s[k_last + 1]) - 1 - m],
        "twice": [int(s[k_twice]) + 2, int(s[k_twice]) + 3 * m],
        "consecutive": [int(s[k_pair]) + 1, int(s[k_pair + 1]) + 5],
        "line-0": [1] if sizes[0] >= m + 2 else [],
        "tail": [len(raw) - m - 4],
        "long-line": [int(s[longest]) + LONG_LINE // 2],
        "boundary": [int(b) - 3 for b in boundaries if int(b) >= 3 and NL[0] not in raw[int(b) - 3:int(b) - 3 + m]],
    }
    assert places["line-0"], "the seed gives a first line that is too short"
    for offsets in places.values():
        for p in offsets:
            assert 0 <= p and p + m <= len(raw) and NL[0] not in raw[p:p + m]
            out[p:p + m] = needle
    return bytes(out), places


def matches_of(raw, pattern, start=0, end=None):
    """Every p with raw[p:p + m] == pattern, start <= p and p + m <= end (clipped to the size); overlapping ones included."""
    end = len(raw) if end is None else min(end, len(raw))
    found, p = [], raw.find(pattern, start, end)
    while p >= 0:
        found.append(p)
        p = raw.find(pattern, p + 1, end)
    return found


def line_numbers_of(raw, offsets, nl=NL):
    """L(p) = the number of nl bytes in raw[0:min(p, size)]."""
    positions = newline_positions(raw, nl)
    clipped = np.minimum(np.array([min(int(p), len(raw)) for p in offsets], dtype=np.int64), len(raw))
    return np.searchsorted(positions, clipped, "left").astype(np.uint64)


def grep_of(raw, pattern, start=0, end=None, limit=None, nl=NL):
    """(numbers, lines) by a plain split: the distinct lines that hold the first byte of a match, whole, in order."""
    pieces = raw.split(nl)
    lines = [piece + nl for piece in pieces[:-1]] + [pieces[-1]]      # the tail as it is (possibly empty)
    numbers = sorted({int(k) for k in line_numbers_of(raw, matches_of(raw, pattern, start, end), nl)})
    if limit is not None:
        numbers = numbers[:limit]
    return np.array(numbers, dtype=np.uint64), [lines[k] for k in numbers]
