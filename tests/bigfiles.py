"""Files whose decoded bytes pass 2^32 (far_file) and whose compressed bits pass 2^32 (deep_file), with a plain
reference of their content that never holds it in memory (VirtualRaw) and bzip2's CRC of a concatenation (crc_concat).

Nothing here touches the code under test or the oracle's decoder.  The encoder is CPython's bz2 module.  Every offset --
decoded and in bits -- comes from arithmetic on the way the streams are stitched together:

  * a level-L stream of data without two equal neighbouring bytes has blocks of exactly 100 000 L - 19 bytes (RLE1 leaves such
    data as it is), and a last, shorter one;
  * a stream of at most FULL_BLOCK equal bytes has one block;
  * streams are byte aligned, so a magic at bit b of a stream that has B bytes in front of it lies at bit b + 8 B;
  * the bit offsets inside ONE copy of a stream come from a plain search for the two 48-bit magics (magic_offsets).

The runs (fillers) have byte values of 0x80 and above: no ASCII pattern, folded or not, holds one, and none is a newline.
VirtualRaw asserts both for every question it answers, so everything is computed from the literal parts alone.

The same holds for the four line queries (regex, line hashes, field spans, field hashes): newlines and delimiters come from
the literals alone, a hash over a run comes in closed form (fieldhash.run_part), and a regular expression sees a line that
holds runs with every run cut to RUN_SHRINK bytes.  That last step is exact only under the rule written at
VirtualRaw.regex_lines; FAR_PATTERNS is the list of patterns the tests use, all inside it.

For the encoder (at the end): far_pieces(), far_file()'s decoded bytes as buffers whose level-9 blocks are ONE launch with
more than 2^32 bytes of input, deep_input(), incompressible bytes whose stream passes 2^32 bits, and the launch planner of
csrc/bz2_compress.hpp restated in Python (plan_blocks, block_bytes, plan_launches)."""
import bisect
import bz2
import functools
import re

import numpy as np

import datagen
import fieldhash
import fields
import linehash

MAGIC_BLOCK = 0x314159265359
MAGIC_EOS = 0x177245385090
FULL_BLOCK = 45_899_235          # the largest run of one byte that libbz2 puts into one level-9 block: 179 997 x 255
CUT = 1 << 32
FILLER_VALUES = (0x81, 0x93, 0xA5, 0xB7, 0xC9, 0xDB, 0xED)      # period 7: divides neither 93 nor 94 (fillers per 2^32)
CRC_POLY = 0x104C11DB7           # bzip2's CRC-32, MSB first, with the x^32 term


# --------------------------------------------------------------------------------------------------- CRC of a concatenation

def _gf_mulmod(a, b):
    """a * b in GF(2)[x] modulo the CRC polynomial; bit k = x^k."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> 32:
            a ^= CRC_POLY
    return r


def x_pow(e):
    """x^e modulo the CRC polynomial for any non-negative Python integer e (square and multiply)."""
    result, base = 1, 2
    while e:
        if e & 1:
            result = _gf_mulmod(result, base)
        base = _gf_mulmod(base, base)
        e >>= 1
    return result


def crc_concat(crc_a, crc_b, len_b):
    """bzip2's CRC (initial value 0xFFFFFFFF, final inversion) of A + B from crc(A), crc(B) and len(B).  With the raw
    register r(M) = crc(M) ^ 0xFFFFFFFF: r(A + B) = r(A) x^(8|B|) + r(B) + 0xFFFFFFFF x^(8|B|), the last term taking back
    the initial value that r(B) carries."""
    shift = x_pow(8 * len_b)
    raw = _gf_mulmod(crc_a ^ 0xFFFFFFFF, shift) ^ (crc_b ^ 0xFFFFFFFF) ^ _gf_mulmod(0xFFFFFFFF, shift)
    return raw ^ 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------ plain helpers

def magic_offsets(enc, magic):
    """Bit offsets of a 48-bit magic in enc, ascending: for each of the eight bit phases, the byte string that starts at
    that phase is compared with the magic's six bytes (plain numpy; as datagen._block_offsets, for either magic)."""
    a = np.frombuffer(bytes(enc) + b"\0", dtype=np.uint8).astype(np.uint16)
    want = magic.to_bytes(6, "big")
    found = []
    if len(enc) < 6:
        return found
    pairs = (a[:-1] << 8) | a[1:]
    for phase in range(8):
        shifted = ((pairs >> (8 - phase)) & 0xFF).astype(np.uint8)      # the 8 bits from bit 8 i + phase
        n = len(shifted) - 5
        hit = shifted[:n] == want[0]
        for k in range(1, 6):
            hit &= shifted[k:n + k] == want[k]
        found += [8 * int(i) + phase for i in np.flatnonzero(hit) if 8 * int(i) + phase + 48 <= 8 * len(enc)]
    return sorted(found)


def break_runs(data):
    """data (uint8 array) with every byte that equals the one in front of it changed to one that differs from both its
    neighbours (printable stays printable, never a newline).  libbz2 closes a block when it holds 100 000 L - 19 bytes, but
    only between runs: with no two equal neighbours every block but the last holds exactly that."""
    a = np.array(data, dtype=np.uint8)
    for i in np.flatnonzero(a[1:] == a[:-1]) + 1:
        if a[i] != a[i - 1]:
            continue
        after = int(a[i + 1]) if i + 1 < len(a) else -1
        c = int(a[i])
        while c == a[i - 1] or c == after or c == 10:
            c = 33 + (c - 33 + 7) % 90 if a[i] < 128 else 128 + (c - 128 + 7) % 128
        a[i] = c
    assert not np.any(a[1:] == a[:-1])
    return a


class VirtualRaw:
    """The decoded bytes as a list of parts: (value, length) is a run of one byte, a bytes object is itself."""

    MATERIALISE_MAX = 64 << 20

    def __init__(self, parts):
        self.parts = []          # (offset, run value or None, bytes or None, length)
        at = 0
        for part in parts:
            if isinstance(part, tuple):
                value, length = part
                assert 0x80 <= value <= 0xFF and length > 0
                self.parts.append((at, value, None, length))
                at += length
            else:
                part = bytes(part)
                assert part and max(part) < 0x80
                if self.parts and self.parts[-1][2] is not None:      # literal neighbours are one part: a match may cross
                    start, _, before, _ = self.parts.pop()
                    part, at = before + part, start
                self.parts.append((at, None, part, len(part)))
                at += len(part)
        self.size = at
        self.run_values = {value for _, value, _, _ in self.parts if value is not None}

    def literals(self):
        return [(offset, data) for offset, value, data, _ in self.parts if value is None]

    def slice(self, start, end):
        start, end = max(0, start), min(end, self.size)
        assert end - start <= self.MATERIALISE_MAX, "VirtualRaw.slice is for small pieces"
        out = bytearray()
        for offset, value, data, length in self.parts:
            lo, hi = max(start, offset), min(end, offset + length)
            if lo < hi:
                out += bytes([value]) * (hi - lo) if data is None else data[lo - offset:hi - offset]
        return bytes(out)

    def _no_run_in(self, pattern, ignore_case):
        pattern = bytes(pattern)
        assert len(pattern) > 0 and not self.run_values & set(pattern), "a run value takes part in the pattern"
        return pattern.lower() if ignore_case else pattern

    def find_all(self, pattern, start=0, end=None, ignore_case=False):
        """Every p with raw[p:p + m] == pattern (under bytes.lower() with ignore_case), start <= p and p + m <= end;
        matches that overlap one another all count."""
        pattern = self._no_run_in(pattern, ignore_case)
        end = self.size if end is None else min(end, self.size)
        found = []
        for offset, data in self.literals():
            lo, hi = max(start, offset) - offset, min(end, offset + len(data)) - offset
            if lo >= hi:
                continue
            hay = data.lower() if ignore_case else data
            p = hay.find(pattern, lo, hi)
            while p != -1:
                found.append(offset + p)
                p = hay.find(pattern, p + 1, hi)
        return found

    def newline_offsets(self, newline=b"\n"):
        assert len(newline) == 1 and newline[0] not in self.run_values
        found = [np.uint64(offset) + np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == newline[0]).astype(np.uint64)
                 for offset, data in self.literals()]
        return np.concatenate(found) if found else np.zeros(0, dtype=np.uint64)

    def line_of(self, offset, newline=b"\n"):
        """The number of newlines in [0, min(offset, size))."""
        return int(np.searchsorted(self.newline_offsets(newline), min(offset, self.size), "left"))

    def line_starts(self, newline=b"\n"):
        """s(k) for k = 0 .. N: N newlines give N + 1 lines, the last one possibly empty."""
        return np.concatenate([np.zeros(1, dtype=np.uint64), self.newline_offsets(newline) + np.uint64(1)])

    def line_ranges(self, ranges, newline=b"\n"):
        """[(first, count)] -> [(start, end)] in bytes: lines first .. first + count - 1, their newlines included,
        clipped to the lines there are."""
        starts = [int(s) for s in self.line_starts(newline)] + [self.size]
        n = len(starts) - 1
        return [(starts[min(first, n)], starts[min(first + count, n)]) for first, count in ranges]

    def grep(self, pattern, start=0, end=None, limit=None, newline=b"\n", ignore_case=False):
        """(numbers, [(start, end)]): the distinct lines that hold the first byte of a match, in order, as byte ranges."""
        positions = self.newline_offsets(newline)
        matches = np.array(self.find_all(pattern, start, end, ignore_case), dtype=np.uint64)
        numbers = sorted({int(k) for k in np.searchsorted(positions, matches, "left")})
        if limit is not None:
            numbers = numbers[:limit]
        return numbers, self.line_ranges([(k, 1) for k in numbers], newline)

    # ---------------------------------------------------------------------------------- lines, hashes, fields, regex
    # Lines are numbered as line_hashes, field_spans and grep_regex number them: a non-empty unterminated tail is one
    # more line.  Everything below is arithmetic on the parts; nothing calls the code under test.

    def byte_offsets(self, value):
        """Every offset that holds byte `value` (not a run's), ascending, as a numpy uint64 array; computed once."""
        assert 0 <= value < 256 and value not in self.run_values, "a run value is asked for as a delimiter"
        cache = self.__dict__.setdefault("_byte_offsets", {})
        if value not in cache:
            cache[value] = self.newline_offsets(bytes([value]))
        return cache[value]

    def _within(self, positions, start, end):
        """positions (sorted) inside [start, end), as Python integers."""
        lo, hi = np.searchsorted(positions, np.uint64(start), "left"), np.searchsorted(positions, np.uint64(max(start, end)), "left")
        return [int(p) for p in positions[lo:hi]]

    def line_bounds(self, newline=b"\n"):
        """[(start, end of content)] of every line."""
        cache = self.__dict__.setdefault("_line_bounds", {})
        if newline[0] not in cache:
            cuts = [int(p) for p in self.byte_offsets(newline[0])]
            starts = [0] + [c + 1 for c in cuts]
            bounds = list(zip(starts, cuts))
            if starts[-1] < self.size:
                bounds.append((starts[-1], self.size))
            cache[newline[0]] = bounds
        return cache[newline[0]]

    def _overlapping(self, start, end):
        """The parts that overlap [start, end), clipped: (run value or None, bytes or None, lo, hi, part's offset)."""
        offsets = self.__dict__.setdefault("_part_offsets", [offset for offset, _, _, _ in self.parts])
        out, k = [], max(0, bisect.bisect_right(offsets, start) - 1)
        while k < len(self.parts) and self.parts[k][0] < end:
            offset, value, data, length = self.parts[k]
            lo, hi = max(start, offset), min(end, offset + length)
            if lo < hi:
                out.append((value, data, lo, hi, offset))
            k += 1
        return out

    def holds_run(self, start, end):
        return any(value is not None for value, _, _, _, _ in self._overlapping(start, end))

    def part(self, start, end, x):
        """(h, xl) of bytes [start, end) under base x: literals by linehash (the hashes of a literal's prefixes computed
        once per x), runs in closed form by fieldhash.run_part, joined by linehash.followed_by."""
        prefixes = self.__dict__.setdefault("_prefixes", {})
        out = (0, 1)
        for value, data, lo, hi, offset in self._overlapping(start, min(end, self.size)):
            if data is None:
                piece = fieldhash.run_part(value, hi - lo, x)
            elif hi - lo <= 64:
                piece = linehash.part(data[lo - offset:hi - offset], x)
            else:
                if (data, x) not in prefixes:
                    prefixes[(data, x)] = linehash.Prefix(data, x)
                piece = prefixes[(data, x)].part(lo - offset, hi - offset)
            out = linehash.followed_by(out, piece)
        return out

    def line_hashes(self, newline=b"\n", seed=0):
        """The hash of every line, as Python integers; computed once per (newline, seed)."""
        cache = self.__dict__.setdefault("_line_hashes", {})
        if (newline[0], seed) not in cache:
            x = linehash.base(seed)
            cache[(newline[0], seed)] = [self.part(a, b, x)[0] for a, b in self.line_bounds(newline)]
        return cache[(newline[0], seed)]

    def first_occurrences(self, newline=b"\n", seed=0):
        """The numbers of the lines that are the first of their hash, ascending; their number is the distinct count."""
        seen, numbers = set(), []
        for k, h in enumerate(self.line_hashes(newline, seed)):
            if h not in seen:
                seen.add(h)
                numbers.append(k)
        return numbers

    def hash_summary(self, start, size, newline=b"\n", seed=0):
        """The summary of span [start, start + size) as Decoder.hash_lines returns it, and the hashes of the lines the span
        closes (the first as if the span were entered at a line start) -> (dict, [hashes])."""
        x, end = linehash.base(seed), start + size
        cuts = self._within(self.byte_offsets(newline[0]), start, end)
        starts = [start] + [c + 1 for c in cuts]
        summary = {"head": self.part(start, cuts[0] if cuts else end, x), "tail": self.part(cuts[-1] + 1, end, x) if cuts else (0, 1),
                   "has_delimiter": bool(cuts), "tail_non_empty": size > 0 and (not cuts or cuts[-1] != end - 1), "count": len(cuts)}
        return summary, [self.part(a, b, x)[0] for a, b in zip(starts, cuts)]

    def _field_of(self, a, b, j, delimiters):
        """(start, size) of field j of the line whose content is [a, b): fields.direct's rule."""
        lo = int(np.searchsorted(delimiters, np.uint64(a), "left"))
        n = int(np.searchsorted(delimiters, np.uint64(b), "left")) - lo
        if j > n:
            return (b, -1)
        first = a if j == 0 else int(delimiters[lo + j - 1]) + 1
        return (first, (int(delimiters[lo + j]) if j < n else b) - first)

    def field_spans(self, j, delimiter=b"\t", newline=b"\n"):
        """[(start, size)] of field j of every line: a missing field has size -1 and its start at the end of the content."""
        assert delimiter != newline
        delimiters = self.byte_offsets(delimiter[0])
        return [self._field_of(a, b, j, delimiters) for a, b in self.line_bounds(newline)]

    def field_values(self, j, delimiter=b"\t", newline=b"\n", first=0, count=None):
        """Field j of lines [first, first + count) as bytes, None where it is missing: what read_fields and read_columns
        return, from field_spans (computed once per field) and slice.  For windows whose fields are short."""
        cache = self.__dict__.setdefault("_field_spans", {})
        key = (j, delimiter[0], newline[0])
        if key not in cache:
            cache[key] = self.field_spans(j, delimiter, newline)
        spans = cache[key][first:None if count is None else first + count]
        return [None if size < 0 else self.slice(start, start + size) for start, size in spans]

    def field_keys(self, j, delimiter=b"\t", newline=b"\n", seed=0):
        """The key of field j of every line: its hash, or fieldhash.MISSING."""
        x = linehash.base(seed)
        return [fieldhash.MISSING if n < 0 else self.part(s, s + n, x)[0] for s, n in self.field_spans(j, delimiter, newline)]

    def field_groups(self, j, delimiter=b"\t", newline=b"\n", seed=0, first=0, count=None):
        """Lines [first, first + count) grouped by the key of field j, as count_by_field returns them -> (lines, counts,
        missing, spans): the number of the first line of every distinct value, ascending; how many lines hold it; the
        number of lines without the field; (start, size) of the field in those first lines."""
        keys, spans = self.field_keys(j, delimiter, newline, seed), self.field_spans(j, delimiter, newline)
        last = len(keys) if count is None else min(len(keys), first + count)
        order, tally, missing = [], {}, 0
        for k in range(min(first, last), last):
            if keys[k] == fieldhash.MISSING:
                missing += 1
            elif keys[k] in tally:
                tally[keys[k]][1] += 1
            else:
                tally[keys[k]] = [k, 1]
                order.append(keys[k])
        return [tally[key][0] for key in order], [tally[key][1] for key in order], missing, [spans[tally[key][0]] for key in order]

    def value_counts(self, j, limit=None, delimiter=b"\t", newline=b"\n", seed=0, first=0, count=None):
        """[(value, count)] by descending count, then by first occurrence, at most `limit`: what value_counts returns.
        The values are materialised, so the caller keeps the filler lines out of the chosen groups."""
        lines, counts, _, spans = self.field_groups(j, delimiter, newline, seed, first, count)
        order = sorted(range(len(lines)), key=lambda i: (-counts[i], lines[i]))[:limit]
        return [(self.slice(spans[i][0], spans[i][0] + spans[i][1]), counts[i]) for i in order]

    def field_summary(self, start, size, j, delimiter=b"\t", newline=b"\n"):
        """The summary of span [start, start + size) for field j as Decoder.field_spans returns it (positions relative
        to the span, None where not reached), with "fields": (start, size) of the field in the lines the span closes,
        offsets in the output, the first as if the span were entered at a line start."""
        assert delimiter != newline
        end = start + size
        delimiters = self.byte_offsets(delimiter[0])
        cuts = self._within(self.byte_offsets(newline[0]), start, end)
        starts = [start] + [c + 1 for c in cuts]
        head = [p - start for p in self._within(delimiters, start, cuts[0] if cuts else end)[:j + 1]]
        tail_start = cuts[-1] + 1 if cuts else start
        in_tail = [p - start for p in self._within(delimiters, tail_start, end)[:j + 1]]
        tail = fields.go_on(fields.line_start(j, tail_start - start), j, in_tail, 0)
        return {"count": len(cuts), "has_delimiter": bool(cuts), "first_nl": cuts[0] - start if cuts else None,
                "head_positions": head, "tail_start": tail_start - start, "tail_delims": tail[0], "tail_field_start": tail[1],
                "tail_field_end": tail[2], "tail_non_empty": size > 0 and (not cuts or cuts[-1] != end - 1),
                "fields": [self._field_of(a, b, j, delimiters) for a, b in zip(starts, cuts)]}

    def field_hash_summary(self, start, size, j, delimiter=b"\t", newline=b"\n", seed=0):
        """field_summary with what Decoder.field_hashes adds: head and tail as (h, xl), head_hashes, tail_start_hash and
        tail_end_hash (fieldhash.Text.summary's rule), and "keys" beside "fields"."""
        x, end = linehash.base(seed), start + size
        s = self.field_summary(start, size, j, delimiter, newline)
        s["head"] = self.part(start, start + s["first_nl"] if s["has_delimiter"] else end, x)
        s["tail"] = self.part(start + s["tail_start"], end, x) if s["has_delimiter"] else (0, 1)
        s["head_hashes"] = [self.part(start, start + p, x)[0] for p in s["head_positions"]]
        for name, position in (("tail_start_hash", s["tail_field_start"]), ("tail_end_hash", s["tail_field_end"])):
            s[name] = None if position is None else self.part(start + s["tail_start"], start + position, x)[0]
        s["keys"] = [fieldhash.MISSING if n < 0 else self.part(a, a + n, x)[0] for a, n in s["fields"]]
        return s

    RUN_SHRINK = 4096

    def line_content(self, a, b):
        """The bytes of [a, b) with every run cut to min(length, RUN_SHRINK) bytes: a line without a run is itself."""
        out = bytearray()
        for value, data, lo, hi, offset in self._overlapping(a, b):
            out += bytes([value]) * min(hi - lo, self.RUN_SHRINK) if data is None else data[lo - offset:hi - offset]
        assert len(out) <= self.MATERIALISE_MAX
        return bytes(out)

    def regex_lines(self, pattern, newline=b"\n", ignore_case=False):
        """The numbers of the lines in whose content re.search(pattern, content, re.DOTALL) finds a match.  A line that
        holds runs is searched on line_content's copy, every run cut to RUN_SHRINK = 4096 bytes.  That is exact only for
        patterns in which a filler byte (0x80 and above) is matched by

          * nothing, or
          * `.` or a negated class that stands unrepeated, under `*` or `+`, or under `{m,n}` with n <= 255
            (REGEX_MAX_COUNT): such an atom cannot tell 4096 equal bytes from 45 MB of them, 4096 being more than 255
            plus the length of any pattern used.

        An unbounded group of two or more such atoms, such as `(..)*`, counts the run's length modulo its own and is
        outside the rule.  FAR_PATTERNS keeps to it; test_bigfiles.py runs every one of them against whole and shrunken
        runs alike."""
        cache = self.__dict__.setdefault("_regex_lines", {})
        key = (bytes(pattern), newline[0], bool(ignore_case))
        if key not in cache:
            compiled = re.compile(bytes(pattern), re.DOTALL | (re.IGNORECASE if ignore_case else 0))
            cache[key] = [k for k, (a, b) in enumerate(self.line_bounds(newline)) if compiled.search(self.line_content(a, b))]
        return cache[key]


# ------------------------------------------------------------------------------------------------------------------ texts

NEEDLE_SEED = 0x9EED1E


def needles():
    """{name: bytes}: mixed-case needles of 1, 2, 16, 17 and 256 bytes without newline or run of four, the 2-byte one being
    bytes 99 and 100 of the 256-byte one, and two that overlap themselves."""
    r = datagen.rng(NEEDLE_SEED)
    letters = np.concatenate([np.arange(65, 91), np.arange(97, 123), np.arange(48, 58)])
    long = bytearray(break_runs(letters[r.integers(0, len(letters), 256)]).tobytes())
    long[98:102] = b"kQzm"
    long = bytes(break_runs(np.frombuffer(bytes(long), dtype=np.uint8)[::-1])[::-1].tobytes())      # changes 97, not 98
    long = bytes(break_runs(np.frombuffer(long, dtype=np.uint8)).tobytes())                          # changes 102, not 101
    assert long[98:102] == b"kQzm" and len(long) == 256
    return {"n1": b"Q", "n2": long[99:101], "n16": b"N3eDLe#16-MiXed.", "n17": b"n3EdlE#17-mIxEd.!", "n256": long,
            "aXa": b"aXa", "abab": b"AbAbAbAb"}


def make_text(size, seed, cut=None):
    """`size` bytes of printable ASCII with newlines and no two equal neighbours, with the needles written over them at seeded
    places, in their own case and case-swapped, the self-overlapping ones as longer repetitions.  With `cut`, the 256-byte
    needle is planted at cut - 100 as well: byte `cut` is its byte 100 and the second byte of the 2-byte needle."""
    n = needles()
    text = bytearray(break_runs(np.frombuffer(datagen.text_like(size, seed), dtype=np.uint8)).tobytes())
    r = datagen.rng(seed ^ 0x7E57)
    plants = []

    def write(at, what):
        """what at `at`, and the bytes next to it made to differ from their neighbours: the last pass leaves it alone"""
        text[at:at + len(what)] = what
        plants.append((at, at + len(what)))
        for j in (at - 1, at + len(what)):
            if 0 <= j < size and text[j] != 10:
                around = (text[j - 1] if j > 0 else -1, text[j + 1] if j + 1 < size else -1)
                text[j] = next(c for c in b" ._,;" if c not in around)

    def plant(at, what):
        assert 0 <= at and at + len(what) <= size
        if all(at + len(what) + 8 <= p or q + 8 <= at for p, q in plants) and (
                cut is None or at + len(what) + 300 <= cut or cut + 300 <= at):
            write(at, what)

    if cut is not None:
        write(cut - 100, n["n256"])
    for name in ("n2", "n16", "n17", "n256"):
        for k in range(12):
            what = n[name] if k % 3 else n[name].swapcase()
            plant(int(r.integers(0, size - 300)), what)
    for k in range(8):
        plant(int(r.integers(0, size - 300)), b"aXaXaXa" if k % 2 else b"AxAxaXa")
        plant(int(r.integers(0, size - 300)), b"AbAbAbAbAbAb" if k % 2 else b"abABabABabAB")
    plant(0, n["n16"])                           # a needle at the text's first bytes and in front of its last one
    plant(size - 17, n["n16"])
    text = bytearray(break_runs(np.frombuffer(bytes(text), dtype=np.uint8)).tobytes())
    if text[-1] != 10:
        text[-1] = 10                            # the fillers behind a text start a line of their own
    if cut is not None:
        assert bytes(text[cut - 100:cut + 156]) == n["n256"]
    return bytes(text)


def stream_of(raw, level):
    """(stream, [(bit offset in the stream, decoded offset in the stream, decoded size)] per block, EOS bit offset):
    for data without runs, by the block size rule; checked against the magics found in the stream."""
    enc = bz2.compress(raw, level)
    per = 100_000 * level - 19
    bits = magic_offsets(enc, MAGIC_BLOCK)
    sizes = [min(per, len(raw) - k) for k in range(0, len(raw), per)]
    assert len(bits) == len(sizes), (len(bits), len(sizes))
    eos = [b for b in magic_offsets(enc[-16:], MAGIC_EOS)]
    assert len(eos) == 1
    blocks = [(b, k * per, s) for k, (b, s) in enumerate(zip(bits, sizes))]
    return enc, blocks, 8 * (len(enc) - 16) + eos[0]


@functools.lru_cache(maxsize=None)
def filler_stream(value, length):
    """The level-9 stream of `length` bytes `value`, one block."""
    assert 0 < length <= FULL_BLOCK
    enc = bz2.compress(bytes([value]) * length, 9)
    assert magic_offsets(enc, MAGIC_BLOCK) == [32], "a filler is one block"
    eos = magic_offsets(enc, MAGIC_EOS)
    assert len(eos) == 1
    return enc, eos[0]


class Stitched:
    """Streams appended one by one: the file, its parts, its block map and its block list, all by arithmetic."""

    def __init__(self):
        self.enc = bytearray()
        self.parts = []
        self.size = 0
        self.map = {}
        self.blocks = []         # (bit offset, decoded offset, decoded size, run value or None), file order
        self.eos = []            # bit offsets of the end-of-stream magics
        self.streams = []        # (first byte, bytes, decoded offset, decoded size)

    def add(self, enc, blocks, eos, part, values=None):
        front = 8 * len(self.enc)
        decoded = sum(size for _, _, size in blocks)
        for bit, offset, size in blocks:
            self.map[front + bit] = self.size + offset
            self.blocks.append((front + bit, self.size + offset, size, values))
        self.map[front + eos] = self.size + decoded
        self.eos.append(front + eos)
        self.streams.append((len(self.enc), len(enc), self.size, decoded))
        self.enc += enc
        self.parts.append(part)
        self.size += decoded

    def add_filler(self, value, length):
        enc, eos = filler_stream(value, length)
        self.add(enc, [(32, 0, length)], eos, (value, length), value)

    def add_text(self, raw, level=1):
        enc, blocks, eos = stream_of(raw, level)
        self.add(enc, blocks, eos, raw)


class BigFile:
    """What a builder returns: enc, raw (VirtualRaw, or None), map {bit offset: decoded offset}, the stitching itself and
    whatever the builder marks."""

    def __init__(self, stitched, virtual=True, **marks):
        stitched.map[8 * len(stitched.enc)] = stitched.size          # the end-of-file entry
        self.enc = bytes(stitched.enc)
        self.raw = VirtualRaw(stitched.parts) if virtual else None
        self.size = stitched.size
        self.map = dict(stitched.map)
        self.blocks = list(stitched.blocks)
        self.eos = list(stitched.eos)
        self.streams = list(stitched.streams)
        self.__dict__.update(marks)

    def __iter__(self):          # enc, raw, block_map = far_file()
        return iter((self.enc, self.raw, self.map))


def assert_no_alias(parts_of, cut):
    """No filler byte at x >= cut has its own value at x - cut: checked filler edge by filler edge."""
    parts = parts_of.parts
    for offset, value, _, length in parts:
        if value is None or offset + length <= cut:
            continue
        lo, hi = max(offset, cut) - cut, offset + length - cut
        for other, low_value, _, low_length in parts:
            if other < hi and lo < other + low_length:
                assert low_value != value, ("a filler aliases onto its own value", offset, other)


@functools.lru_cache(maxsize=None)
def far_file(cut=CUT, filler=FULL_BLOCK, text_size=1_000_000, tail_fillers=2):
    """A file that decodes past `cut` (2^32): T0, fillers, T1 around the cut, `tail_fillers` full fillers, T2 = T0's bytes.
    `filler` is the size of a full filler; the small-scale layouts of the CPU tests pass smaller ones."""
    per = 99_981
    target = 4 * per + 50_000 if text_size > 5 * per else text_size // 2        # of the cut inside T1
    t0 = make_text(text_size, 0xFA00)
    t1 = make_text(text_size, 0xFA01, cut=target)
    s = Stitched()
    s.add_text(t0)
    gap = cut - target - len(t0)
    assert gap > 0
    k = 0
    while gap > 0:
        s.add_filler(FILLER_VALUES[k % 7], min(filler, gap))
        gap -= min(filler, gap)
        k += 1
    t1_at = s.size
    s.add_text(t1)
    for _ in range(tail_fillers):
        s.add_filler(FILLER_VALUES[k % 7], filler)
        k += 1
    t2_at = s.size
    s.add_text(t0)
    far = BigFile(s, cut=cut, t0=t0, t1=t1, t1_at=t1_at, t2_at=t2_at, shift=t2_at, target=target)

    # the placement promises
    n = needles()
    raw = far.raw
    assert t1_at + target == cut and raw.size > cut + tail_fillers * filler
    inside = [(bit, at, size) for bit, at, size, value in far.blocks if at < cut < at + size]
    assert len(inside) == 1 and inside[0][1] >= t1_at and inside[0][1] + inside[0][2] <= t1_at + len(t1)
    assert all(at != cut and at + size != cut for _, at, size, _ in far.blocks)
    assert raw.slice(cut - 100, cut + 156) == n["n256"] and raw.slice(cut - 1, cut + 1) == n["n2"]
    # byte `cut` lies inside a line that begins and ends inside T1: a newline of T1 in front of the needle, one behind it
    newlines = raw.newline_offsets()
    assert 10 not in raw.slice(cut - 100, cut + 156)
    assert np.any((newlines >= t1_at) & (newlines < cut - 100)) and np.any((newlines >= cut + 156) & (newlines < t1_at + len(t1)))
    for value in raw.run_values:
        assert all(value not in needle and value != 10 for needle in n.values())
    assert_no_alias(raw, cut)
    for (_, _, _, a), (_, _, _, b) in zip(far.blocks, far.blocks[1:]):
        assert a is None or a != b, "neighbouring fillers differ"
    return far


# The regular expressions of the far-file tests, all inside the rule of VirtualRaw.regex_lines: a filler byte is matched
# by nothing, or by a `.` that stands alone or under `*`.  What each is for (checked by test_bigfiles.py at full scale):
FAR_PATTERNS = {
    "caret": rb"^dkb dqtlnhgz dqt",                    # anchored at the start of the line that straddles 2^32
    "dollar": rb"tmid apktzeld$",                      # ... and at its end
    "across": rb"pnSQ.*kQzm.*OG4 mb",                  # a literal below 2^32, `.*`, the bytes around it, `.*`, one above
    "t2-only": rb".N3eDLe#16-MiXed\. pek",             # T2's first line: a filler byte in front of T0's first bytes
    "ascii-tail": rb"MiXed\. qtlnhgz cnrntjvxu pmb",   # the line that holds the 94 fillers, through T1's first bytes
    "short": rb"n3EdlE#17-m[iI]xEd\.!",                # every matching line is short (grep_regex returns lines)
    "class": rb"^[a-z]+ [a-z ]+$",                # many lines, none with a filler
    "behind-fillers": rb"^.+N3eDLe#16-MiXed\. [a-z]",  # the first lines of T1 and T2, `.+` over every filler in front
    "nowhere": rb"never[0-9]there",
}
FAR_CARRIED = (rb"jdk \.N3e.*nipf lguogvy", b"_")     # under newline b"_": X in T0, the 94 fillers, Y in T1, one line


def long_field_batch(far):
    """(blocks, VirtualRaw) of a batch over far_file()'s blocks in another order: T0, then all fillers (the 94 and the two
    tail ones, back to back), then T2.  In far_file() itself no byte value is absent from T0 and from T1's first 450 kB,
    so no closed line or field there reaches 2^32 bytes (the fillers between T0 and T1 are 1.45 MB short of it); in this
    batch's output the bytes between T0's last byte and T2's first are more than 2^32 of one line.  No second file."""
    texts = [block for block in far.blocks if block[3] is None]
    t0 = [block for block in texts if block[1] < len(far.t0)]
    t2 = [block for block in texts if block[1] >= far.t2_at]
    fillers = [block for block in far.blocks if block[3] is not None]
    assert all(a[3] != b[3] for a, b in zip(fillers, fillers[1:])), "neighbouring fillers differ"
    blocks = t0 + fillers + t2
    raw = VirtualRaw([far.raw.slice(at, at + size) if value is None else (value, size) for _, at, size, value in blocks])
    assert raw.size == 2 * len(far.t0) + sum(size for _, _, size, _ in fillers) and raw.size - 2 * len(far.t0) > far.cut
    return blocks, raw


@functools.lru_cache(maxsize=None)
def deep_file(min_bits=(1 << 32) + (1 << 26), cut_bits=1 << 32, prefix_size=4_499_900, text_size=600_000):
    """A file whose compressed size passes `cut_bits` (2^32 bits): one level-9 stream of incompressible bytes, repeated
    until the prefix passes `min_bits`, then two text streams.  The prefix is not ASCII, so there is no VirtualRaw of the
    whole: `tail` is the VirtualRaw of the two texts, at decoded offset `prefix_decoded`, and deep_slice gives any bytes.
    One block's magic starts below cut_bits while the block's data lies above it (`straddling`)."""
    body = break_runs(np.frombuffer(datagen.random_bytes(prefix_size, 0xDEE9), dtype=np.uint8))
    body[body == 10] = 11                        # no newline in the prefix: the line index is the texts'
    body = break_runs(body).tobytes()
    enc, blocks, eos = stream_of(body, 9)
    copies = -(-min_bits // (8 * len(enc)))
    s = Stitched()
    for _ in range(copies):
        s.add(enc, blocks, eos, None)
    prefix_decoded = s.size
    ta, tb = make_text(text_size, 0xDE00), make_text(text_size, 0xDE01)
    s.add_text(ta)
    s.add_text(tb)
    deep = BigFile(s, virtual=False, body=body, body_stream=enc, copies=copies, prefix_decoded=prefix_decoded,
                   tail=VirtualRaw([ta + tb]), cut_bits=cut_bits)
    assert 8 * copies * len(enc) >= min_bits > cut_bits
    starts = [bit for bit, _, _, _ in deep.blocks]
    ends = starts[1:] + [8 * len(deep.enc)]
    # (112: the end-of-stream magic, the stream CRC and the next stream's header lie between a stream's last block and
    # the next magic)
    deep.straddling = [b for b, e in zip(starts, ends) if b + 48 <= cut_bits < e - 112 - 8]
    assert len(deep.straddling) == 1, "choose another copy count or prefix size: no block straddles the cut"
    return deep


def deep_slice(deep, start, end):
    """Decoded bytes [start, end) of deep_file(): the prefix by its period, the tail from its texts."""
    out = bytearray()
    period = len(deep.body)
    at = start
    while at < min(end, deep.prefix_decoded):
        k = at % period
        take = min(period - k, min(end, deep.prefix_decoded) - at)
        out += deep.body[k:k + take]
        at += take
    if end > deep.prefix_decoded:
        out += deep.tail.slice(max(start, deep.prefix_decoded) - deep.prefix_decoded, end - deep.prefix_decoded)
    return bytes(out)


# ------------------------------------------------------------------------------------------------ inputs of the encoder
# The same offsets the other way round: far_pieces() is far_file()'s decoded bytes as buffers to compress (one launch whose
# input passes 2^32 bytes), deep_input() is incompressible bytes whose stream passes 2^32 bits.  The launch planner of
# csrc/bz2_compress.hpp is restated below in plain Python; test_bigfiles.py compares its constants with the header.

LAUNCH_BLOCKS = 512
LAUNCH_BYTES = 12 << 30
BYTES_PER_POSITION = 45
GROUP_SIZE = 50


@functools.lru_cache(maxsize=None)
def _filler_array(value, length):
    a = np.full(length, value, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def far_pieces():
    """The decoded pieces of far_file(), in order, as buffers: the texts as bytes, every filler a read-only numpy uint8
    array of one value.  Fillers of equal value and length are the SAME object: nine arrays, about 0.4 GB, stand for 4.4 GB."""
    far = far_file()
    pieces = tuple(data if value is None else _filler_array(value, length) for _, value, data, length in far.raw.parts)
    assert sum(len(p) for p in pieces) == far.raw.size
    return pieces


def plan_blocks(part, level=9):
    """[(start, size, rle)] of the blocks libbz2 cuts `part` into -- bytes, or a (value, length) run: RLE1 pieces are runs
    of one value cut every 255 bytes, a piece of L < 4 bytes takes L RLE1 bytes, a longer one 5; a block ends with the first
    piece that brings its RLE1 bytes to 100 000 level - 19."""
    if isinstance(part, tuple):
        runs = np.array([part[1]], dtype=np.int64)
    else:
        a = np.frombuffer(bytes(part), dtype=np.uint8)
        edges = np.concatenate([[0], np.flatnonzero(a[1:] != a[:-1]) + 1, [len(a)]])
        runs = np.diff(edges).astype(np.int64)
    whole, rest = runs // 255, runs % 255
    counts = whole + (rest > 0)
    lengths = np.full(int(counts.sum()), 255, dtype=np.int64)
    last = np.cumsum(counts) - 1
    lengths[last[rest > 0]] = rest[rest > 0]
    ends = np.cumsum(lengths)                                # input bytes up to and with each piece
    rle = np.cumsum(np.where(lengths < 4, lengths, 5))       # RLE1 bytes likewise
    limit = 100_000 * level - 19
    blocks, first, start, base = [], 0, 0, 0
    while first < len(lengths):
        k = int(np.searchsorted(rle, base + limit, "left"))  # the first piece that fills the block
        k = min(k, len(lengths) - 1)
        blocks.append((start, int(ends[k]) - start, int(rle[k]) - base))
        first, start, base = k + 1, int(ends[k]), int(rle[k])
    return blocks


def block_bytes(size, rle):
    """blockBytes of bz2_compress.hpp: what a block costs of a launch's device budget."""
    return rle * BYTES_PER_POSITION + size + -(-(rle + 1) // GROUP_SIZE) * 8


def plan_launches(blocks, cap=0, budget=0):
    """[(first, count, input start, input bytes, device bytes)]: planLaunches of bz2_compress.hpp over [(size, rle)]."""
    cap, budget = cap or LAUNCH_BLOCKS, budget or LAUNCH_BYTES
    launches, at = [], 0
    for i, (size, rle) in enumerate(blocks):
        need = block_bytes(size, rle)
        if not launches or launches[-1][1] == cap or launches[-1][4] + need > budget:
            launches.append([i, 0, at, 0, 0])
        launches[-1][1] += 1
        launches[-1][3] += size
        launches[-1][4] += need
        at += size
    return [tuple(l) for l in launches]


DEEP_INPUT_SIZE = 550_000_000
DEEP_INPUT_SEED = 0xDEE9


@functools.lru_cache(maxsize=None)
def deep_input():
    """550 000 000 seeded incompressible bytes: at level 9 about 611 blocks and a stream of more than 2^32 + 2^26 bits
    (libbz2's ratio on such bytes is above 1: test_bigfiles.py)."""
    return datagen.random_bytes(DEEP_INPUT_SIZE, DEEP_INPUT_SEED)
