"""A plain Python model of field hashes (indexed_bzip2_amd/csrc/bz2_fieldhash.hpp): the key of field j of every line by
the definition -- bytes.split per line, then a Python restatement of the line hash --, the summary of a stretch, the
summary of a stretch cut into chunks, and the rule that stitches stretches that lie back to back.  It builds on the models
of fields.py and linehash.py; Python's integers do the arithmetic and nothing here calls the code under test.  An unknown
position or hash is None."""
import re

import fields as F
import linehash as LH

P = LH.P
MISSING = 2**61 - 1
FIELD_KEYS = ("count", "has_delimiter", "first_nl", "head_positions", "tail_start", "tail_delims", "tail_field_start",
              "tail_field_end", "tail_non_empty")
HASH_KEYS = ("head", "tail", "head_hashes", "tail_start_hash", "tail_end_hash")


def key_of(field, seed=0):
    """The key of a field as fields_of gives it: None is a missing one."""
    return MISSING if field is None else LH.line_hash(field, seed)


def direct(data, nl, dl, j, seed=0):
    """(key, start, size) of field j in every line of data, by the definition."""
    return [(key_of(field, seed), start, size)
            for field, (start, size) in zip(F.fields_of(data, nl, dl, j), F.direct(data, nl, dl, j))]


def keys_of(data, nl, dl, j, seed=0):
    return [key_of(field, seed) for field in F.fields_of(data, nl, dl, j)]


LONG_RUN = re.compile(rb"(.)\1{63,}", re.DOTALL)


def run_part(byte, n, x):
    """(h, xl) of n times the same byte: ( b + 1 ) ( x^n - 1 ) / ( x - 1 )."""
    xl = pow(x, n, P)
    return (byte + 1) * (xl - 1) * pow(x - 1, P - 2, P) % P, xl


def part(content, x):
    """linehash.part, with the long runs of one byte in closed form: the same value, sooner."""
    content = bytes(content)
    out, at = (0, 1), 0
    for run in LONG_RUN.finditer(content):
        out = LH.followed_by(out, LH.part(content[at:run.start()], x))
        out = LH.followed_by(out, run_part(content[run.start()], run.end() - run.start(), x))
        at = run.end()
    return LH.followed_by(out, LH.part(content[at:], x))


class Text:
    """A byte string under base x whose pieces are hashed often: part(a, b) is part(data[a:b], x).  With prefixes=True the
    hashes of all prefixes are computed once (linehash.Prefix: right for many spans of a text of a megabyte); otherwise
    every piece is hashed when asked for, long runs in closed form (right for a few spans of a text of runs)."""

    def __init__(self, data, x, prefixes=True):
        self.data, self.x = bytes(data), x
        self.prefix = LH.Prefix(self.data, x) if prefixes else None

    def part(self, a, b):
        return self.prefix.part(a, b) if self.prefix is not None else part(self.data[a:b], self.x)

    def key(self, start, size):
        return MISSING if size < 0 else self.part(start, start + size)[0]

    def summary(self, offset, size, nl, dl, j):
        """The summary of data[offset:offset + size] for field j, positions relative to the stretch: fields.py's dict, and
        head, tail (each (h, xl)), head_hashes (the hash of the stretch's bytes in front of every head position),
        tail_start_hash and tail_end_hash (the hash of the tail's bytes in front of its field's start and end, None
        where not reached) and keys (of the lines it closes, the first as if the stretch were entered at a line
        start)."""
        s = F.summarise_chunk(self.data[offset:offset + size], nl, dl, j)
        end_of_head = s["first_nl"] if s["has_delimiter"] else size
        s["head"] = self.part(offset, offset + end_of_head)
        s["tail"] = self.part(offset + s["tail_start"], offset + size) if s["has_delimiter"] else (0, 1)
        s["head_hashes"] = [self.part(offset, offset + p)[0] for p in s["head_positions"]]
        for name, position in (("tail_start_hash", s["tail_field_start"]), ("tail_end_hash", s["tail_field_end"])):
            s[name] = None if position is None else self.part(offset + s["tail_start"], offset + position)[0]
        s["keys"] = [self.key(offset + start, n) for start, n in s["fields"]]
        return s


def summarise_chunk(data, nl, dl, j, x):
    return Text(data, x).summary(0, len(data), nl, dl, j)


def empty(j):
    return summarise_chunk(b"", 10, 9, j, 256)


def go_on(carry, j, x, dl, positions, hashes, offset):
    """The carry (field carry, line (h, xl), P at the field's start, P at its end) over the head of a stretch at `offset`;
    the line stays the line in front of the stretch."""
    (d, start, end), line, p_start, p_end = carry
    n = len(positions)

    def prefix_at(k):
        return (line[0] * pow(x, positions[k], P) + hashes[k]) % P
    if start is None and d + n >= j:
        p_start = (prefix_at(j - d - 1) * x + dl + 1) % P
    if end is None and d + n >= j + 1:
        p_end = prefix_at(j - d)
    return F.go_on((d, start, end), j, positions, offset), line, p_start, p_end


def close(carry, x, at, line_hash_at):
    """(key, start, size) of the open line closed at `at`, where its whole content hashes to line_hash_at."""
    field, _, p_start, p_end = carry
    start, size = F.close(field, at)
    if size < 0:
        return MISSING, start, size
    if field[2] is None:
        p_end = line_hash_at
    return (p_end - p_start * pow(x, size, P)) % P, start, size


def line_start(j, at):
    return F.line_start(j, at), (0, 1), 0 if j == 0 else None, None


def tail_carry(s):
    return ((s["tail_delims"], s["tail_field_start"], s["tail_field_end"]), s["tail"] if s["has_delimiter"] else s["head"],
            s["tail_start_hash"], s["tail_end_hash"])


def moved_carry(carry, offset):
    (d, start, end), line, p_start, p_end = carry
    return (d, F.moved(start, offset), F.moved(end, offset)), line, p_start, p_end


def append(left, right, j, x, dl):
    """left followed by right, both summaries for field j under x."""
    offset = left["size"]
    fields = F.append({k: left[k] for k in FIELD_KEYS + ("size", "fields")}, {k: right[k] for k in FIELD_KEYS + ("size", "fields")}, j)
    out = dict(left, **fields)
    out["keys"] = list(left["keys"])
    carry = go_on(tail_carry(left), j, x, dl, right["head_positions"], right["head_hashes"], offset)
    line = LH.followed_by(carry[1], right["head"])
    if not left["has_delimiter"]:
        room = j + 1 - len(left["head_positions"])
        out["head_hashes"] = left["head_hashes"] + [(left["head"][0] * pow(x, p, P) + h) % P
                                                    for p, h in zip(right["head_positions"][:room], right["head_hashes"])]
    if right["has_delimiter"]:
        out["keys"].append(close(carry, x, offset + right["first_nl"], line[0])[0])
        out["keys"] += right["keys"][1:]
        if not left["has_delimiter"]:
            out["head"] = line
        out.update(tail=right["tail"], tail_start_hash=right["tail_start_hash"], tail_end_hash=right["tail_end_hash"])
    else:
        out["tail" if left["has_delimiter"] else "head"] = line
        out.update(tail_start_hash=carry[2], tail_end_hash=carry[3])
    return out


def summarise(data, nl, dl, j, x, chunk):
    """The summary of data, cut into chunks of `chunk` bytes and composed."""
    out = empty(j)
    for at in range(0, len(data), chunk):
        out = append(out, summarise_chunk(data[at:at + chunk], nl, dl, j, x), j, x, dl)
    return out


def stitch(summaries, j, x, dl, offset=0):
    """(key, start, size) of field j in all lines of stretches that lie back to back from a line start at `offset` to the
    end of the file, from their summaries alone."""
    out, carry, non_empty = [], line_start(j, offset), False
    for s in summaries:
        carry = go_on(carry, j, x, dl, s["head_positions"], s["head_hashes"], offset)
        line = LH.followed_by(carry[1], s["head"])
        if s["has_delimiter"]:
            listed = [(key, offset + start, size) for key, (start, size) in zip(s["keys"], s["fields"])]
            out.append(close(carry, x, offset + s["first_nl"], line[0]) if non_empty else listed[0])
            out += listed[1:]
            carry = moved_carry(tail_carry(s), offset)
            non_empty = s["tail_non_empty"]
        else:
            carry = (carry[0], line, carry[2], carry[3])
            non_empty = non_empty or s["tail_non_empty"]
        offset += s["size"]
    if non_empty:
        out.append(close(carry, x, offset, carry[1][0]))
    return out
