"""A plain Python model of field numbers (indexed_bzip2_amd/csrc/bz2_fieldnum.hpp): the number of field j of every line by
the definition -- bytes.split per line, then a regular expression and int() --, the summary of a stretch, the summary of a
stretch cut into chunks, the rule that stitches stretches that lie back to back, and the sums per key.  It builds on the
model of fields.py; Python's integers do the arithmetic and nothing here calls the code under test.  An unknown position
is None.  A text is (size saturated at 20, the first 19 bytes)."""
import re

import fields as F

NOT_A_NUMBER = -2**63
MISSING = -2**63 + 1
NUMBER = re.compile(rb"[+-]?[0-9]{1,18}")
FIELD_KEYS = ("count", "has_delimiter", "first_nl", "head_positions", "tail_start", "tail_delims", "tail_field_start",
              "tail_field_end", "tail_non_empty")


def number(content):
    """The definition: int(content) if the bytes are a number, else None."""
    content = bytes(content)
    return int(content) if NUMBER.fullmatch(content) else None


def word(field):
    """The int64 word of a field as fields_of gives it: None is a missing one."""
    if field is None:
        return MISSING
    value = number(field)
    return NOT_A_NUMBER if value is None else value


def direct(data, nl, dl, j):
    """(word, start, size) of field j in every line of data, by the definition."""
    return [(word(field), start, size) for field, (start, size) in zip(F.fields_of(data, nl, dl, j), F.direct(data, nl, dl, j))]


def words_of(data, nl, dl, j):
    return [word(field) for field in F.fields_of(data, nl, dl, j)]


def text(content):
    return min(len(content), 20), bytes(content[:19])


def join(first, second):
    """first followed by second: the size saturates."""
    return min(first[0] + second[0], 20), (first[1] + second[1])[:19]


def text_word(t):
    return NOT_A_NUMBER if t[0] > 19 else word(t[1])


def summarise_chunk(data, nl, dl, j):
    """The summary of one stretch for field j: fields.py's dict, and head_texts (the texts of the pieces between the head
    positions, at most j + 1 and one more than there are positions), tail_text (the tail's field as far as the stretch
    reaches, empty where its start is not reached) and numbers (the words of the lines it closes, the first as if the
    stretch were entered at a line start)."""
    data = bytes(data)
    s = F.summarise_chunk(data, nl, dl, j)
    head = data[:s["first_nl"]] if s["has_delimiter"] else data
    s["head_texts"] = [text(piece) for piece in head.split(bytes([dl]))[:min(len(s["head_positions"]) + 1, j + 1)]]
    if s["tail_field_start"] is None:
        s["tail_text"] = text(b"")
    else:
        s["tail_text"] = text(data[s["tail_field_start"]:len(data) if s["tail_field_end"] is None else s["tail_field_end"]])
    s["numbers"] = words_of(data[:s["tail_start"]], nl, dl, j) if s["has_delimiter"] else []
    return s


def empty(j):
    return summarise_chunk(b"", 10, 9, j)


def go_on(carry, j, positions, texts, offset):
    """The carry (field carry, text of the field so far) over the head of a stretch at `offset`."""
    (d, start, end), so_far = carry
    if end is None and d <= j and j - d < len(texts):
        so_far = join(so_far, texts[j - d])
    return F.go_on((d, start, end), j, positions, offset), so_far


def close(carry, at):
    """(word, start, size) of the open line closed at `at`."""
    field, so_far = carry
    start, size = F.close(field, at)
    if size < 0:
        return MISSING, start, size
    return (NOT_A_NUMBER if size > 19 else text_word(so_far)), start, size


def line_start(j, at):
    return F.line_start(j, at), text(b"")


def tail_carry(s):
    return (s["tail_delims"], s["tail_field_start"], s["tail_field_end"]), s["tail_text"]


def moved_carry(carry, offset):
    (d, start, end), so_far = carry
    return (d, F.moved(start, offset), F.moved(end, offset)), so_far


def append(left, right, j):
    """left followed by right, both summaries for field j."""
    offset = left["size"]
    fields = F.append({k: left[k] for k in FIELD_KEYS + ("size", "fields")}, {k: right[k] for k in FIELD_KEYS + ("size", "fields")}, j)
    out = dict(left, **fields)
    out["numbers"] = list(left["numbers"])
    out["head_texts"] = list(left["head_texts"])
    if not left["has_delimiter"] and len(left["head_texts"]) == len(left["head_positions"]) + 1:
        # the last text is open: no dl has closed it
        out["head_texts"][-1] = join(out["head_texts"][-1], right["head_texts"][0])
        out["head_texts"] = (out["head_texts"] + right["head_texts"][1:])[:j + 1]
    carry = go_on(tail_carry(left), j, right["head_positions"], right["head_texts"], offset)
    if right["has_delimiter"]:
        out["numbers"].append(close(carry, offset + right["first_nl"])[0])
        out["numbers"] += right["numbers"][1:]
        out["tail_text"] = right["tail_text"]
    else:
        out["tail_text"] = carry[1]
    return out


def summarise(data, nl, dl, j, chunk):
    """The summary of data, cut into chunks of `chunk` bytes and composed."""
    out = empty(j)
    for at in range(0, len(data), chunk):
        out = append(out, summarise_chunk(data[at:at + chunk], nl, dl, j), j)
    return out


def stitch(summaries, j, offset=0):
    """(word, start, size) of field j in all lines of stretches that lie back to back from a line start at `offset` to the
    end of the file, from their summaries alone."""
    out, carry, non_empty = [], line_start(j, offset), False
    for s in summaries:
        carry = go_on(carry, j, s["head_positions"], s["head_texts"], offset)
        if s["has_delimiter"]:
            listed = [(value, offset + start, size) for value, (start, size) in zip(s["numbers"], s["fields"])]
            out.append(close(carry, offset + s["first_nl"]) if non_empty else listed[0])
            out += listed[1:]
            carry = moved_carry(tail_carry(s), offset)
            non_empty = s["tail_non_empty"]
        else:
            non_empty = non_empty or s["tail_non_empty"]
        offset += s["size"]
    if non_empty:
        out.append(close(carry, offset))
    return out


def group_sums(data, nl, dl, key_field, value_field, first=0, count=None):
    """What sum_by_field gives for lines [first, first + count) of data, with the keys themselves: (groups, missing), the
    groups in the order of their first line, each a dict with key, line, count, numbers, sum, min, max (NOT_A_NUMBER
    without a number)."""
    keys = F.fields_of(data, nl, dl, key_field)
    values = words_of(data, nl, dl, value_field)
    last = len(keys) if count is None else min(len(keys), first + count)
    groups, missing = {}, 0
    for line in range(first, last):
        if keys[line] is None:
            missing += 1
            continue
        g = groups.setdefault(keys[line], {"key": keys[line], "line": line, "count": 0, "numbers": 0, "sum": 0,
                                           "min": NOT_A_NUMBER, "max": NOT_A_NUMBER})
        g["count"] += 1
        if values[line] not in (NOT_A_NUMBER, MISSING):
            g["min"] = values[line] if g["numbers"] == 0 else min(g["min"], values[line])
            g["max"] = values[line] if g["numbers"] == 0 else max(g["max"], values[line])
            g["numbers"] += 1
            g["sum"] += values[line]
    return list(groups.values()), missing
