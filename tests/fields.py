"""A plain Python model of field access (indexed_bzip2_amd/csrc/bz2_fields.hpp): where field j of every line lies by the
definition -- bytes.split per line --, the summary of a stretch for field j, the summary of a stretch cut into chunks, and
the rule that stitches stretches that lie back to back.  bytes.split and bytes.find do the work; nothing here calls the
code under test.  An unknown position is None."""


def lines_of(data, nl):
    """The contents of the lines of data as line_hashes numbers them: a non-empty unterminated tail is one more line."""
    pieces = bytes(data).split(bytes([nl]))
    return pieces[:-1] + ([pieces[-1]] if pieces[-1] else [])


def direct(data, nl, dl, j):
    """(start, size) of field j in every line of data, by the definition; a missing field is (end of content, -1)."""
    out, s = [], 0
    for content in lines_of(data, nl):
        parts = content.split(bytes([dl]))
        if j < len(parts):
            out.append((s + sum(len(p) + 1 for p in parts[:j]), len(parts[j])))
        else:
            out.append((s + len(content), -1))
        s += len(content) + 1
    return out


def fields_of(data, nl, dl, j):
    """Field j of every line as bytes, None where it is missing: what read_fields returns."""
    parts = [content.split(bytes([dl])) for content in lines_of(data, nl)]
    return [p[j] if j < len(p) else None for p in parts]


def delimiters(content, dl, limit):
    """The positions of the first `limit` dl bytes of content."""
    out, at = [], content.find(bytes([dl]))
    while at >= 0 and len(out) < limit:
        out.append(at)
        at = content.find(bytes([dl]), at + 1)
    return out


def line_start(j, at):
    """The carry (delimiters passed, field start, field end) of a line that starts at `at`."""
    return (0, at if j == 0 else None, None)


def go_on(carry, j, positions, offset):
    """The carry behind more dl bytes at positions (at most j + 1 of them) + offset."""
    d, start, end = carry
    n = len(positions)
    if start is None and d + n >= j:
        start = offset + positions[j - d - 1] + 1
    if end is None and d + n >= j + 1:
        end = offset + positions[j - d]
    return (min(d + n, j + 1), start, end)


def close(carry, at):
    """The open line closed at `at`, by a delimiter or by the end of the file."""
    _, start, end = carry
    if start is None:
        return (at, -1)
    return (start, (at if end is None else end) - start)


def summarise_chunk(data, nl, dl, j):
    """The summary of one stretch for field j, all positions relative to it: a dict with count, has_delimiter, first_nl,
    head_positions, tail_start, tail_delims, tail_field_start, tail_field_end, tail_non_empty, size, and fields: (start,
    size) of field j in the lines it closes, the first as if the stretch were entered at a line start."""
    data = bytes(data)
    pieces = data.split(bytes([nl]))
    has = len(pieces) > 1
    tail_start = len(data) - len(pieces[-1]) if has else 0
    tail = go_on(line_start(j, tail_start), j, delimiters(pieces[-1], dl, j + 1), tail_start)
    return {"size": len(data), "count": len(pieces) - 1, "has_delimiter": has, "first_nl": len(pieces[0]) if has else None,
            "head_positions": delimiters(pieces[0], dl, j + 1), "tail_start": tail_start, "tail_delims": tail[0],
            "tail_field_start": tail[1], "tail_field_end": tail[2], "tail_non_empty": len(data) > 0 and data[-1] != nl,
            "fields": direct(data[:tail_start], nl, dl, j) if has else []}


def empty(j):
    return summarise_chunk(b"", 10, 9, j)


def moved(position, offset):
    return None if position is None else position + offset


def append(left, right, j):
    """left followed by right, both summaries for field j."""
    offset = left["size"]
    carry = go_on((left["tail_delims"], left["tail_field_start"], left["tail_field_end"]), j, right["head_positions"], offset)
    out = dict(left, fields=list(left["fields"]), size=offset + right["size"])
    if not left["has_delimiter"]:
        out["head_positions"] = (left["head_positions"] + [offset + p for p in right["head_positions"]])[:j + 1]
    if right["has_delimiter"]:
        out["fields"].append(close(carry, offset + right["first_nl"]))
        out["fields"] += [(offset + start, size) for start, size in right["fields"][1:]]
        if not left["has_delimiter"]:
            out["first_nl"] = offset + right["first_nl"]
        out.update(has_delimiter=True, tail_start=offset + right["tail_start"], tail_delims=right["tail_delims"],
                   tail_field_start=moved(right["tail_field_start"], offset), tail_field_end=moved(right["tail_field_end"], offset),
                   tail_non_empty=right["tail_non_empty"])
    else:
        out.update(tail_delims=carry[0], tail_field_start=carry[1], tail_field_end=carry[2],
                   tail_non_empty=left["tail_non_empty"] or right["tail_non_empty"])
    out["count"] = len(out["fields"])
    return out


def summarise(data, nl, dl, j, chunk):
    """The summary of data, cut into chunks of `chunk` bytes and composed."""
    out = empty(j)
    for at in range(0, len(data), chunk):
        out = append(out, summarise_chunk(data[at:at + chunk], nl, dl, j), j)
    return out


def stitch(summaries, j, offset=0):
    """(start, size) of field j in all lines of stretches that lie back to back from a line start at `offset` to the end
    of the file, from their summaries alone: a carry that starts as a line start's; the head of a stretch continues it;
    with a delimiter the first closed line is the carry closed at first_nl and the carry becomes the tail; at the end a
    carry over at least one byte is the unterminated tail."""
    fields, carry, non_empty = [], line_start(j, offset), False
    for s in summaries:
        carry = go_on(carry, j, s["head_positions"], offset)
        if s["has_delimiter"]:
            fields.append(close(carry, offset + s["first_nl"]) if non_empty else (offset + s["fields"][0][0], s["fields"][0][1]))
            fields += [(offset + start, size) for start, size in s["fields"][1:]]
            carry = (s["tail_delims"], moved(s["tail_field_start"], offset), moved(s["tail_field_end"], offset))
            non_empty = s["tail_non_empty"]
        else:
            non_empty = non_empty or s["tail_non_empty"]
        offset += s["size"]
    if non_empty:
        fields.append(close(carry, offset))
    return fields
