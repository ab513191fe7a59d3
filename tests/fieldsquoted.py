"""A plain Python model of quoted field access (indexed_bzip2_amd/csrc/bz2_fieldquote.hpp), restated here without the
C++: the definition -- every quote byte toggles, a delimiter inside quotes does not part the line, the newline always
closes it, the content of a field loses its enclosing pair --, the summary of a stretch with its head under both entry
hypotheses, the rule that stitches stretches, and the scanned element with its composition.  Lines, carries and "missing"
are those of fields.py.  Nothing here calls the code under test.  An unknown position is None."""
import fields as F


def parts_of_loop(content, dl, q, inq=0):
    """[(start, end)] of the raw fields of one line's content, entered in state `inq`: the definition as it is written."""
    parts, s = [], 0
    for i, b in enumerate(content):
        if b == q:
            inq ^= 1
        elif b == dl and not inq:
            parts.append((s, i))
            s = i + 1
    parts.append((s, len(content)))
    return parts


def parts_of(content, dl, q, inq=0):
    """parts_of_loop without a step per byte, for lines of megabytes: the quotes cut the content into pieces that lie
    outside and inside quotes in turn, and only the delimiters of the pieces outside part it."""
    parts, s, at = [], 0, 0
    for k, piece in enumerate(bytes(content).split(bytes([q]))):
        if (k + inq) % 2 == 0:
            found = piece.find(dl)
            while found >= 0:
                parts.append((s, at + found))
                s = at + found + 1
                found = piece.find(dl, found + 1)
        at += len(piece) + 1
    parts.append((s, len(content)))
    return parts


def raw_direct(data, nl, dl, q, j):
    """(start, size) of RAW field j in every line of data; a missing field is (end of content, -1)."""
    out, s = [], 0
    for content in F.lines_of(data, nl):
        parts = parts_of(content, dl, q)
        out.append((s + parts[j][0], parts[j][1] - parts[j][0]) if j < len(parts) else (s + len(content), -1))
        s += len(content) + 1
    return out


def content_of(data, span, q):
    """The content of the raw field `span` of data: without its first and last byte if both are the quote."""
    start, size = span
    if size >= 2 and data[start] == q and data[start + size - 1] == q:
        return (start + 1, size - 2)
    return span


def direct(data, nl, dl, q, j):
    """(start, size) of the CONTENT of field j in every line of data: what field_spans(quote=) returns."""
    return [content_of(data, span, q) for span in raw_direct(data, nl, dl, q, j)]


def fields_of(data, nl, dl, q, j):
    """The content of field j of every line as bytes, None where it is missing: what read_fields(quote=) returns."""
    return [bytes(data[start:start + size]) if size >= 0 else None for start, size in direct(data, nl, dl, q, j)]


def counted(content, dl, q, inq, limit):
    """The positions of the first `limit` delimiters of content that lie outside quotes, entered in state `inq`."""
    return [end for _, end in parts_of(content, dl, q, inq)[:-1]][:limit]


def summarise_chunk(data, nl, dl, q, j):
    """The summary of one stretch for field j, all positions relative to it: count, has_delimiter, first_nl,
    head_positions (a pair: entered outside and inside quotes), head_quote_parity, tail_start, tail_delims,
    tail_field_start, tail_field_end, tail_in_quote, tail_non_empty, size, and fields: the RAW (start, size) of field j in
    the lines it closes, the first as if the stretch were entered at a line start, outside quotes."""
    data = bytes(data)
    pieces = data.split(bytes([nl]))
    has = len(pieces) > 1
    tail_start = len(data) - len(pieces[-1]) if has else 0
    tail = F.go_on(F.line_start(j, tail_start), j, counted(pieces[-1], dl, q, 0, j + 1), tail_start)
    return {"size": len(data), "count": len(pieces) - 1, "has_delimiter": has, "first_nl": len(pieces[0]) if has else None,
            "head_positions": [counted(pieces[0], dl, q, h, j + 1) for h in (0, 1)],
            "head_quote_parity": pieces[0].count(bytes([q])) % 2 == 1,
            "tail_start": tail_start, "tail_delims": tail[0], "tail_field_start": tail[1], "tail_field_end": tail[2],
            "tail_in_quote": pieces[-1].count(bytes([q])) % 2 == 1, "tail_non_empty": len(data) > 0 and data[-1] != nl,
            "fields": raw_direct(data[:tail_start], nl, dl, q, j) if has else []}


def stitch(summaries, j, offset=0):
    """RAW (start, size) of field j in all lines of stretches that lie back to back from a line start at `offset` to the
    end of the file, from their summaries alone: fields.stitch with a quote state beside the carry -- the head list is the
    one of the state the carry is in, the head's parity moves the state on, and a tail brings its own."""
    fields, carry, inq, non_empty = [], F.line_start(j, offset), False, False
    for s in summaries:
        carry = F.go_on(carry, j, s["head_positions"][1 if inq else 0], offset)
        inq = inq != s["head_quote_parity"]
        if s["has_delimiter"]:
            fields.append(F.close(carry, offset + s["first_nl"]) if non_empty else (offset + s["fields"][0][0], s["fields"][0][1]))
            fields += [(offset + start, size) for start, size in s["fields"][1:]]
            carry = (s["tail_delims"], F.moved(s["tail_field_start"], offset), F.moved(s["tail_field_end"], offset))
            inq, non_empty = s["tail_in_quote"], s["tail_non_empty"]
        else:
            non_empty = non_empty or s["tail_non_empty"]
        offset += s["size"]
    if non_empty:
        fields.append(F.close(carry, offset))
    return fields


def element_of(data, nl, dl, q, cap):
    """The scanned element (reset, p, a0, a1) of a stretch, by the definition: reset = it holds a newline; over the bytes
    behind its last newline (all of them without one), p = the parity of the quotes and a0 / a1 = the delimiters that
    count when these bytes are entered outside / inside quotes, saturated at cap.  Behind a newline a line is outside."""
    data = bytes(data)
    pieces = data.split(bytes([nl]))
    reset, last = len(pieces) > 1, pieces[-1]
    a0 = min(len(counted(last, dl, q, 0, cap)), cap)
    a1 = a0 if reset else min(len(counted(last, dl, q, 1, cap)), cap)
    return (reset, last.count(bytes([q])) % 2 == 1, a0, a1)


def compose(first, second, cap):
    """`first` followed by `second`."""
    if second[0]:
        return second
    e0 = first[1]
    e1 = first[1] if first[0] else not first[1]
    return (first[0], first[1] != second[1], min(first[2] + second[3 if e0 else 2], cap), min(first[3] + second[3 if e1 else 2], cap))
