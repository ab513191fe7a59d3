"""A plain Python model of field columns (indexed_bzip2_amd/csrc/bz2_fieldcols.hpp): field j of every line as packed bytes
with offsets and sizes, by the definition -- bytes.split per line, fields.py --; what gather_fields makes of a list of spans;
and the column's own assembly from per-stretch packs, the stitcher's patches and fix-ups fetched from the text.  Nothing
here calls the code under test."""
import fields as F


def column(data, nl, dl, j, first=0, count=None):
    """(bytes, offsets, sizes) of field j over the lines [first, first + count) of data: a missing field has size -1 and
    owns no bytes."""
    fields = F.fields_of(data, nl, dl, j)[first:None if count is None else first + count]
    offsets = [0]
    for field in fields:
        offsets.append(offsets[-1] + len(field or b""))
    return b"".join(field or b"" for field in fields), offsets, [-1 if field is None else len(field) for field in fields]


def gathered(output, starts, sizes, base=0):
    """(total, offsets, bytes) that gather_fields gives for the spans (starts[i] - base, sizes[i]) of output; every span
    with bytes must lie inside it."""
    offsets, parts = [0], []
    for start, size in zip(starts, sizes):
        size = max(int(size), 0)
        if size:
            at = int(start) - base
            assert 0 <= at and at + size <= len(output), (start, size)
            parts.append(output[at:at + size])
        offsets.append(offsets[-1] + size)
    return offsets[-1], offsets, b"".join(parts)


def stretch_pack(stretch, nl, dl, j, skip, take):
    """What a stretch packs for the lines [skip, skip + take) of those it closes: (bytes, size of the first of them), each
    field as the stretch alone sees it -- the first closed line as if the stretch were entered at a line start."""
    fields = F.summarise_chunk(stretch, nl, dl, j)["fields"][skip:skip + take]
    parts = [stretch[start:start + max(size, 0)] for start, size in fields]
    return b"".join(parts), len(parts[0]) if parts else 0


def patches_of(summaries, j):
    """[(closed line, start, size)] the stitcher patches, from the stretches' summaries alone: the first closed line of a
    stretch that an open line enters; and (closed lines, tail or None), the unterminated tail as (start, size)."""
    patches, closed, offset = [], 0, 0
    carry, non_empty = F.line_start(j, 0), False
    for s in summaries:
        carry = F.go_on(carry, j, s["head_positions"], offset)
        if s["has_delimiter"]:
            if non_empty:
                patches.append((closed,) + F.close(carry, offset + s["first_nl"]))
            closed += s["count"]
            carry = (s["tail_delims"], F.moved(s["tail_field_start"], offset), F.moved(s["tail_field_end"], offset))
            non_empty = s["tail_non_empty"]
        else:
            non_empty = non_empty or s["tail_non_empty"]
        offset += s["size"]
    return patches, closed, F.close(carry, offset) if non_empty else None


def assemble(data, cuts, nl, dl, j, first=0, count=None):
    """The column of the lines [first, first + count) of data, assembled as the reader assembles it: data is cut at `cuts`
    into stretches, every stretch packs the wanted lines it closes, and the lines the stitcher patches -- the tail among
    them -- are fetched from data.  Returns (bytes, fix-ups as [(offset in data, size, place in the column)])."""
    data = bytes(data)
    bounds = [0] + sorted(cuts) + [len(data)]
    stretches = [data[a:b] for a, b in zip(bounds, bounds[1:])]
    summaries = [F.summarise_chunk(s, nl, dl, j) for s in stretches]
    patches, closed, tail = patches_of(summaries, j)
    end = closed + (tail is not None) if count is None else min(first + count, closed + (tail is not None))
    patched = {line: (start, size) for line, start, size in patches}
    out, fixups, before = [], [], 0

    def fix(start, size):
        if size >= 0:
            fixups.append((start, size, sum(map(len, out))))
            out.append(data[start:start + size])
    for stretch, summary in zip(stretches, summaries):
        lo, hi = max(before, first), min(before + summary["count"], end, closed)
        if hi > lo:
            pack, first_size = stretch_pack(stretch, nl, dl, j, lo - before, hi - lo)
            if lo == before and lo in patched:
                fix(*patched[lo])
                pack = pack[first_size:]
            out.append(pack)
        before += summary["count"]
    if tail is not None and first <= closed < end:
        fix(*tail)
    return b"".join(out), fixups
