"""A plain Python model of the selection of lines by a field (indexed_bzip2_amd/csrc/bz2_fieldmatch.hpp): bytes.split per
line (fields.py), `in` on a Python set for a predicate of values, and the number of the field with integer comparisons for
a range.  Nothing here calls the code under test: `number` is fieldnum.py's model of the definition by default, and the GPU
tests hand in indexed_bzip2_amd.parse_field_number, which test_fieldnum_plan.py pins to that model."""
import fields as F
import fieldnum as FN

NUMBER_MAX = 10**18 - 1                       # the largest number a field can be; the least is its negative


def clipped(between):
    """(lo, hi) of between=(lo, hi) as the definition clips them: None is an open side."""
    lo, hi = between
    lo = -NUMBER_MAX if lo is None else max(-NUMBER_MAX, min(NUMBER_MAX, lo))
    hi = NUMBER_MAX if hi is None else max(-NUMBER_MAX, min(NUMBER_MAX, hi))
    return lo, hi


def matches(field, values=None, between=None, number=FN.number):
    """Does a field as fields_of gives it (None: the line has no such field) satisfy the predicate?"""
    assert (values is None) != (between is None)
    if field is None:
        return False
    if values is not None:
        return bytes(field) in {bytes(value) for value in values}
    n = number(bytes(field))
    if n is None:
        return False
    lo, hi = clipped(between)
    return lo <= n <= hi


def flags_of(data, nl, dl, j, values=None, between=None, number=FN.number):
    """One bool per line of data."""
    wanted = None if values is None else {bytes(value) for value in values}
    if wanted is not None:
        return [field is not None and field in wanted for field in F.fields_of(data, nl, dl, j)]
    return [matches(field, None, between, number) for field in F.fields_of(data, nl, dl, j)]


def selected(flags, invert=False, first=0, count=None, limit=None):
    """The numbers, in the file, of the selected lines of [first, first + count) among the lines with these flags."""
    end = len(flags) if count is None else min(len(flags), first + count)
    out = [i for i in range(min(first, len(flags)), end) if flags[i] != invert]
    return out if limit is None else out[:limit]


def where(data, nl, dl, j, values=None, between=None, invert=False, first=0, count=None, limit=None, number=FN.number):
    return selected(flags_of(data, nl, dl, j, values, between, number), invert, first, count, limit)


def lines_with_delimiters(data, nl):
    """The lines of data whole, each with its delimiter; the unterminated tail as it is."""
    data = bytes(data)
    pieces = data.split(bytes([nl]))
    return [piece + bytes([nl]) for piece in pieces[:-1]] + ([pieces[-1]] if pieces[-1] else [])
