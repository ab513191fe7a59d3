"""A plain Python model of the selection of lines by a regular expression on a field
(indexed_bzip2_amd/csrc/bz2_fieldregex.hpp): fields.fields_of -- bytes.split per line -- and regexgen.table_matches, the
compiled table run from state 0 over the field's bytes.  The field is to the pattern what a line's content is to grep_regex.
Nothing here calls the code under test but the compiler, whose table test_regex_plan.py pins to Python's `re`; `by_re` is
that reference itself, for fields without the byte 0x0A."""
import re

import fields as F
import regexgen as G

# the reader tests' list over columnshapes.corpus: (name, field, pattern, ignore_case).  Field 0 is the line's number, 1 a
# key (GET, GE, GETS, PUT, k07, bytes of 0x80 and above, one of 256 bytes, empty), 2 a number or something that is none, 3
# filler over b"abcdefgh ,.;" (one of 9 000 bytes, one of about 20 000), 4 b"end" and the number again
PATTERNS = (
    ("get", 1, rb"^GET$", False),
    ("ge-prefix", 1, rb"^GE", False),
    ("t-suffix", 1, rb"T$", False),
    ("empty", 1, rb"^$", False),
    ("anything", 3, rb"a*", False),
    ("e", 1, rb"E", False),
    ("high", 1, rb"[\x80-\xff]", False),
    ("number", 2, rb"^-?[0-9]+$", False),
    ("not-a-number", 2, rb"[^0-9+-]|^[+-]?$|.[+-]", False),
    ("k-keys", 1, rb"^k[0-9]+$", False),
    ("folded", 1, rb"^(get|put)s?$", True),
    ("filler", 3, rb"h;|,, |^[a-d]*$", False),
    ("filler-end", 3, rb"[ ,.;]{2}$", False),
    ("counter", 0, rb"^[0-9]*7$", False),
    ("end", 4, rb"^end[0-9]*3$|tail", False),
    ("either", 1, rb"^P|S$", False),
)
FIELDS = (0, 1, 2, 3, 4, 1023)


def field_matches(regex, field):
    """Does a field as fields_of gives it (None: the line has no such field) match the compiled table?"""
    return field is not None and G.table_matches(regex.transitions, regex.accepts_at_end, field)


def flags_of(regex, fields):
    """One bool per line, from the fields of its lines."""
    return [field_matches(regex, field) for field in fields]


def flags_of_data(regex, data, nl, dl, j):
    return flags_of(regex, F.fields_of(data, nl, dl, j))


def by_re(pattern, field, ignore_case=False):
    """Python's answer for a field that holds no byte 0x0A (its `$` also matches in front of a trailing one)."""
    assert field is None or b"\n" not in field
    return field is not None and re.search(pattern, field, G.reference_flags(ignore_case)) is not None


def dead_state(regex):
    """The state, not 1, that every byte leads back to and that does not accept at the end; None if there is none."""
    for d in range(regex.states):
        if d != G.MATCHED and not regex.accepts_at_end[d] and (regex.transitions[d] == d).all():
            return d
    return None
