"""Lines selected by a regular expression on a field, on the GPU: the kernel under Decoder.match_fields_regex (k_field_regex
behind the field-span passes) on one decoded text of a few KB, the reader's where_field / count_where_field / select_lines
with regex= and their tensor forms on the corpus of columnshapes.py, whose planted lines cross the launch seams, two
equivalences that need no model, the hold rules, the count of decoded blocks, and the tool's --where-field --matches.

The reference is the plain Python model of fieldregex.py -- bytes.split per line and the compiled table run over the field's
bytes, which test_fieldregex_plan.py pins to Python's `re` --, never the code under test.  Every comparison is exact."""
import bisect
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import columnshapes as C
import datagen
import fieldregex as FR
import fields as F
import regexgen as G
from columnshapes import NL, TAB

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
ONES = 2**64 - 1                                               # what Decoder.match_fields_regex fills `flags` with
INVALID_ARGUMENT = 103
THREADS, BLOCKS = 256, 512                                     # of k_field_regex: a grid covers THREADS * BLOCKS lines
LITERAL_62 = b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"      # 62 bytes and the two fixed states: 64 states
LAST = b"the-last-GET"
KERNEL_PATTERNS = ((rb"^GET$", False), (rb"^GE", False), (rb"T$", False), (rb"^$", False), (rb"a*", False), (rb"E", False),
                   (rb"[\x80-\xff]", False), (rb"^-?[0-9]+$", False), (LITERAL_62, False), (rb"^get$", True), (rb"[^a]", True),
                   (rb"^a|b$", False), (rb"qb", False), (rb"^q*$", False))


# ------------------------------------------------------------------------------------------------ the kernel

def device_text():
    """About 14 kB of tab-separated lines whose field 1 has the sizes 0, 1, 3, 4, 5, 255, 256, 257 and 5 000 among others,
    at every alignment of its first byte, lines without field 1, and an unterminated tail whose field ends on the last
    byte."""
    rng = random.Random(0xF1E1D)
    common = [b"", b"x", b"b", b"GET", b"GE", b"GETS", b"xGET", b"get", b"Get", b"xb", b"ab", b"ax", b"xbx", b"abcd", b"PUT-5",
              b"\x80\xff", b"\xfe", b"404", b"-7", b"-", b"12x", b"E", b"a\x00b", LITERAL_62, b"_" + LITERAL_62 + b"_", LITERAL_62[:-1]]
    long_ones = [b"p" * 255, b"q" * 256, b"q" * 256 + b"b", b"q" * 255 + b"r", b"q" * 256 + b"b" + b"z" * 4743, b"x" * 254 + b"b"]
    assert len(long_ones[4]) == 5000 and len(long_ones[2]) == 257
    out = bytearray()
    todo = list(long_ones)
    for k in range(330):
        pad = bytes(rng.choice(b"abc") for _ in range(k % 19))
        if k % 11 == 10:
            out += pad + b"\n"                                     # no field 1
        elif k % 50 == 7 and todo:
            out += pad + b"\t" + todo.pop() + b"\t" + pad[:3] + b"\n"
        else:
            out += pad + b"\t" + common[(k * 7 + k // len(common)) % len(common)] + b"\t" + pad[:3] + b"\n"
    assert not todo
    for a in range(8):
        out += b"z" * a + b"\tGET\t\n"                            # the field's first byte at every alignment
    out += b"tail\t" + LAST
    return bytes(out)


@pytest.fixture(scope="module")
def device(native):
    text = device_text()
    enc = datagen.compress(text, 9)
    dec = native.Decoder(device=0)
    dec.set_input(enc)
    _, total = dec.decode_batch(native.find_magic(enc))
    assert total == len(text) and dec.copy_output(0, total) == text
    # computed once, shared, left unchanged
    fields = F.fields_of(text, NL, TAB, 1)[:-1]                 # of the closed lines
    _, starts, sizes = dec.field_spans([(0, total)], 1)
    assert len(starts) == len(fields) > THREADS + 1 and [int(s) for s in sizes] == [-1 if f is None else len(f) for f in fields]
    assert all(text[int(a):int(a) + int(s)] == f for a, s, f in zip(starts, sizes, fields) if f is not None)
    assert {int(a) % 4 for a, f in zip(starts, fields) if f == b"GET"} == set(range(4))         # every alignment mod 4
    assert {len(f) for f in fields if f is not None} >= {0, 1, 3, 4, 5, 255, 256, 257, 5000}
    regexes = {(p, fold): native.compile_regex(p, fold) for p, fold in KERNEL_PATTERNS}
    assert regexes[(LITERAL_62, False)].states == 64
    yield {"dec": dec, "text": text, "fields": fields, "starts": starts, "sizes": sizes, "regexes": regexes}
    dec.close()


def check(device, key, n=None, base=0, room_behind=8):
    """Decoder.match_fields_regex over the first n lines against the model, exactly; the words behind n stay as they were."""
    regex = device["regexes"][key]
    starts, sizes = device["starts"], device["sizes"]
    n = len(starts) if n is None else n
    want = [int(FR.field_matches(regex, f)) for f in device["fields"][:n]]
    got = device["dec"].match_fields_regex(regex, starts[:n] + np.uint64(base), sizes[:n], base=base, room=n + room_behind)
    assert got.dtype == np.uint64 and len(got) == n + room_behind
    assert got[:n].tolist() == want, (key, next(i for i, (a, b) in enumerate(zip(got[:n].tolist(), want)) if a != b))
    assert (got[n:] == ONES).all(), "written behind n"
    return sum(want)


def test_line_counts_and_the_canary(device):
    for n in (0, 1, THREADS - 1, THREADS, THREADS + 1, None):
        check(device, (rb"^GE", False), n)
    assert check(device, (rb"^GE", False)) > 20


def test_every_pattern_against_the_model(device):
    """Anchors, the empty pattern, bytes of 0x80 and above, 64 states, ignore_case, fields of 0 to 5 000 bytes."""
    fields = device["fields"]
    for key in KERNEL_PATTERNS:
        hits = check(device, key)
        assert 0 < hits < len(fields), key
        # the model is `re` where no field holds the newline (none does here)
        assert hits == sum(FR.by_re(key[0], f, key[1]) for f in fields), key
    assert check(device, (rb"^$", False)) == fields.count(b"")                           # present and empty, never missing
    assert check(device, (rb"a*", False)) == sum(f is not None for f in fields)          # every field that is present
    assert check(device, (rb"qb", False)) == 2                                           # behind 256 bytes; the 5 000-byte field too
    assert check(device, (rb"^q*$", False)) == 1 + fields.count(b"")                     # walks all 256 bytes, dies on none


def test_a_lane_does_not_stop_early_wrongly(native, device):
    """`^a` alone is dead behind an x; `^a|b$` is not: xb matches, xbx does not."""
    fields = device["fields"]
    regex = device["regexes"][(rb"^a|b$", False)]
    assert FR.dead_state(regex) is None and FR.dead_state(native.compile_regex(rb"^a")) is not None
    flags = device["dec"].match_fields_regex(regex, device["starts"], device["sizes"])
    for field, want in ((b"xb", 1), (b"xbx", 0), (b"ax", 1), (b"b", 1), (b"x" * 254 + b"b", 1), (b"GET", 0)):
        assert field in fields and {int(flags[i]) for i, f in enumerate(fields) if f == field} == {want}, field
    # a dead state there is: the answers stay the model's (check), and a long field costs it nothing to refuse
    assert FR.dead_state(device["regexes"][(rb"^GE", False)]) is not None
    check(device, (rb"^GE", False))


def test_the_grid_strides(native, device):
    """One line more than a grid covers, of one-byte fields: every byte of the text in turn."""
    text = np.frombuffer(device["text"], dtype=np.uint8)
    n = THREADS * BLOCKS + 1
    starts = (np.arange(n, dtype=np.uint64) * np.uint64(7)) % np.uint64(len(text))
    regex = device["regexes"][(rb"[^a]", True)]
    behind = regex.transitions[0][text[starts.astype(np.int64)]]
    want = ((behind == G.MATCHED) | (regex.accepts_at_end[behind] != 0)).astype(np.uint64)
    got = device["dec"].match_fields_regex(regex, starts, np.ones(n, dtype=np.int64), room=n + 8)
    assert np.array_equal(got[:n], want) and (got[n:] == ONES).all()
    assert 1000 < want.sum() < n - 1000


def test_base_beyond_32_bits(device):
    for base in (2**32 + 5, 2**64 - 3):
        check(device, (rb"^GET$", False), base=base)
        check(device, (rb"qb", False), base=base)


def test_the_last_byte_and_spans_outside(device):
    end = len(device["text"])
    assert device["text"].endswith(b"\t" + LAST)
    n = len(LAST)
    ends_in_get = device["regexes"][(rb"T$", False)]
    # a field that ends on the output's last byte, at each alignment of its first byte; one byte further it ends outside
    starts = np.array([end - n, end - n + 1, end - n + 2, end - n + 3, end - 1, end - n + 1, end - 3, end, end + 1, 2**63, 0],
                      dtype=np.uint64)
    sizes = np.array([n, n - 1, n - 2, n - 3, 1, n, 4, 1, 1, 5, -1], dtype=np.int64)
    assert device["dec"].match_fields_regex(ends_in_get, starts, sizes).tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    # an empty field at the very end is inside, one behind it is not; a missing one never matches
    anything = device["regexes"][(rb"a*", False)]
    assert device["dec"].match_fields_regex(anything, [end, end + 1, 0, end, 2**64 - 1], [0, 0, 0, -1, 2]).tolist() == [1, 0, 1, 0, 0]
    empty = device["regexes"][(rb"^$", False)]
    assert device["dec"].match_fields_regex(empty, [end, 0, 0], [0, 0, 1]).tolist() == [1, 1, 0]


def test_a_pattern_to_compile_and_the_refusals(native, device):
    starts, sizes = device["starts"][:40], device["sizes"][:40]
    want = [int(f is not None and re.search(rb"^GE", f) is not None) for f in device["fields"][:40]]
    assert device["dec"].match_fields_regex(rb"^GE", starts, sizes).tolist() == want
    with pytest.raises(ValueError):
        device["dec"].match_fields_regex(rb"(a)\1", starts, sizes)
    with pytest.raises(ValueError):
        device["dec"].match_fields_regex(rb"a", starts[:3], sizes)


# ------------------------------------------------------------------------------------------------ the reader

@pytest.fixture(scope="module")
def world(native, tmp_path_factory):
    """One entry per corpus variant: columnshapes.expected (shared, never changed), the file, and the flags of
    fieldregex.PATTERNS by the model, computed once."""
    folder = tmp_path_factory.mktemp("fieldregex")
    out = {}
    for variant in C.VARIANTS:
        e = dict(C.expected(variant))
        path = folder / (variant + ".bz2")
        path.write_bytes(e["enc"])
        e.update(path=str(path), n=len(e["lines"]), variant=variant, regexes={}, flags={})
        for name, j, pattern, fold in FR.PATTERNS:
            e["regexes"][name] = native.compile_regex(pattern, fold)
            e["flags"][name] = FR.flags_of(e["regexes"][name], e["fields"][j])
        e["missing"] = [False] * e["n"]                             # field 1023: no line has it
        # the lines that cross a planted launch boundary, and the blocks as the reader sees them
        newlines = e["newlines"]
        e["seam_lines"] = sorted({int(np.searchsorted(newlines, b, "left")) for b in C.planted()[0] if e["raw"][b - 1:b] != b"\n"})
        out[variant] = e
    assert out["tail"]["n"] == out["closed"]["n"] and not out["tail"]["raw"].endswith(b"\n")
    return out


def how_of(name):
    _, j, pattern, fold = next(p for p in FR.PATTERNS if p[0] == name)
    return j, dict(regex=pattern, ignore_case=fold)


def selected(e, name, invert=False, first=0, count=None, limit=None):
    flags = e["flags"][name]
    end = len(flags) if count is None else min(len(flags), first + count)
    out = [i for i in range(min(first, len(flags)), end) if flags[i] != invert]
    return out if limit is None else out[:limit]


def agree(f, e, name, forms="wcs", **how):
    """where_field, count_where_field and select_lines (each where its letter is in `forms`) against the model."""
    want = selected(e, name, **how)
    j, regex = how_of(name)
    if "w" in forms:
        got = f.where_field(j, **regex, **how)
        assert got.dtype == np.uint64 and got.tolist() == want, (name, how, len(got), len(want))
    if "c" in forms:
        assert f.count_where_field(j, **regex, **how) == len(want), (name, how)
    if "s" in forms:
        numbers, lines = f.select_lines(j, **regex, **how)
        assert numbers.tolist() == want and lines == [e["whole_lines"][i] for i in want], (name, how)
    return want


@pytest.mark.parametrize("parallelization", [0, 1, 5])
@pytest.mark.parametrize("variant", C.VARIANTS)
def test_patterns_against_the_model(native, world, variant, parallelization):
    """Parallelization 0 is one launch; at 1 every block is a launch of its own and every planted boundary a seam (347
    launches per pass, 0.3 s on an MI355X: with all sixteen patterns in every form over the whole file this case took 8.3 s,
    so there the whole file goes through where_field for five of the patterns -- 3.6 s --, and the other patterns and forms
    see windows around the seam lines; parallelization 5, whose 70 launches afford the full list in every form, is added for
    that reason); at 5 the boundaries planted for cap 5 are seams."""
    e = world[variant]
    n, seams = e["n"], e["seam_lines"]
    names = [name for name, _, _, _ in FR.PATTERNS]
    with native.open(e["path"], parallelization=parallelization) as f:
        # the whole file
        for name in names if parallelization != 1 else ("get", "number", "filler", "folded", "end"):
            want = agree(f, e, name, "w" if parallelization == 1 else "wcs")
            assert 0 < len(want) < n, name
        if parallelization != 1:
            for name in ("get", "number", "filler", "empty"):
                assert len(agree(f, e, name, invert=True)) == n - len(selected(e, name))
        # the seam lines one by one, and their neighbours: where the host decides
        picked = seams if parallelization != 1 else seams[::5]
        for k, line in enumerate(picked):
            for name in ("get", "number", "end", "filler", "counter")[k % 2::2]:
                agree(f, e, name, "wc" if k % 3 else "wcs", first=max(line - 1, 0), count=3, invert=k % 4 == 3)
        assert sum(e["flags"]["get"][line] for line in seams) >= 3 and sum(not e["flags"]["get"][line] for line in seams) >= 3
        # the tail, or the last line
        assert agree(f, e, "get", first=n - 1) == [n - 1] and agree(f, e, "end", first=n - 1) == [n - 1]
        assert agree(f, e, "k-keys", first=n - 1) == [] and agree(f, e, "k-keys", first=n - 1, invert=True) == [n - 1]
        # three windows: inside, across the end, behind it; an empty one; limits
        for k, (first, count) in enumerate(((5, 700 if parallelization != 1 else 120), (n - 3, 10**12), (n, 4), (7, 0), (seams[2], 1))):
            agree(f, e, "ge-prefix", first=first, count=count, invert=k % 2 == 1)
            agree(f, e, "not-a-number", first=first, count=count)
        first = seams[len(seams) // 2] - 40
        total = len(selected(e, "folded", first=first, count=90))
        assert total > 5
        for limit in (0, 1, total - 1, total, total + 1):
            assert len(agree(f, e, "folded", first=first, count=90, limit=limit)) == min(limit, total)
        # a field that no line has: nothing matches, and the complement is every line
        assert f.where_field(1023, regex=rb"a*", first=n - 300).tolist() == []
        assert f.count_where_field(1023, regex=rb"a*", invert=True, first=n - 300) == 300
        if parallelization != 1:
            # one pattern over every field: a* matches every field that is present
            for j in FR.FIELDS:
                want = [i for i, field in enumerate(e["fields"][j] if j != 1023 else [None] * n) if field is not None]
                assert f.where_field(j, regex=rb"a*").tolist() == want, j
            assert f.count_where_field(1023, regex=rb"a*", invert=True) == n
        # a compiled object serves as well, and carries its own ignore_case
        assert f.where_field(1, regex=e["regexes"]["folded"], first=first, count=90).tolist() == selected(e, "folded", first=first, count=90)
        assert f.tell() == 0
    with native.IndexedBzip2File(e["path"], parallelization=parallelization) as f:
        assert f.where_field(1, regex=rb"^GET$", first=n - 1).tolist() == [n - 1]
        assert f.count_where_field(1, regex=rb"^get$", ignore_case=True, invert=True, first=n - 1) == 0


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import indexed_bzip2_amd as m

with m.open(sys.argv[2], parallelization=int(sys.argv[3])) as f:
    n = f.count_lines()
    for j, how in ((1, dict(regex=rb"^GET$")), (1, dict(regex=rb"^(get|put)s?$", ignore_case=True, invert=True, first=100, count=900, limit=70)),
                   (2, dict(regex=rb"^-?[0-9]+$", first=n - 400)), (3, dict(regex=rb"h;|,, ", first=50, count=600)),
                   (1, dict(regex=rb"never")), (2, dict(regex=rb"^-", limit=0)), (4, dict(regex=rb"tail", first=n - 200)),
                   (1023, dict(regex=rb"a*", invert=True, first=n - 5))):
        host = f.where_field(j, **how)
        got = f.where_field_to_tensor(j, **how)
        assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 1 and got.cpu().tolist() == host.tolist(), (j, how)
        numbers, lines = f.select_lines(j, **how)
        tn, data, offsets = f.select_lines_to_tensor(j, **how)
        assert data.dtype == torch.uint8 and data.is_cuda and offsets.dtype == torch.int64
        bounds, blob = offsets.tolist(), bytes(data.cpu().numpy())
        assert tn.tolist() == numbers.tolist() == host.tolist() and [blob[a:b] for a, b in zip(bounds, bounds[1:])] == lines, (j, how)
        assert f.count_where_field(j, **how) == len(host)
        print(j, sorted(how), len(host))
    # two calls intersect with torch: GET rows whose number is negative
    rows = f.where_field_to_tensor(1, regex=rb"^GET$")
    negative = f.where_field_to_tensor(2, regex=rb"^-[1-9]")
    both = rows[torch.isin(rows, negative)]
    ints = f.field_ints_to_tensor(2)
    assert len(both) > 5 and bool((ints[both] < 0).all())
    assert f.tell() == 0
print("where regex tensors ok")
"""


@pytest.mark.parametrize("parallelization", [0, 5])
def test_tensor_forms_equal_the_host_forms(native, world, parallelization):
    """In a process of its own that imports torch first; the host forms are pinned to the model above."""
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, world["tail"]["path"], str(parallelization)],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "where regex tensors ok" in run.stdout


def test_equivalences_that_need_no_model(native, world):
    e = world["tail"]
    assert b"\x01" not in e["raw"]
    for parallelization in (0, 5):
        with native.open(e["path"], parallelization=parallelization) as f:
            # an alternation of whole values is the value set
            want = f.where_field(1, values=[b"GE", b"GET", b"PUT"])
            assert len(want) > 100 and f.where_field(1, regex=rb"^(GE|GET|PUT)$").tolist() == want.tolist()
            assert f.where_field(1, regex=rb"^(GE|GET|PUT)$", invert=True).tolist() == f.where_field(1, values=[b"GE", b"GET", b"PUT"], invert=True).tolist()
            # with a delimiter that the file does not hold, field 0 is the line
            for pattern in G.FIXED_PATTERNS[::1 if parallelization == 0 else 6]:
                for fold in ((False, True) if parallelization == 0 else (False,)):
                    lines = f.grep_regex(pattern, ignore_case=fold)[0]
                    assert f.where_field(0, regex=pattern, ignore_case=fold, delimiter=b"\x01").tolist() == lines.tolist(), (pattern, fold)


def test_interleaved_with_other_calls_and_the_hold_rules(native, world):
    e = world["tail"]
    raw = e["raw"]
    lib = native.lib()
    N = native._native
    regex = e["regexes"]["get"]
    with native.open(e["path"], parallelization=5) as f:
        handle = f._open_reader()._h
        assert f.read(1000) == raw[:1000] and f.tell() == 1000
        spans = f.field_spans(1, 0, 500)
        numbers, lines = f.grep(b"endtail", limit=20)
        want = selected(e, "get", first=10, count=2000)
        n, matching = ctypes.c_uint64(), ctypes.c_uint64()
        assert lib.mi355x_bz2_reader_field_matches_regex(handle, NL, TAB, 1, regex._h, 0, 10, 2000, 50, 0, ctypes.byref(n),
                                                         ctypes.byref(matching)) == 0
        assert n.value == 50 and matching.value == len(want) > 50
        assert f.tell() == 1000
        # it released the lines grep held
        assert lib.mi355x_bz2_reader_take_line_ranges(handle, None, 0) == INVALID_ARGUMENT
        # the numbers stay held through calls of other families, and are taken as often as wanted
        assert f.grep(b"endtail", limit=20)[1] == lines
        assert [list(map(int, column)) for column in f.field_spans(1, 0, 500)] == [list(map(int, column)) for column in spans]
        for capacity in (50, 7, 50):
            out = np.full(51, ONES, dtype=np.uint64)
            assert lib.mi355x_bz2_reader_take_field_matches(handle, ctypes.c_void_p(out.ctypes.data), capacity, 0) == 0
            assert out[:capacity].tolist() == want[:capacity] and (out[capacity:] == ONES).all()
        # a selection by values releases the regex selection, and the reverse
        values = [b"PUT"]
        by_value = f.where_field(1, values=values, first=10, count=2000)
        assert 0 < len(by_value) != len(want)
        out = np.full(len(by_value), ONES, dtype=np.uint64)
        assert lib.mi355x_bz2_reader_take_field_matches(handle, ctypes.c_void_p(out.ctypes.data), len(out), 0) == 0
        assert out.tolist() == by_value.tolist()
        assert lib.mi355x_bz2_reader_field_matches_regex(handle, NL, TAB, 1, regex._h, 0, 10, 2000, 9, 0, ctypes.byref(n),
                                                         ctypes.byref(matching)) == 0
        out = np.full(len(by_value), ONES, dtype=np.uint64)
        assert lib.mi355x_bz2_reader_take_field_matches(handle, ctypes.c_void_p(out.ctypes.data), len(out), 0) == 0
        assert out[:9].tolist() == want[:9] and (out[9:] == ONES).all()
        # a count holds none
        assert f.count_where_field(1, regex=rb"^GET$") == len(selected(e, "get"))
        out = np.full(4, ONES, dtype=np.uint64)
        assert lib.mi355x_bz2_reader_take_field_matches(handle, ctypes.c_void_p(out.ctypes.data), 4, 0) == 0 and (out == ONES).all()
        # select_lines holds its lines as grep does, and no numbers of its own; grep releases them
        picked = f.select_lines(4, regex=rb"^endtail")
        assert picked[0].tolist() == [e["n"] - 1] and picked[1] == [e["whole_lines"][-1]]
        assert lib.mi355x_bz2_reader_take_field_matches(handle, None, 0, 0) == INVALID_ARGUMENT
        total = ctypes.c_uint64()
        assert lib.mi355x_bz2_reader_select_lines_regex(handle, NL, TAB, 1, regex._h, 0, 10, 2000, 6, 0, ctypes.byref(n), ctypes.byref(total)) == 0
        assert n.value == 6 and total.value == sum(len(e["whole_lines"][i]) for i in want[:6])
        taken, sizes = (ctypes.c_uint64 * 6)(), (ctypes.c_uint64 * 6)()
        assert lib.mi355x_bz2_reader_take_grep(handle, taken, sizes, 6) == 0 and list(taken) == want[:6]
        blob = ctypes.create_string_buffer(total.value)
        assert lib.mi355x_bz2_reader_take_line_ranges(handle, blob, 0) == 0
        assert blob.raw == b"".join(e["whole_lines"][i] for i in want[:6])
        assert f.grep(b"endtail", limit=20)[1] == lines
        assert f.read(500) == raw[1000:1500] and f.tell() == 1500
    # a closed reader refuses
    f = native.open(e["path"], parallelization=0)
    reader = f
    f.close()
    for call in (lambda: reader.where_field(1, regex=b"GET"), lambda: reader.count_where_field(2, regex=b"1"),
                 lambda: reader.select_lines(1, regex=b"GET")):
        with pytest.raises(Exception):
            call()
    wrapped = native.IndexedBzip2File(e["path"], parallelization=0)
    wrapped.close()
    with pytest.raises(ValueError):
        wrapped.where_field(1, regex=b"GET")


def blocks_decoded(f, call):
    before = f.statistics()["blocks_decoded"]
    call()
    return f.statistics()["blocks_decoded"] - before


@pytest.mark.parametrize("parallelization", [0, 5])
def test_every_block_is_decoded_once(native, world, parallelization):
    """On the corpus without a tail: one decode of every block, plus the blocks that hold a byte of the field of a line that
    crosses a launch seam."""
    e = world["closed"]
    raw, blocks = e["raw"], e["block_starts"]
    spans = F.direct(raw, NL, TAB, 1)
    with native.open(e["path"], parallelization=parallelization) as f:
        f.count_lines()
        once = blocks_decoded(f, lambda: f.field_spans(1))
        assert once == len(blocks)
        boundaries = C.boundaries_of(blocks, parallelization or 10**9)
        again = set()
        for b in boundaries:
            if raw[b - 1:b] == b"\n":
                continue
            start, size = spans[int(np.searchsorted(e["newlines"], b, "left"))]
            if size > 0:
                again.update(range(bisect.bisect_right(blocks, start) - 1, bisect.bisect_right(blocks, start + size - 1)))
        for regex in (rb"^GET$", rb"a*", rb"never"):
            got = blocks_decoded(f, lambda: f.count_where_field(1, regex=regex))
            print("parallelization", parallelization, regex, "field_spans", once, "count_where_field", got, "bound", once + len(again))
            # no key filters here: every seam line with a non-empty field is fetched, whatever the pattern
            assert got == once + len(again), regex
            assert blocks_decoded(f, lambda: f.where_field(1, regex=regex, invert=True)) == got
        if parallelization == 0:
            assert not again and got == once                            # one launch, no tail: nothing is decoded twice
        else:
            assert 10 < len(again) < len(blocks) // 3 and got > once


def test_tool(native, world):
    """--matches with --line-number, --invert-match and --ignore-case, against the Python result."""
    for k, (variant, options, j, how) in enumerate((
            ("tail", ["--where-field", "2", "--matches", "^GE", "--line-number"], 2, dict(regex=rb"^GE")),
            ("tail", ["--where-field", "1", "--matches", "^GE", "--line-number"], 1, dict(regex=rb"^GE")),
            ("closed", ["--where-field=1", "--matches=^GE", "--invert-match", "--line-number", "-P", "5"], 1, dict(regex=rb"^GE", invert=True)),
            ("tail", ["--where-field", "1", "--matches", "^ge", "--ignore-case", "-P", "5"], 1, dict(regex=rb"^ge", ignore_case=True)),
            ("tail", ["--where-field", "1", "--matches", "^ge"], 1, dict(regex=rb"^ge")),
            ("closed", ["--where-field", "3", "--matches", "h;|,, ", "--field-delimiter", "\\t"], 3, dict(regex=rb"h;|,, ")))):
        e = world[variant]
        with native.open(e["path"], parallelization=0) as f:
            numbers, lines = f.select_lines(j, **how)
        regex = native.compile_regex(how["regex"], how.get("ignore_case", False))
        want = [i for i, flag in enumerate(FR.flags_of(regex, e["fields"][j])) if flag != how.get("invert", False)]
        assert numbers.tolist() == want
        numbered = "--line-number" in options
        run = subprocess.run([CLI] + options + [e["path"]], capture_output=True, timeout=300)
        assert run.returncode == 0, (options, run.stderr)               # 0 whether or not a line was selected
        assert run.stdout == b"".join((b"%d:" % (i + 1) if numbered else b"") + line for i, line in zip(numbers.tolist(), lines)), options
        assert (len(want) == 0) == (k in (0, 4)), (k, len(want))        # field 2 holds numbers, and no key is lower case
