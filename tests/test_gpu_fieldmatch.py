"""Lines selected by a field, on the GPU: the kernel under Decoder.match_fields (k_field_match behind the field-hash
passes) on one decoded text of about 150 kB, the reader's where_field / count_where_field / select_lines and their tensor
forms on a corpus of several launches, the count of decoded blocks, and the tool's --where-field.

The reference is the plain Python model of fieldmatch.py -- bytes.split per line, `in` on a Python set, and
parse_field_number with integer comparisons --, never the code under test.  Every comparison is exact."""
import bisect
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import datagen
import fieldmatch as FM
import fields as F

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
NL, TAB = 10, 9
ONES = 2**64 - 1                                               # what Decoder.match_fields fills `flags` with
INVALID_ARGUMENT, CLOSED = 103, 106
THREADS, BLOCKS = 256, 512                                     # of k_field_match: a grid covers THREADS * BLOCKS lines
P255, Q256 = b"p" * 255, b"q" * 256
LAST = b"the-last-field"


# ------------------------------------------------------------------------------------------------ the kernel

def device_text():
    """About 150 kB of tab-separated lines whose field 1 is drawn from a small vocabulary -- with the sizes 0, 1, 255, 256
    and 257, a value that is a prefix of another, bytes 0x80..0xFF and the newline's neighbours --, lines without field 1,
    and an unterminated tail whose last field ends on the last byte."""
    rng = random.Random(0xF1E1D)
    common = [b"", b"x", b"GET", b"GE", b"GETS", b"PUT", b"\x0b\x0c", b"\x80\xff", b"\xfe", b"404", b"-7"]
    long_ones = [P255, Q256, Q256 + b"q", Q256[:255] + b"r"]
    rare = [b"w%d" % i for i in range(1200)]
    out = bytearray()
    while len(out) < 150_000:
        pad = bytes(rng.choice(b"abc") for _ in range(rng.randrange(0, 18)))
        if rng.randrange(12) == 0:
            out += pad + b"\n"                                     # no field 1
        else:
            kind = rng.randrange(20)
            out += pad + b"\t" + rng.choice(long_ones if kind == 0 else rare if kind < 8 else common) + b"\t" + pad[:3] + b"\n"
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
    columns = {}
    for seed in (0, 1):
        _, keys, starts, sizes = dec.field_hashes([(0, total)], 1, seed=seed)
        assert len(keys) == len(fields) and [int(s) for s in sizes] == [-1 if f is None else len(f) for f in fields]
        columns[seed] = (keys, starts, sizes)
    assert {int(s) % 16 for s, f in zip(columns[0][1], fields) if f == b"GET"} == set(range(16))      # every alignment
    yield {"dec": dec, "text": text, "fields": fields, "columns": columns}
    dec.close()


def check(device, values, n=None, seed=0, base=0, keys=None, room_behind=8):
    """Decoder.match_fields over the first n lines against the model, exactly; the words behind n stay as they were."""
    all_keys, starts, sizes = device["columns"][seed]
    keys = all_keys if keys is None else keys
    n = len(keys) if n is None else n
    wanted = {bytes(v) for v in values}
    want = [1 if f is not None and f in wanted else 0 for f in device["fields"][:n]]
    got = device["dec"].match_fields(values, keys[:n], starts[:n] + np.uint64(base), sizes[:n], base=base, seed=seed, room=n + room_behind)
    assert got.dtype == np.uint64 and len(got) == n + room_behind
    assert got[:n].tolist() == want, next(i for i, (a, b) in enumerate(zip(got[:n].tolist(), want)) if a != b)
    assert (got[n:] == ONES).all(), "written behind n"
    return sum(want)


def test_line_counts_and_the_canary(device):
    values = [b"GET", b"", b"\x80\xff"]
    for n in (0, 1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1, None):
        check(device, values, n)
    assert check(device, values) > 300


def test_sets_of_1_2_1023_and_1024_values(device):
    present = sorted({f for f in device["fields"] if f is not None and len(f) < 12})
    assert len(present) > 500
    for n in (1, 2, 1023, 1024):
        some = present[:n // 2 + 1] + [b"never-%d" % i for i in range(n)]
        assert check(device, some[:n]) > 0, n
        assert check(device, [b"never-%d" % i for i in range(n)]) == 0, n
    # equal values count once; a prefix of a value is another value
    assert check(device, [b"GE", b"GE", b"GE"]) == device["fields"].count(b"GE") > 0
    assert check(device, [b"G", b"GETSS"]) == 0


def test_value_sizes_and_the_field_of_257_bytes(device):
    fields = device["fields"]
    for value in (b"", b"x", P255, Q256):
        assert check(device, [value]) == fields.count(value) > 0, len(value)
    # the lines whose field is 257 bytes and begins with the value give 0, and so does the field that differs in byte 255
    assert fields.count(Q256 + b"q") > 0 and fields.count(Q256[:255] + b"r") > 0
    assert check(device, [Q256, P255, b"", b"x"]) == sum(fields.count(v) for v in (Q256, P255, b"", b"x"))
    # bytes 0x80..0xFF and the newline's neighbours
    assert check(device, [b"\x0b\x0c", b"\x80\xff", b"\xfe"]) == sum(fields.count(v) for v in (b"\x0b\x0c", b"\x80\xff", b"\xfe")) > 0


def test_the_answer_does_not_depend_on_the_seed(device):
    for seed in (0, 1):
        check(device, [b"GET", b"PUT", b"", b"404"], seed=seed)


def test_the_grid_strides(native, device):
    """More than twice the lines one grid covers: the columns of the text's lines, repeated."""
    keys, starts, sizes = device["columns"][0]
    n = 2 * THREADS * BLOCKS + 5
    times = n // len(keys) + 1
    values = [b"GET", b"w7", b""]
    wanted = set(values)
    want = np.tile(np.array([1 if f in wanted else 0 for f in device["fields"]], dtype=np.uint64), times)[:n]
    got = device["dec"].match_fields(values, np.tile(keys, times)[:n], np.tile(starts, times)[:n], np.tile(sizes, times)[:n], room=n + 8)
    assert np.array_equal(got[:n], want) and (got[n:] == ONES).all()
    assert want.sum() > 1000


def test_base_beyond_32_bits(device):
    for base in (2**32 + 5, 2**64 - 3):
        check(device, [b"GET", b"", Q256], base=base)


def test_forged_keys_do_not_match(native, device):
    """A keys column in which lines that do not match carry the key of a value -- also lines whose field has the value's
    size -- must still give 0: the bytes decide."""
    keys, starts, sizes = device["columns"][0]
    for value, others in ((b"GET", (b"PUT", b"404")), (Q256, (Q256[:255] + b"r",)), (b"x", ())):
        forged = keys.copy()
        forged[[i for i, f in enumerate(device["fields"]) if f != value]] = native.line_hash(value)
        assert sum(1 for f in device["fields"] if f in others) >= len(others)       # same size, other bytes
        assert check(device, [value], keys=forged) == device["fields"].count(value)
    # and the other way round: a matching line under another key is no match, the key filters
    forged = keys.copy()
    at = device["fields"].index(b"GET")
    forged[at] = native.line_hash(b"PUT")
    got = device["dec"].match_fields([b"GET"], forged, starts, sizes)
    assert got[at] == 0 and got.sum() == device["fields"].count(b"GET") - 1


def test_a_field_that_ends_on_the_last_byte_and_spans_outside(native, device):
    end = len(device["text"])
    assert device["text"].endswith(b"\t" + LAST)
    key = native.line_hash(LAST)
    n = len(LAST)
    keys = np.array([key] * 6, dtype=np.uint64)
    starts = np.array([end - n, end - n + 1, end - n - 1, end, end + 1, 2**63], dtype=np.uint64)
    sizes = np.array([n] * 6, dtype=np.int64)
    # only the first lies where the value lies; the second and the last three do not lie inside the output and are not read
    assert device["dec"].match_fields([LAST], keys, starts, sizes).tolist() == [1, 0, 0, 0, 0, 0]
    # an empty field at the very end is inside; a missing one never matches
    empty = native.line_hash(b"")
    got = device["dec"].match_fields([b""], [empty] * 4, [end, end + 1, 0, end], [0, 0, 0, -1])
    assert got.tolist() == [1, 0, 1, 0]


def test_refusals_come_before_any_launch(native, device):
    keys, starts, sizes = (column[:4] for column in device["columns"][0])
    for values, why in (([], "1 to 1024 values, not 0"), ([b"x"] * 1025, "1 to 1024 values, not 1025"), ([b"v" * 257], "value 0 has 257 bytes"),
                        ([b"%04d" % i + b"p" * 252 for i in range(64)] + [b"q"], "at most 16384 bytes in total, not 16385")):
        with pytest.raises(native.Bz2Error) as refused:
            device["dec"].match_fields(values, keys, starts, sizes, check=False)
        assert refused.value.status == INVALID_ARGUMENT and why in str(refused.value)
    with pytest.raises(ValueError):
        device["dec"].match_fields([b"a"], keys, starts[:3], sizes)


# ------------------------------------------------------------------------------------------------ the reader

TAIL = b"id-tail\tTAILMETHOD\t42\tfill\tend-tail"


def reader_text(tail=True):
    """About 700 kB of records `id TAB method TAB number TAB filler TAB id`, both ids unique to the line, among them lines
    with fewer fields, empty lines and numbers that are none; with an unterminated tail or none."""
    rng = random.Random(0x5E1EC7)
    out = bytearray()
    methods = [b"GET"] * 60 + [b"PUT"] * 25 + [b"POST"] * 10 + [b"", b"GE", b"GETS", b"\x80\xff", b"DELETE"]
    n = 0
    while len(out) < 700_000:
        kind = rng.randrange(40)
        if kind == 0:
            out += b"\n"
        elif kind == 1:
            out += b"id%07d\tshort\n" % n
        else:
            number = rng.choice([b"%d" % rng.randrange(-300, 600), b"%d" % rng.randrange(-300, 600), b"", b"n/a", b"+5", b"1e3",
                                 b"%d" % rng.randrange(10**17, 10**18)])
            filler = bytes(rng.choice(b"abcdefgh ") for _ in range(rng.randrange(0, 200)))
            out += b"id%07d\t" % n + rng.choice(methods) + b"\t" + number + b"\t" + filler + b"\tend%07d\n" % n
        n += 1
    out += b"id%07d\tONCE\t-300\t\tend%07d\n" % (n, n)
    return bytes(out) + (TAIL if tail else b"")


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("fieldmatch")
    files = {}
    for name in ("tail", "closed"):
        raw = reader_text(name == "tail")
        path = folder / (name + ".bz2")
        path.write_bytes(datagen.compress(raw, 1))
        starts = [0]
        for line in raw.split(b"\n")[:-1]:
            starts.append(starts[-1] + len(line) + 1)
        with native.open(str(path), parallelization=0) as f:
            blocks = [b for b in sorted(f.block_offsets().values()) if b < len(raw)]
        assert len(blocks) >= 6
        # computed once, shared, left unchanged.  At parallelization 1 every block is a launch of its own: the lines that
        # hold a block boundary inside them cross a launch seam
        seam_lines = sorted({bisect.bisect_right(starts, b) - 1 for b in blocks[1:] if raw[b - 1:b] != b"\n"})
        files[name] = {"raw": raw, "path": str(path), "starts": starts, "blocks": blocks, "seam_lines": seam_lines,
                       "lines": FM.lines_with_delimiters(raw, NL), "fields": {j: F.fields_of(raw, NL, TAB, j) for j in range(5)},
                       "numbers": None}
        assert len(seam_lines) >= 4
    return files


def model(entry, native, j, values=None, between=None, **how):
    if values is not None:
        wanted = {bytes(v) for v in values}
        flags = [f is not None and f in wanted for f in entry["fields"][j]]
    else:
        if entry["numbers"] is None:                               # parse_field_number is pinned to the model by the CPU tests
            entry["numbers"] = {}
        if j not in entry["numbers"]:
            entry["numbers"][j] = [None if f is None else native.parse_field_number(f) for f in entry["fields"][j]]
        lo, hi = FM.clipped(between)
        flags = [x is not None and lo <= x <= hi for x in entry["numbers"][j]]
    return FM.selected(flags, **how)


def agree(f, entry, native, j, **how):
    """where_field, count_where_field and select_lines against the model."""
    want = model(entry, native, j, **how)
    got = f.where_field(j, **how)
    assert got.dtype == np.uint64 and got.tolist() == want, (j, how, len(got), len(want))
    assert f.count_where_field(j, **how) == len(want), (j, how)
    numbers, lines = f.select_lines(j, **how)
    assert numbers.tolist() == want and lines == [entry["lines"][i] for i in want], (j, how)
    return want


@pytest.mark.parametrize("parallelization", [0, 1])
@pytest.mark.parametrize("name", ["tail", "closed"])
def test_values_against_the_model(native, corpus, name, parallelization):
    entry = corpus[name]
    n = len(entry["lines"])
    with native.open(entry["path"], parallelization=parallelization) as f:
        assert len(agree(f, entry, native, 1, values=[b"GET"])) > 3000                   # often
        assert agree(f, entry, native, 1, values=[b"ONCE"]) == [n - 1 - (name == "tail")]    # once
        assert agree(f, entry, native, 1, values=[b"NEVER", b"G"]) == []                  # never
        assert len(agree(f, entry, native, 1, values=[b"", b"GE", b"\x80\xff", b"GETS", b"GE"])) > 100
        assert len(agree(f, entry, native, 1, values=[b""])) > 10                        # empty and present, never missing
        assert agree(f, entry, native, 4, values=[b""]) == [] and agree(f, entry, native, 3, values=[b""])
        # a value that occurs only in a line that crosses a launch seam: its first field, its last, and the field the seam
        # cuts
        for line in entry["seam_lines"]:
            for j in (0, 4):
                value = entry["fields"][j][line]
                if value is not None and len(value) <= 256:
                    assert agree(f, entry, native, j, values=[value, b"id-none"]) == [line], (line, j)
            boundary = next(b for b in entry["blocks"][1:] if entry["starts"][line] < b < entry["starts"][line] + len(entry["lines"][line]))
            cut = entry["lines"][line][:boundary - entry["starts"][line]].count(b"\t")
            value = entry["fields"][cut][line]
            if len(value) <= 256:
                assert line in agree(f, entry, native, cut, values=[value]), (line, cut)
                assert line not in agree(f, entry, native, cut, values=[value[:-1] + b"#"]), (line, cut)
        assert any(entry["fields"][4][line] is not None for line in entry["seam_lines"])
        # all the seam lines at once, and their complement
        ids = [entry["fields"][0][line] for line in entry["seam_lines"]]
        assert agree(f, entry, native, 0, values=ids) == entry["seam_lines"]
        assert len(agree(f, entry, native, 0, values=ids, invert=True)) == n - len(ids)
        if name == "tail":
            assert agree(f, entry, native, 1, values=[b"TAILMETHOD"]) == [n - 1]
            assert agree(f, entry, native, 4, values=[b"end-tail"]) == [n - 1]
            assert agree(f, entry, native, 4, values=[b"end-tai", b"end-tail2", b"end-tailend-tail"]) == []
            assert agree(f, entry, native, 3, values=[b"fill"], first=n - 1) == [n - 1]
            assert n - 1 not in agree(f, entry, native, 1, values=[b"TAILMETHOD"], invert=True, first=n - 5)
        # invert selects the lines without the field too
        inverted = agree(f, entry, native, 1, values=[b"GET", b"PUT", b"POST"], invert=True)
        assert any(entry["fields"][1][i] is None for i in inverted)
        # windows and limits
        seam = entry["seam_lines"][1]
        for k, (first, count) in enumerate(((0, 1), (5, 700), (seam, 1), (seam - 2, 5), (seam + 1, 3000), (n - 3, 3), (n - 2, 10**12),
                                            (n, 4), (7, 0))):
            agree(f, entry, native, 1, values=[b"GET", b""], first=first, count=count, invert=k % 2 == 1)
        total = len(model(entry, native, 1, values=[b"PUT"]))
        for limit in (0, 1, total - 1, total, total + 1):
            assert len(agree(f, entry, native, 1, values=[b"PUT"], limit=limit)) == min(limit, total)
        # the answer is the same under every seed
        for j, values in ((1, [b"GET", b"", b"ONCE"]), (0, ids)):
            want = model(entry, native, j, values=values)
            for seed in (0, 1, 2):
                assert f.where_field(j, values=values, seed=seed).tolist() == want, seed
        assert f.tell() == 0
    with native.IndexedBzip2File(entry["path"], parallelization=parallelization) as f:
        assert f.where_field(1, values=[b"ONCE"]).tolist() == [n - 1 - (name == "tail")]
        assert f.count_where_field(1, values=[b"ONCE"], invert=True) == n - 1


@pytest.mark.parametrize("parallelization", [0, 1])
@pytest.mark.parametrize("name", ["tail", "closed"])
def test_ranges_against_the_model(native, corpus, name, parallelization):
    entry = corpus[name]
    n = len(entry["lines"])
    with native.open(entry["path"], parallelization=parallelization) as f:
        everything = agree(f, entry, native, 2, between=(None, None))                    # all the numbers
        assert 1000 < len(everything) < n                                               # the column holds non-numbers and missing fields
        assert len(agree(f, entry, native, 2, between=(None, None), invert=True)) == n - len(everything)
        agree(f, entry, native, 2, between=(10**18, None))                              # clipped to the largest number there is
        assert agree(f, entry, native, 2, between=(600, 10**17 - 1)) == []               # none
        assert agree(f, entry, native, 2, between=(5, 4)) == []                          # lo > hi
        assert len(agree(f, entry, native, 2, between=(5, 4), invert=True)) == n
        assert len(agree(f, entry, native, 2, between=(-300, -1))) > 100                 # negative bounds
        assert len(agree(f, entry, native, 2, between=(-10**30, -1))) > 100 and len(agree(f, entry, native, 2, between=(0, 10**30))) > 100
        assert len(agree(f, entry, native, 2, between=(500, 599))) > 10
        assert len(agree(f, entry, native, 2, between=(5, 5))) >= 1                      # lo = hi; "+5" is 5
        big = next(x for x in model_numbers(entry, native, 2) if x is not None and x >= 10**17)
        assert agree(f, entry, native, 2, between=(big, big)) == [model_numbers(entry, native, 2).index(big)]     # one line
        assert agree(f, entry, native, 0, between=(None, None)) == []                    # ids are no numbers
        assert len(agree(f, entry, native, 4, between=(None, None), invert=True)) == n
        if name == "tail":
            assert agree(f, entry, native, 2, between=(42, 42), first=n - 4) == [n - 1]
        seam = entry["seam_lines"][0]
        for first, count in ((seam, 1), (seam - 3, 7), (n - 2, 5), (n, 1)):
            agree(f, entry, native, 2, between=(0, 300), first=first, count=count)
        total = len(model(entry, native, 2, between=(-300, -200)))
        for limit in (0, 1, total - 1, total, total + 1):
            agree(f, entry, native, 2, between=(-300, -200), limit=limit)
        assert f.tell() == 0


def model_numbers(entry, native, j):
    model(entry, native, j, between=(None, None))
    return entry["numbers"][j]


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import indexed_bzip2_amd as m

with m.open(sys.argv[2], parallelization=int(sys.argv[3])) as f:
    for j, how in ((1, dict(values=[b"GET", b""])), (1, dict(values=[b"PUT"], invert=True, first=100, count=5000, limit=70)),
                   (2, dict(between=(500, 599))), (2, dict(between=(None, -1), first=3000)), (1, dict(values=[b"NEVER"])),
                   (2, dict(between=(0, 10), limit=0)), (4, dict(values=[b"end-tail"]))):
        host = f.where_field(j, **how)
        got = f.where_field_to_tensor(j, **how)
        assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 1 and got.cpu().tolist() == host.tolist(), (j, how)
        numbers, lines = f.select_lines(j, **how)
        tn, data, offsets = f.select_lines_to_tensor(j, **how)
        assert data.dtype == torch.uint8 and data.is_cuda and offsets.dtype == torch.int64
        bounds, blob = offsets.tolist(), bytes(data.cpu().numpy())
        assert tn.tolist() == numbers.tolist() == host.tolist() and [blob[a:b] for a, b in zip(bounds, bounds[1:])] == lines, (j, how)
        print(j, sorted(how), len(host))
    # the numbers index the other columns' tensors
    first = 200
    rows = f.where_field_to_tensor(2, between=(500, 599), first=first)
    ints = f.field_ints_to_tensor(2, first=first)
    picked = ints[rows - first]
    assert len(rows) > 10 and bool(((picked >= 500) & (picked <= 599)).all())
    others = torch.ones(len(ints), dtype=torch.bool, device=ints.device)
    others[rows - first] = False
    rest = ints[others]
    assert not bool(((rest >= 500) & (rest <= 599)).any())
    keys = f.field_hashes_to_tensor(1, first=first)
    rows = f.where_field_to_tensor(1, values=[b"POST"], first=first)
    assert len(rows) > 10 and bool((keys[rows - first] == m.line_hash(b"POST")).all())
    assert f.tell() == 0
print("where tensors ok")
"""


@pytest.mark.parametrize("parallelization", [0, 1])
def test_tensor_forms_equal_the_host_forms(native, corpus, parallelization):
    """In a process of its own that imports torch first; the host forms are pinned to the model above."""
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, corpus["tail"]["path"], str(parallelization)],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "where tensors ok" in run.stdout


def test_interleaved_with_other_calls_and_the_hold_rules(native, corpus):
    entry = corpus["tail"]
    raw = entry["raw"]
    lib = native.lib()
    N = native._native
    with native.open(entry["path"], parallelization=1) as f:
        handle = f._open_reader()._h
        assert lib.mi355x_bz2_reader_take_field_matches(handle, None, 0, 0) == INVALID_ARGUMENT          # nothing is held
        assert f.read(1000) == raw[:1000] and f.tell() == 1000
        keys = f.field_hashes(1, 0, 500)
        numbers, lines = f.grep(b"ONCE", limit=20)
        want = model(entry, native, 1, values=[b"PUT"], first=10, count=2000)
        n, matching = ctypes.c_uint64(), ctypes.c_uint64()
        assert lib.mi355x_bz2_reader_field_matches(handle, NL, TAB, 1, *N.value_set([b"PUT"]), 0, 0, 10, 2000, 50, 0, ctypes.byref(n),
                                                   ctypes.byref(matching)) == 0
        assert n.value == 50 and matching.value == len(want)
        assert f.tell() == 1000
        # it released the lines grep held, and not the field hashes
        assert lib.mi355x_bz2_reader_take_line_ranges(handle, None, 0) == INVALID_ARGUMENT
        taken = np.zeros(500, dtype=np.uint64)
        assert lib.mi355x_bz2_reader_take_field_hashes(handle, ctypes.c_void_p(taken.ctypes.data), 500, 0) == 0
        assert taken.tolist() == keys.tolist()
        # the numbers stay held through calls of other families, and are taken as often as wanted
        assert f.grep(b"ONCE", limit=20)[1] == lines
        assert f.read_line_ranges([(3, 2)]) == [b"".join(entry["lines"][3:5])]
        assert f.field_hashes(1, 0, 500).tolist() == keys.tolist()
        for capacity in (50, 7, 50):
            out = np.full(51, ONES, dtype=np.uint64)
            assert lib.mi355x_bz2_reader_take_field_matches(handle, ctypes.c_void_p(out.ctypes.data), capacity, 0) == 0
            assert out[:capacity].tolist() == want[:capacity] and (out[capacity:] == ONES).all()
        # the next call of the family replaces them; a count holds none
        assert f.count_where_field(2, between=(0, 5)) == len(model(entry, native, 2, between=(0, 5)))
        out = np.full(4, ONES, dtype=np.uint64)
        assert lib.mi355x_bz2_reader_take_field_matches(handle, ctypes.c_void_p(out.ctypes.data), 4, 0) == 0 and (out == ONES).all()
        # select_lines holds its lines as grep does, and no numbers of its own
        assert f.select_lines(1, values=[b"ONCE"])[1] == lines
        assert lib.mi355x_bz2_reader_take_field_matches(handle, None, 0, 0) == INVALID_ARGUMENT
        assert f.read(500) == raw[1000:1500] and f.tell() == 1500
    # a closed reader refuses
    f = native.open(entry["path"], parallelization=0)
    reader = f
    f.close()
    for call in (lambda: reader.where_field(1, values=[b"GET"]), lambda: reader.count_where_field(2, between=(1, 2)),
                 lambda: reader.select_lines(1, values=[b"GET"])):
        with pytest.raises(Exception):
            call()
    wrapped = native.IndexedBzip2File(entry["path"], parallelization=0)
    wrapped.close()
    with pytest.raises(ValueError):
        wrapped.where_field(1, values=[b"GET"])


def blocks_decoded(f, call):
    before = f.statistics()["blocks_decoded"]
    call()
    return f.statistics()["blocks_decoded"] - before


@pytest.mark.parametrize("parallelization", [0, 1])
def test_every_block_is_decoded_once(native, corpus, parallelization):
    entry = corpus["tail"]
    raw, blocks, starts = entry["raw"], entry["blocks"], entry["starts"]
    with native.open(entry["path"], parallelization=parallelization) as f:
        f.count_lines()
        hashes = blocks_decoded(f, lambda: f.field_hashes(1))
        ints = blocks_decoded(f, lambda: f.field_ints(2))
        assert hashes == ints == len(blocks)
        # a value the file does not hold: no candidate, no second decode
        assert blocks_decoded(f, lambda: f.count_where_field(1, values=[b"NEVER"])) == hashes
        assert blocks_decoded(f, lambda: f.where_field(1, values=[b"NEVER"], invert=True)) == hashes
        assert blocks_decoded(f, lambda: f.count_where_field(2, between=(0, 100))) == ints
        assert blocks_decoded(f, lambda: f.where_field(2, between=(0, 100))) == ints
        # present values: beyond one decode, at most the blocks that hold a byte of field 1 of a seam line or of the tail
        candidates = list(entry["seam_lines"]) + [len(entry["lines"]) - 1]
        again = set()
        for line in candidates:
            parts = entry["lines"][line].rstrip(b"\n").split(b"\t")
            if len(parts) > 1 and len(parts[1]) > 0:
                begin = starts[line] + len(parts[0]) + 1
                again.update(range(bisect.bisect_right(blocks, begin) - 1, bisect.bisect_right(blocks, begin + len(parts[1]) - 1)))
        values = sorted({entry["fields"][1][line] for line in candidates if entry["fields"][1][line]})
        assert values and len(again) >= 1
        got = blocks_decoded(f, lambda: f.count_where_field(1, values=values + [b"TAILMETHOD"]))
        print("parallelization", parallelization, "field_hashes", hashes, "count_where_field", got, "bound", hashes + len(again))
        assert hashes <= got <= hashes + len(again)
        if parallelization == 0:
            # one launch: only the tail is a candidate
            assert got <= hashes + 1


def test_tool(native, corpus, tmp_path):
    """Each of the three forms, --invert-match and --line-number; one run per case, every second one numbered."""
    values = tmp_path / "values.txt"
    values.write_bytes(b"PUT\nONCE\nTAILMETHOD\nnever\n")
    for k, (name, options, j, how) in enumerate((
            ("tail", ["--where-field", "1", "--equals", "POST"], 1, dict(values=[b"POST"])),
            ("closed", ["--where-field=1", "--equals=", "-P", "1"], 1, dict(values=[b""])),
            ("tail", ["--where-field", "1", "--in-file", str(values), "-P", "1", "--seed", "5"], 1,
             dict(values=[b"PUT", b"ONCE", b"TAILMETHOD", b"never"])),
            ("tail", ["--where-field", "2", "--between", "500,599"], 2, dict(between=(500, 599))),
            ("closed", ["--where-field", "2", "--between=,-250", "--invert-match", "-P", "1"], 2, dict(between=(None, -250), invert=True)),
            ("tail", ["--where-field", "4", "--equals", "end-tai", "--field-delimiter", "\\t"], 4, dict(values=[b"end-tai"])))):
        entry = corpus[name]
        want = model(entry, native, j, **how)
        numbered = k % 2 == 1
        run = subprocess.run([CLI] + options + (["--line-number"] if numbered else []) + [entry["path"]], capture_output=True, timeout=300)
        assert run.returncode == 0, (options, run.stderr)               # 0 whether or not a line was selected
        assert run.stdout == b"".join((b"%d:" % (i + 1) if numbered else b"") + entry["lines"][i] for i in want), options
    assert want == []                                                   # the last case selects nothing, and its status is 0 too
