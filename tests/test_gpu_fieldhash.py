"""Field hashes on the GPU: the kernels under Decoder.field_hashes (k_fieldhash_emit, k_fieldhash_finish behind the field
and line-hash passes), the reader's field_hashes / field_hashes_to_tensor / count_by_field / value_counts, and the tool's
--count-by-field.

The reference is the plain Python model of fieldhash.py -- bytes.split per line, a Python restatement of the hash, and its
own summarise and stitch -- never the code under test.  Keys, offsets, sizes, counts and bytes are compared exactly.  The
texts and the corpus are those of test_gpu_fields.py: the shapes at which the kernels can go wrong are the same."""
import collections
import ctypes
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import datagen
import fieldhash as FH
import fields as F
import linehash as LH
import test_gpu_fields as TF

pytestmark = pytest.mark.gpu

CLI = TF.CLI
NL, TAB = TF.NL, TF.TAB
ONES, UNTOUCHED = TF.ONES, TF.UNTOUCHED
SIZES, EDGES = TF.SIZES, TF.EDGES
SUMMARY_KEYS = FH.FIELD_KEYS + FH.HASH_KEYS


# ------------------------------------------------------------------------------------------------ the kernels

@pytest.fixture(scope="module")
def device(native):
    text, where = TF.device_text()
    dec = TF.decoded(native, text)
    yield {"dec": dec, "text": text, "where": where, "models": {}, "texts": {}}
    dec.close()


def model_of(device, span, field, nl, dl, seed, prefixes=True):
    """The model's summary of a span, computed once per (span, field, nl, dl, seed), shared, left unchanged; the prefix
    hashes of the text once per seed."""
    if seed not in device["texts"]:
        device["texts"][seed] = FH.Text(device["text"], LH.base(seed), prefixes)
    key = (span, field, nl, dl, seed)
    if key not in device["models"]:
        device["models"][key] = device["texts"][seed].summary(span[0], span[1], nl, dl, field)
    return device["models"][key]


def check_spans(device, spans, field=1, nl=NL, dl=TAB, seed=0, capacity=None, room=None, prefixes=True):
    """Summaries, head hashes, keys, starts and sizes of Decoder.field_hashes against the model, exactly; returns the
    model's (key, start, size) per closed line."""
    models = [model_of(device, span, field, nl, dl, seed, prefixes) for span in spans]
    summaries, keys, starts, sizes = device["dec"].field_hashes(spans, field, bytes([dl]), bytes([nl]), seed, capacity, room)
    assert keys.dtype == np.uint64 and starts.dtype == np.uint64 and sizes.dtype == np.int64
    for span, model, got in zip(spans, models, summaries):
        assert got == {key: model[key] for key in SUMMARY_KEYS}, (span, field, seed)
    wanted = [(key, span[0] + start, size) for span, model in zip(spans, models)
              for key, (start, size) in zip(model["keys"], model["fields"])]
    written = len(wanted) if capacity is None else min(capacity, len(wanted))
    assert keys[:written].tolist() == [k for k, _, _ in wanted[:written]], (spans[:3], field, seed)
    assert starts[:written].tolist() == [s for _, s, _ in wanted[:written]], (spans[:3], field)
    assert sizes[:written].tolist() == [n for _, _, n in wanted[:written]], (spans[:3], field)
    assert (keys[written:] == ONES).all() and (starts[written:] == ONES).all() and (sizes[written:] == UNTOUCHED).all(), \
        "written at or beyond the capacity"
    return wanted


def test_span_sizes_at_every_alignment(native, device):
    base = device["where"]["lines"][0]
    base += -base % 16                                              # the output buffer is 16-byte aligned
    spans = [(base + start, size) for start in range(16) for size in SIZES]
    assert {o % 16 for o, _ in spans} == set(range(16))
    wanted = check_spans(device, spans)
    missing = sum(1 for key, _, size in wanted if key == FH.MISSING)
    assert len(wanted) > 10_000 and 1000 < missing < len(wanted) - 1000
    assert all((key == FH.MISSING) == (size < 0) for key, _, size in wanted)
    # a key is the CPU's line hash of the field's bytes
    text = device["text"]
    for key, start, size in wanted[:200]:
        assert size < 0 or key == native.line_hash(text[start:start + size])
    check_spans(device, spans[::5], seed=0xDEADBEEF)                # another base
    for field in (0, 7, 1023):
        check_spans(device, spans[::7], field)
    # other delimiters: ',' between fields; 0 between lines, "\n" then a byte like any other
    check_spans(device, spans[3::11], 1, dl=ord(","))
    check_spans(device, spans[5::11], 0, nl=0)
    check_spans(device, spans[5::11], 1, nl=0, dl=NL, seed=0xDEADBEEF)
    # the whole output as one span, and the same span twice
    whole = (0, len(text))
    check_spans(device, [whole, spans[20], whole])
    check_spans(device, [whole], 0, seed=0xDEADBEEF)
    # without the span columns the keys are the same
    dec, lib = device["dec"], native.lib()
    again = dec.field_hashes([whole], 1)[1]
    summaries = (native._native.FieldHashSummary * 1)()
    arr = (native._native.ByteSpan * 1)(native._native.ByteSpan(*whole))
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    keys, pointer = np.zeros(len(again), dtype=np.uint64), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(pointer), keys.nbytes) == 0
    try:
        assert lib.mi355x_bz2_field_hashes(dec._h, arr, 1, NL, TAB, 1, 0, summaries, None, None, pointer, None, None, len(keys)) == 0
        assert hip.hipMemcpy(keys.ctypes.data, pointer, keys.nbytes, 2) == 0
    finally:
        hip.hipFree(pointer)
    assert keys.tolist() == again.tolist() and summaries[0].count == len(again)


def test_delimiters_on_chunk_and_tile_edges(device):
    text = device["text"]
    for name, value in (("edges-nl", NL), ("edges-dl", TAB)):
        offset, size = device["where"][name]
        assert offset % 16 == 0 and all(text[offset + k] == value for k in EDGES)
        for field in (0, 1, 7):
            # the delimiters at exactly these offsets of a span, and one and two bytes in front of them
            check_spans(device, [(offset + shift, size - shift) for shift in (0, 1, 2)], field)
        # a delimiter as a span's first byte, as its last byte, and as all of it
        for k in EDGES:
            spans = [(offset + k, 300), (offset + k - 299, 300), (offset + k, 1), (offset + k, EDGES[-1] + 300 - k)]
            check_spans(device, spans, 0)
            check_spans(device, spans, 1)
    # the two roles swapped: the tabs close the lines and the newlines part the fields
    for name in ("edges-nl", "edges-dl"):
        check_spans(device, [device["where"][name]], 1, nl=TAB, dl=NL)
        check_spans(device, [device["where"][name]], 0, nl=TAB, dl=NL, seed=0xDEADBEEF)


def test_empty_lines_and_lines_without_and_of_delimiters(device):
    where = device["where"]
    offset, size = where["empty-lines"]
    wanted = check_spans(device, [(offset, size), (offset + 1, 255), (offset + 3, 256), (offset + 5, 513)], 0)
    assert wanted[:700] == [(0, offset + k, 0) for k in range(700)]                      # present and empty: key 0
    wanted = check_spans(device, [(offset, size)], 1)
    assert wanted == [(FH.MISSING, offset + k, -1) for k in range(700)]
    none, only, one = where["no-dl"], where["only-dl"], where["one-nl"]
    for field in (0, 1, 7, 1023):
        check_spans(device, [none, (none[0], none[1] + 1), only, (only[0], only[1] + 1), (only[0] + 700, only[1] - 699), one,
                             (one[0] + 301, one[1] - 301)], field)
    # a line of 2 100 tabs has 2 101 empty fields; without its newline the span closes nothing and knows both ends
    assert check_spans(device, [(only[0], only[1] + 1)], 1023) == [(0, only[0] + 1023, 0)]
    summaries = device["dec"].field_hashes([only, none], 1023)[0]
    assert len(summaries[0]["head_hashes"]) == 1024 and summaries[0]["tail_start_hash"] == summaries[0]["tail_end_hash"]
    assert summaries[0]["head_hashes"][:2] == [0, TAB + 1] and summaries[0]["tail_start_hash"] == LH.part(b"\t" * 1023, LH.base(0))[0]
    assert summaries[1]["head_hashes"] == [] and summaries[1]["tail_start_hash"] is None
    assert check_spans(device, [(none[0], none[1] + 1)], 0)[0][0] == LH.line_hash(device["text"][none[0]:none[0] + none[1]])
    assert check_spans(device, [(none[0], none[1] + 1)], 1) == [(FH.MISSING, none[0] + none[1], -1)]


@pytest.mark.parametrize("length", [70_000, 200_000])
def test_lines_longer_than_a_tile(device, length):
    text, where = device["text"], device["where"]
    for kind in ("inside", "straddling", "missing"):
        offset, size = where["line-%d-%s" % (length, kind)]
        for field in (0, 1, 7):
            # the line whole, closed by its newline; entered in its middle; and as the head of a span that goes on
            wanted = check_spans(device, [(offset, size + 1), (offset + 12_345, size + 1 - 12_345), (offset - 1, size + 300)], field)
            parts = text[offset:offset + size].split(b"\t")
            assert wanted[0][0] == (LH.line_hash(parts[field]) if field < len(parts) else FH.MISSING), (kind, field)
    offset, size = where["line-%d-straddling" % length]
    assert check_spans(device, [(offset, size + 1)], 1)[0][1:] == (offset + 65_001, 999)         # across the tile edge at 65 536
    assert check_spans(device, [(offset, size + 1)], 1, seed=0xDEADBEEF)[0][0] == LH.line_hash(text[offset + 65_001:offset + 66_000], 0xDEADBEEF)
    offset, size = where["line-%d-inside" % length]
    assert check_spans(device, [(offset, size + 1)], 1)[0][1:] == (offset + 101, 99)
    # many spans in one call, each its own workgroup of the links
    check_spans(device, [(offset + 7 * k, 1 + k % 3) for k in range(600)], 0)
    check_spans(device, [(offset + 95 + k, 10) for k in range(120)], 1)


def test_capacity_smaller_than_the_count(device):
    offset, _ = device["where"]["lines"]
    spans = [(offset + 3, 70_000), (offset + 70_003, 5_000)]
    total = len(check_spans(device, spans))
    assert total > 1000
    for capacity in (0, 1, 255, 256, total - 1, total):
        check_spans(device, spans, capacity=capacity, room=total + 64)
    check_spans(device, spans, 0, capacity=257, room=total + 64)
    # nothing is asked for: no span; spans outside the output and arguments out of range are refused
    assert device["dec"].field_hashes([], 1)[0] == []
    with pytest.raises(Exception):
        device["dec"].field_hashes([(len(device["text"]) - 5, 6)], 1)
    for field, delimiter, newline, seed in ((1024, b"\t", b"\n", 0), (-1, b"\t", b"\n", 0), (0, b"\n", b"\n", 0), (0, b"", b"\n", 0),
                                            (0, b"\t", b"ab", 0), (0, b"\t", b"\n", -1), (0, b"\t", b"\n", 2**64)):
        with pytest.raises(ValueError):
            device["dec"].field_hashes([(0, 10)], field, delimiter, newline, seed)


def test_a_span_of_more_than_256_tiles(native):
    """Just over 16 MiB in one span are more tiles than one step of the links scans, and the long line crosses the step:
    its field 3 starts in the first step and ends in the second.  Runs of one byte, so that the file is small and the
    model hashes them in closed form."""
    rng = random.Random(7)
    front = b"".join(bytes(rng.choice(b"ab\t") for _ in range(rng.randrange(30))) + b"\n" for _ in range(60))
    text = front + b"x\ty\t" + b"a" * 9_000_000 + b"\t" + b"b" * 8_000_000 + b"\tc\n" + front + b"no newline\tat the end"
    assert len(text) > 257 * 65_536
    dec = TF.decoded(native, text)
    try:
        device = {"dec": dec, "text": text, "models": {}, "texts": {}}
        x, long_at = LH.base(0), len(front)
        lines = {}
        for field in (0, 2, 3, 5):
            wanted = check_spans(device, [(0, len(text))], field, prefixes=False)
            assert wanted[60][1] >= long_at and len(wanted) == 121
            lines[field] = wanted[60]
        assert lines[3] == (FH.run_part(ord("b"), 8_000_000, x)[0], long_at + 4 + 9_000_001, 8_000_000)
        assert lines[2][0] == FH.run_part(ord("a"), 9_000_000, x)[0] and lines[5][0] == FH.MISSING
        # the line entered behind its second tab, in a span that starts off the 16-byte grid
        check_spans(device, [(long_at + 5, len(text) - long_at - 5), (3, 17_000_000)], 1, prefixes=False)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ the reader

WANTED = ((0, TAB, 0), (1, TAB, 0), (3, TAB, 0), (7, TAB, 0), (1023, TAB, 0), (1, ord(","), 0), (1, TAB, 0xDEADBEEF))


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("fieldhash")
    files = {}
    for name, raw in (("tail", TF.reader_text(True)), ("closed", TF.reader_text(False))):
        path = folder / (name + ".bz2")
        path.write_bytes(datagen.compress(raw, 1))
        # computed once, shared, left unchanged
        wanted = {(j, dl, seed): FH.keys_of(raw, NL, dl, j, seed) for j, dl, seed in WANTED}
        files[name] = {"raw": raw, "path": str(path), "wanted": wanted}
    with native.open(files["tail"]["path"], parallelization=0) as f:
        blocks = f.block_offsets()
    assert len(blocks) >= 6                                     # several launch seams, and the long line crosses two
    return {"files": files, "folder": folder, "blocks": sorted(blocks.values())}


def keys(got):
    assert got.dtype == np.uint64 and got.ndim == 1
    return got.tolist()


@pytest.mark.parametrize("parallelization", [1, 2, 0])
@pytest.mark.parametrize("name", ["tail", "closed"])
def test_reader_whole_file_and_windows(native, corpus, name, parallelization):
    entry = corpus["files"][name]
    raw, wanted = entry["raw"], entry["wanted"]
    n = len(F.lines_of(raw, NL))
    with native.open(entry["path"], parallelization=parallelization) as f:
        for (j, dl, seed), want in wanted.items():
            assert keys(f.field_hashes(j, delimiter=bytes([dl]), seed=seed)) == want, (j, dl, seed)
        assert native.FIELD_MISSING in wanted[(3, TAB, 0)] and 0 in wanted[(3, TAB, 0)]
        # the long line's field 1 crosses two block seams: it is the CPU's hash of those 89 994 bytes
        contents = F.lines_of(raw, NL)
        long_line = max(range(n), key=lambda k: len(contents[k]))
        field = contents[long_line].split(b"\t")[1]
        assert len(field) == 89_994 and wanted[(1, TAB, 0)][long_line] == native.line_hash(field)
        # windows: inside one block, across blocks, around block seams, at and past the end, and empty ones
        starts = f.line_starts(range(n)).tolist()
        seam_lines = [max(k for k in range(n) if starts[k] <= b) for b in corpus["blocks"][1:-1]]
        windows = [(0, 1), (0, 3), (5, 7), (seam_lines[0], 1), (seam_lines[0] - 1, 3), (seam_lines[1] + 1, 1),
                   (seam_lines[0], seam_lines[3] - seam_lines[0] + 2), (n - 1, 1), (n - 1, 5), (n - 3, 3), (n - 2, 10**12),
                   (n, 1), (n + 5, 2), (7, 0), (0, 0), (1, None), (n // 2, None)]
        want = wanted[(3, TAB, 0)]
        for first, count in windows:
            end = n if count is None else first + count
            assert keys(f.field_hashes(3, first, count)) == want[first:end], (first, count)
        assert keys(f.field_hashes(1, seam_lines[1], 4, delimiter=b",")) == wanted[(1, ord(","), 0)][seam_lines[1]:seam_lines[1] + 4]
        assert f.tell() == 0                                        # positionless
    with native.IndexedBzip2File(entry["path"], parallelization=parallelization) as f:
        assert keys(f.field_hashes(1, 3, 2)) == wanted[(1, TAB, 0)][3:5]
        assert keys(f.field_hashes(1, 3, 2, seed=0xDEADBEEF)) == wanted[(1, TAB, 0xDEADBEEF)][3:5]


def counted(raw, j, dl=TAB, first=0, count=None):
    """(lines, counts, missing, value_counts) of the model: collections.Counter over bytes.split's fields."""
    fields = F.fields_of(raw, NL, dl, j)
    fields = fields[first:] if count is None else fields[first:first + count]
    counter = collections.Counter(field for field in fields if field is not None)
    first_line = {}
    for k, field in enumerate(fields):
        if field is not None:
            first_line.setdefault(field, first + k)
    values = sorted(counter, key=lambda value: first_line[value])
    ranked = sorted(values, key=lambda value: (-counter[value], first_line[value]))
    return ([first_line[v] for v in values], [counter[v] for v in values], sum(1 for field in fields if field is None),
            [(v, counter[v]) for v in ranked])


def test_small_files(native, corpus):
    folder = corpus["folder"]
    cases = [("small-empty.bz2", b""), ("small-newline.bz2", b"\n"), ("small-closed.bz2", b"a\tb\n\n"),
             ("small-tail.bz2", b"a\tb\nc\td\te\nf\t"), ("small-tabs.bz2", b"\t\t\n\t"), ("small-nul.bz2", b"\0\t\0\n\0\0\n\0"),
             ("small-same.bz2", b"k\tv\nk\tv\nq\nk\tw\n\nk\tv")]
    for name, raw in cases:
        with native.open(TF.small_file(folder, name, raw), parallelization=1) as f:
            for j in (0, 1, 2, 3):
                assert keys(f.field_hashes(j)) == FH.keys_of(raw, NL, TAB, j), (name, j)
                assert keys(f.field_hashes(j, 1)) == FH.keys_of(raw, NL, TAB, j)[1:], (name, j)
                lines, counts, missing, ranked = counted(raw, j)
                got = f.count_by_field(j)
                assert (got[0].tolist(), got[1].tolist(), got[2]) == (lines, counts, missing), (name, j)
                assert got[0].dtype == got[1].dtype == np.uint64
                assert f.value_counts(j) == ranked, (name, j)
            assert keys(f.field_hashes(0, newline=b"\0", delimiter=b"\n")) == FH.keys_of(raw, 0, NL, 0), name
    assert FH.keys_of(b"f\t", NL, TAB, 1) == [0] and FH.keys_of(b"a\tb\n\n", NL, TAB, 1) == [LH.line_hash(b"b"), FH.MISSING]


def test_interleaved_with_other_calls(native, corpus):
    entry = corpus["files"]["tail"]
    raw, wanted = entry["raw"], entry["wanted"]
    with native.open(entry["path"], parallelization=0) as f:
        head = f.read(1000)
        assert head == raw[:1000] and f.tell() == 1000
        hashes = f.line_hashes(0, 500)
        numbers, lines = f.grep(b"abc", limit=20)
        spans = f.field_spans(1, 10, 300)
        assert keys(f.field_hashes(1, 10, 300)) == wanted[(1, TAB, 0)][10:310]
        assert f.tell() == 1000
        assert f.line_hashes(0, 500).tolist() == hashes.tolist()
        again = f.grep(b"abc", limit=20)
        assert again[0].tolist() == numbers.tolist() and again[1] == lines
        assert [a.tolist() for a in f.field_spans(1, 10, 300)] == [a.tolist() for a in spans]
        assert spans[0].tolist() == [s for s, _ in F.direct(raw, NL, TAB, 1)[10:310]]
        lines_, counts, missing = f.count_by_field(0, 100, 50)
        assert (lines_.tolist(), counts.tolist(), missing) == counted(raw, 0, TAB, 100, 50)[:3]
        assert f.read(500) == raw[1000:1500] and f.tell() == 1500
        assert keys(f.field_hashes(7)) == wanted[(7, TAB, 0)]
        assert f.read_fields(0, 100, 50) == F.fields_of(raw, NL, TAB, 0)[100:150]
        assert f.read(100) == raw[1500:1600]
        # a whole line as its field 0 under a delimiter that does not occur: the line hash
        assert 1 not in raw[:2000]
        assert keys(f.field_hashes(0, 0, 5, delimiter=b"\x01")) == f.line_hashes(0, 5).tolist()


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import numpy as np
import indexed_bzip2_amd as m

with m.open(sys.argv[2], parallelization=int(sys.argv[3])) as f:
    for field, first, count, delimiter, seed in ((0, 0, None, b"\t", 0), (1, 0, None, b"\t", 5), (3, 100, 2000, b"\t", 0),
                                                 (1, 0, None, b",", 0), (1023, 0, None, b"\t", 0), (2, 10**9, 5, b"\t", 0),
                                                 (2, 3, 0, b"\t", 0)):
        host = f.field_hashes(field, first, count, delimiter, seed=seed)
        tensor = f.field_hashes_to_tensor(field, first, count, delimiter, seed=seed)
        assert tensor.dtype == torch.int64 and tensor.is_cuda and tensor.dim() == 1
        assert tensor.cpu().numpy().tolist() == host.tolist(), (field, first, count)
        assert int(tensor.min()) >= 0 if len(host) else True
        print(field, first, count, len(host))
    # join keys: the lines whose field 1 is one of two values, by torch.isin
    wanted = torch.tensor([m.line_hash(b"abc"), m.FIELD_MISSING], dtype=torch.int64, device=tensor.device)
    keys = f.field_hashes_to_tensor(1)
    hits = torch.isin(keys, wanted).cpu().numpy()
    host = f.field_hashes(1)
    assert hits.tolist() == [int(k) in (m.line_hash(b"abc"), m.FIELD_MISSING) for k in host] and hits.any()
    assert f.tell() == 0
print("field hash tensors ok")
"""


@pytest.mark.parametrize("parallelization", [1, 0])
def test_tensor_forms_equal_the_host_forms(native, corpus, parallelization):
    """In a process of its own that imports torch first; the host forms are pinned to the model above."""
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, corpus["files"]["tail"]["path"], str(parallelization)],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "field hash tensors ok" in run.stdout and "0 0 None 0" not in run.stdout


# ------------------------------------------------------------------------------------------------ grouping

def grouping_text():
    """About 600 kB of records "<number>\t<user>\t<status>[\t<word>]": a few hundred distinct users with heavy repeats,
    among them the empty one; every eleventh line has one field only, so fields 1, 2 and 3 are missing there."""
    rng = random.Random(0xC0FFEE)
    users = [b""] + [b"user%d" % rng.randrange(10**6) for _ in range(299)]
    weights = [1000 // (k + 1) + 1 for k in range(len(users))]
    out = bytearray()
    for k in range(20_000):
        if k % 11 == 10:
            out += b"%d\n" % k
            continue
        user = rng.choices(users, weights)[0]
        fields = [b"%d" % k, user, rng.choice([b"200", b"200", b"200", b"404", b"500", b"301"])]
        if rng.randrange(3) == 0:
            fields.append(rng.choice([b"alpha", b"beta", b""]))
        out += b"\t".join(fields) + b"\n"
    return bytes(out) + b"20000\tuser-at-the-end\t200"


@pytest.fixture(scope="module")
def grouped(native, tmp_path_factory):
    raw = grouping_text()
    path = tmp_path_factory.mktemp("fieldgroups") / "groups.bz2"
    path.write_bytes(datagen.compress(raw, 1))
    return {"raw": raw, "path": str(path)}


@pytest.mark.parametrize("parallelization", [1, 0])
def test_count_by_field_and_value_counts(native, grouped, parallelization):
    raw = grouped["raw"]
    n = len(F.lines_of(raw, NL))
    assert n == 20_001
    for j, seed in ((1, 0), (2, 0), (3, 0), (0, 0), (1, 0xDEADBEEF)):
        # a condition on the input, checked on the CPU: the model's keys are collision-free for this corpus
        fields = F.fields_of(raw, NL, TAB, j)
        values = {field for field in fields if field is not None}
        assert len({FH.key_of(value, seed) for value in values}) == len(values) and FH.MISSING not in {FH.key_of(v, seed) for v in values}
    fields = F.fields_of(raw, NL, TAB, 1)
    assert 200 < len({f_ for f_ in fields if f_ is not None}) <= 301 and b"" in fields and None in fields
    with native.open(grouped["path"], parallelization=parallelization) as f:
        assert len(f.block_offsets()) >= 5
        position = f.tell()                                         # completing the block map may have read ahead
        for j, first, count, seed in ((1, 0, None, 0), (2, 0, None, 0), (3, 0, None, 0), (0, 0, None, 0), (1, 0, None, 0xDEADBEEF),
                                      (1, 5000, 7000, 0), (1, n - 3, 10, 0), (1, n, 5, 0), (2, 10, 1, 0), (5, 0, None, 0)):
            lines, counts, missing, ranked = counted(raw, j, TAB, first, count)
            got = f.count_by_field(j, first, count, seed=seed)
            assert got[0].dtype == got[1].dtype == np.uint64 and isinstance(got[2], int)
            assert (got[0].tolist(), got[1].tolist(), got[2]) == (lines, counts, missing), (j, first, count)
            in_range = max(0, min(n, n if count is None else first + count) - first)
            assert int(got[1].sum()) + got[2] == in_range
            assert f.value_counts(j, first=first, count=count, seed=seed) == ranked, (j, first, count)
            for limit in (0, 1, 20, 10**6):
                assert f.value_counts(j, limit, first, count, seed=seed) == ranked[:limit], (j, limit)
        top = f.value_counts(1, limit=3)
        assert top[0][0] == b"" and top[0][1] > top[1][1] >= top[2][1]
        assert f.tell() == position                                 # positionless
        # the calls around it stay intact
        assert f.line_hashes(0, 3).tolist() == LH.direct(raw, NL)[:3]
    with native.IndexedBzip2File(grouped["path"], parallelization=parallelization) as f:
        lines, counts, missing, ranked = counted(raw, 2)
        got = f.count_by_field(2)
        assert (got[0].tolist(), got[1].tolist(), got[2]) == (lines, counts, missing)
        assert f.value_counts(2, 2) == ranked[:2] == [(b"200", ranked[0][1]), ranked[1]]


def test_tool(native, grouped, corpus):
    raw = grouped["raw"]
    for options, j, dl in ((["--count-by-field", "1"], 1, TAB), (["--count-by-field=2", "-P", "1"], 2, TAB),
                           (["--count-by-field", "3", "--seed", "99"], 3, TAB),
                           (["--count-by-field", "1", "--field-delimiter", "0"], 1, ord("0")),
                           (["--count-by-field", "0", "--field-delimiter=\\x09"], 0, TAB), (["--count-by-field", "9"], 9, TAB)):
        run = subprocess.run([CLI] + options + [grouped["path"]], capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr
        assert run.stdout == b"".join(b"%d\t%s\n" % (count, value) for value, count in counted(raw, j, dl)[3]), options
    entry = corpus["files"]["tail"]
    values = {field for field in F.fields_of(entry["raw"], NL, TAB, 1) if field is not None}
    assert len({FH.key_of(value) for value in values}) == len(values)          # collision-free: a condition on the input
    run = subprocess.run([CLI, "--count-by-field", "1", entry["path"]], capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert run.stdout == b"".join(b"%d\t%s\n" % (count, value) for value, count in counted(entry["raw"], 1)[3])
