"""grep_regex on the GPU: the kernels under Decoder.match_lines (k_regex_chunks, k_regex_link, k_regex_emit), the
reader's grep_regex / count_matching_lines_regex / grep_regex_to_tensor, and `ibzip2-mi355x --grep-regex`.

Device level: one decoded block of generated text; the summaries and witnesses of every span must equal those of the model
in regexgen.py (the compiled table run chunk by chunk in Python) exactly.  Reader level: which lines match is Python's
re.search(pattern, content, re.DOTALL [| re.IGNORECASE]), line by line -- never the code under test."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import datagen
import grepgen
import regexgen as G

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
NL = 10


# ------------------------------------------------------------------------------------------------ the kernels

def device_text(C):
    """(text, {name: (offset, size)}): regions built around the chunk size C, each behind a stretch of seeded lines."""
    rng = random.Random(0xA11CE)
    parts, at, where = [], 0, {}

    def add(piece, name=None):
        nonlocal at
        if name is not None:
            where[name] = (at, len(piece))
        parts.append(piece)
        at += len(piece)

    def filler(n):
        out = bytearray()
        while len(out) < n:
            out += bytes(rng.choice(b"aab,xyz ") for _ in range(rng.choice([0, 1, 3, 8, 20, 60]))) + b"\n"
        return bytes(out[:n - 1]) + b"\n"

    add(filler(20 * C + 7), "lines")
    add(b"ab" * (3 * C // 2), "no-delimiter")                       # 3C bytes, none of them the delimiter
    add(b"\n")
    add(b"\n" + b"xa" * C, "delimiter-first")                       # the only delimiter is the first byte
    add(b"ya" * C + b"\n", "delimiter-last")                        # ... is the last byte
    add(filler(5))
    # relative to the region's start: a delimiter on a chunk's first byte (C) and one on a chunk's last byte (3C - 1)
    edge = bytearray(b"a" * (4 * C))
    edge[C] = edge[3 * C - 1] = NL
    add(bytes(edge) + b"\n", "chunk-edges")
    # an empty line that starts on a chunk's first byte: delimiters at C - 1 and C
    empty = bytearray(b"x,y" * C)[:3 * C]
    empty[C - 1] = empty[C] = NL
    add(bytes(empty) + b"\n", "empty-line")
    # one line of 5C + 3 bytes whose match completes in its last chunk: x, y and z in three different chunks
    line = bytearray(b"q" * (5 * C + 3))
    line[3], line[2 * C + 1], line[5 * C + 1] = ord("x"), ord("y"), ord("z")
    add(b"a\n" + bytes(line) + b"\naaa\n", "long-line")
    # delimiter-free stretches of more chunks than one step of k_regex_link takes (256), each a line that matches only
    # through the state carried from its first chunk: ^a+$, and x.*y.*z with the three letters far apart
    steps = 300 * C + 5
    far = bytearray(b"a" * steps)
    far[C + 2], far[150 * C], far[299 * C + 9] = ord("x"), ord("y"), ord("z")
    add(b"b\n" + b"a" * steps + b"\n" + bytes(far) + b"\n" + b"a" * steps + b"b\nzz\n", "carried")
    add(filler(3 * C))
    return b"".join(parts), where


@pytest.fixture(scope="module")
def device(native):
    C = native._native.regex_chunk_bytes()
    text, where = device_text(C)
    enc = datagen.compress(text, 9)
    dec = native.Decoder(device=0)
    dec.set_input(enc)
    offsets = native.find_magic(enc)
    results, total = dec.decode_batch(offsets)
    assert len(offsets) == 1 and total == len(text) and dec.copy_output(0, total) == text
    yield {"dec": dec, "text": text, "where": where, "C": C}
    dec.close()


def check_spans(native, device, pattern, spans, ignore_case=False, nl=b"\n"):
    compiled = native.compile_regex(pattern, ignore_case)
    transitions, accepts = compiled.transitions.tolist(), compiled.accepts_at_end.tolist()
    text, C = device["text"], device["C"]
    models = [G.summarise(transitions, accepts, text[o:o + n], nl[0], C, o) for o, n in spans]
    head_maps, has_delimiter, exits, positions, counts = device["dec"].match_lines(spans, compiled, nl)
    for i, model in enumerate(models):
        assert head_maps[i].tolist() == model.padded_head_map(), (pattern, spans[i])
        assert has_delimiter[i] == model.has_delimiter and exits[i] == model.exit, (pattern, spans[i])
        assert counts[i] == len(model.witnesses), (pattern, spans[i])
    wanted = [p for model in models for p in model.witnesses]
    assert positions == wanted, pattern
    return models, wanted


def test_span_sizes_and_starts(native, device):
    C = device["C"]
    base = device["where"]["lines"][0]
    spans = [(base + start, size) for start in (1, 7, 21, C + 3) for size in (1, C - 1, C, C + 1, 2 * C + 1)]
    spans += [(base + 13, 0), (base + 5, 19 * C + 2)]
    assert all(o % 16 != 0 for o, _ in spans)
    for pattern in (rb"ab", rb"a*", rb"^$", rb"(^|,)x(,|$)", rb"[^a]$", rb"^a+$", rb"x.*y.*z"):
        check_spans(native, device, pattern, spans)
    check_spans(native, device, rb"AB|Z$", spans, ignore_case=True)
    # another delimiter: ',' ends the lines and "\n" is a byte like any other
    check_spans(native, device, rb"^x", spans, nl=b",")
    # the whole block as one span, and the same span twice
    whole = (0, len(device["text"]))
    check_spans(native, device, rb"(^|,)x(,|$)", [whole, spans[3], whole])


def test_spans_without_and_with_one_delimiter(native, device):
    where = device["where"]
    spans = [where["no-delimiter"], where["delimiter-first"], where["delimiter-last"]]
    for pattern in (rb"ab", rb"^(ab)+$", rb"xa", rb"^(ya)+$", rb"a*", rb"b$"):
        models, _ = check_spans(native, device, pattern, spans)
        assert [m.has_delimiter for m in models] == [False, True, True]
    # the head of a span without a delimiter is all of it: every entry state is carried through 3C bytes
    models, _ = check_spans(native, device, rb"^(ab)+$", [where["no-delimiter"]])
    assert models[0].head_map[0] not in (0, 1) and models[0].witnesses == []


def test_delimiters_on_chunk_edges(native, device):
    C, where = device["C"], device["where"]
    offset, size = where["chunk-edges"]
    assert device["text"][offset + C] == NL and device["text"][offset + 3 * C - 1] == NL
    for pattern in (rb"^a+$", rb"a$", rb"^a", rb"a*"):
        models, wanted = check_spans(native, device, pattern, [(offset, size), (offset + 1, size - 1)])
        assert len(wanted) >= 2
    offset, size = where["empty-line"]
    assert device["text"][offset + C - 1:offset + C + 1] == b"\n\n"
    for pattern in (rb"^$", rb"^.$", rb"y$", rb"^x"):
        models, wanted = check_spans(native, device, pattern, [(offset, size)])
    models, wanted = check_spans(native, device, rb"^$", [(offset, size)])
    assert wanted == [offset + C]                          # the empty line is its own delimiter, a chunk's first byte


def test_long_line_completes_in_its_last_chunk(native, device):
    C = device["C"]
    offset, size = device["where"]["long-line"]
    models, wanted = check_spans(native, device, rb"x.*y.*z", [(offset, size)])
    line = offset + 2
    assert wanted == [offset + 5 * C]                      # the head hit of the line's last chunk: that chunk's first byte
    models, wanted = check_spans(native, device, rb"^q+xq+yq+zq$", [(offset, size)])
    assert len(wanted) == 1
    # the same line as the span's head line: no witness, the head map carries it
    models, wanted = check_spans(native, device, rb"x.*y.*z", [(line, 5 * C + 4)])
    assert wanted == [] and models[0].head_map[0] == G.MATCHED


def test_state_carried_over_more_chunks_than_a_link_step(native, device):
    C = device["C"]
    offset, size = device["where"]["carried"]
    assert size > 3 * 256 * C
    text = device["text"][offset:offset + size]
    for pattern in (rb"^a+$", rb"x.*y.*z"):
        models, wanted = check_spans(native, device, pattern, [(offset, size), (offset + 3, size - 3)])
        lines = G.lines_of_offsets(text, [p - offset for p in models[0].witnesses])
        assert lines == G.expected_lines(pattern, text) and len(lines) == 1
    # entered in the middle of the first long line: its rest is the span's head, carried over 200 chunks
    models, wanted = check_spans(native, device, rb"^a+$", [(offset + 2 + 100 * C, size - 2 - 100 * C)])
    assert models[0].has_delimiter and models[0].head_map[0] != G.MATCHED


def test_capacity_smaller_than_the_count(native, device):
    dec = device["dec"]
    spans = [device["where"]["lines"], device["where"]["chunk-edges"]]
    compiled = native.compile_regex(rb"a")
    _, _, _, everything, counts = dec.match_lines(spans, compiled)
    assert sum(counts) == len(everything) > 40
    for capacity in (1, 7, len(everything) - 1, len(everything), len(everything) + 5):
        _, _, _, positions, again = dec.match_lines(spans, compiled, capacity=capacity)
        assert positions == everything[:capacity] and again == counts
    # nothing is written at or beyond the capacity
    import ctypes
    N = native._native
    room = (ctypes.c_uint64 * 16)(*([0xDEADBEEF] * 16))
    arr = (N.ByteSpan * 2)(*[N.ByteSpan(o, n) for o, n in spans])
    head_maps = (ctypes.c_uint8 * 128)()
    flags, exits, out = (ctypes.c_uint8 * 2)(), (ctypes.c_uint8 * 2)(), (ctypes.c_uint64 * 2)()
    assert N.lib().mi355x_bz2_match_lines(dec._h, arr, 2, compiled._h, NL, head_maps, flags, exits, room, 9, out) == 0
    assert list(room[:9]) == everything[:9] and list(room[9:]) == [0xDEADBEEF] * 7
    # a count-only call, and the argument checks
    assert N.lib().mi355x_bz2_match_lines(dec._h, arr, 2, compiled._h, NL, head_maps, flags, exits, None, 0, out) == 0
    assert list(out) == counts
    outside = (N.ByteSpan * 1)(N.ByteSpan(len(device["text"]) - 3, 4))
    assert N.lib().mi355x_bz2_match_lines(dec._h, outside, 1, compiled._h, NL, head_maps, flags, exits, None, 0, out) == 103
    assert N.lib().mi355x_bz2_match_lines(dec._h, arr, 2, None, NL, head_maps, flags, exits, None, 0, out) == 103


# ------------------------------------------------------------------------------------------------ the reader

READER_PATTERNS = [
    rb"error",
    rb"(error|warning|fatal)",
    rb"^$",
    rb"\.$",
    rb"^.$",
    rb"^\s*$",
    rb"\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}",
    rb"^(GET|POST) /[a-z/]* HTTP/1\.[01]$",
    rb"^[0-9]{4}-[0-9]{2}-[0-9]{2} .*(ERROR|FATAL)",
    rb"x.*y.*z",
    rb"(^|,)x(,|$)",
    rb"[Qq]u[aeiou]+",
]


def reader_text():
    """About 400 kB of grepgen's lines, some of them replaced by lines that the patterns are about."""
    text = grepgen.make_text()[:400_000]
    lines = text.split(b"\n")
    rng = random.Random(0xBEEF)
    crafted = [b"error", b"an ERROR here", b"Warning: disk", b"fatal", b"", b" \t ", b".", b"ends.", b"10.0.0.255 up", b"1.2.3",
               b"GET /a/b HTTP/1.1", b"POST / HTTP/1.0", b"get / HTTP/1.1", b"2024-01-02 boot ERROR", b"2024-01-02 boot error",
               b"2024-1-02 FATAL", b"x", b"a,x", b"x,b", b"quae", b"QUI", b"xyz"]
    for k in rng.sample(range(1, len(lines) - 1), 6 * len(crafted)):
        lines[k] = crafted[k % len(crafted)]
    lines[0] = b"2024-12-31 first line FATAL"
    lines[-1] = b"the tail ends with error"
    return b"\n".join(lines)


def reference(raw, pattern, ignore_case=False, nl=b"\n", limit=None):
    compiled = re.compile(pattern, G.reference_flags(ignore_case))
    numbers, lines = [], []
    for k, (at, content) in enumerate(G.split_lines(raw, nl)):
        if compiled.search(content):
            numbers.append(k)
            lines.append(raw[at:at + len(content) + 1])
    if limit is not None:
        numbers, lines = numbers[:limit], lines[:limit]
    return numbers, lines


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    folder = tmp_path_factory.mktemp("regex")
    raw = reader_text()
    assert 350_000 < len(raw) < 450_000 and not raw.endswith(b"\n")
    path = folder / "text.bz2"
    path.write_bytes(datagen.compress(raw, 1))
    with native.open(str(path), parallelization=0) as f:
        blocks = f.block_offsets()
    assert len(blocks) >= 4                                     # blocks of about 100 kB: several launch seams
    return {"raw": raw, "path": str(path), "folder": folder}


@pytest.mark.parametrize("parallelization", [1, 0])
def test_reader_against_re(native, corpus, parallelization):
    raw = corpus["raw"]
    with native.open(corpus["path"], parallelization=parallelization) as f:
        for pattern in READER_PATTERNS:
            for ignore_case in (False, True):
                numbers, lines = reference(raw, pattern, ignore_case)
                got_numbers, got_lines = f.grep_regex(pattern, ignore_case=ignore_case)
                assert got_numbers.dtype == np.uint64 and got_numbers.tolist() == numbers, (pattern, ignore_case)
                assert got_lines == lines, (pattern, ignore_case)
                assert f.count_matching_lines_regex(pattern, ignore_case=ignore_case) == len(numbers)
        assert len(reference(raw, rb"error")[0]) > 5
        # a fixed string is a regular expression
        numbers, lines = f.grep_regex(b"error")
        plain_numbers, plain_lines = f.grep(b"error")
        assert numbers.tolist() == plain_numbers.tolist() and lines == plain_lines
        # limits
        total = len(numbers)
        for limit in (1, total - 1):
            got_numbers, got_lines = f.grep_regex(b"error", limit=limit)
            assert got_numbers.tolist() == numbers.tolist()[:limit] and got_lines == lines[:limit]
        # a compiled regex, and the IndexedBzip2File spelling
        compiled = native.compile_regex(rb"^$")
        assert f.grep_regex(compiled)[0].tolist() == reference(raw, rb"^$")[0]
        assert f.tell() == 0                                        # positionless
    with native.IndexedBzip2File(corpus["path"], parallelization=parallelization) as f:
        assert f.count_matching_lines_regex(rb"\.$") == len(reference(raw, rb"\.$")[0])


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import numpy as np
import indexed_bzip2_amd as m

with m.open(sys.argv[2], parallelization=1) as f:
    for pattern, limit in ((rb"(error|warning|fatal)", None), (rb"^$", 3), (rb"never-there", None), (rb"error", 0)):
        numbers, lines = f.grep_regex(pattern, limit=limit, ignore_case=True)
        got_numbers, data, offsets = f.grep_regex_to_tensor(pattern, limit=limit, ignore_case=True)
        assert got_numbers.dtype == np.uint64 and got_numbers.tolist() == numbers.tolist(), pattern
        assert data.dtype == torch.uint8 and data.is_cuda and data.dim() == 1
        assert bytes(data.cpu().numpy()) == b"".join(lines), pattern
        bounds = [0]
        for line in lines:
            bounds.append(bounds[-1] + len(line))
        assert offsets.tolist() == bounds, pattern
        print(pattern, len(lines))
    assert f.tell() == 0
print("regex tensor ok")
"""


def test_grep_regex_to_tensor(native, corpus):
    """In a process of its own that imports torch first; grep_regex itself is pinned to re above."""
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, corpus["path"]], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "regex tensor ok" in run.stdout and "b'(error|warning|fatal)' 0" not in run.stdout


def test_other_delimiters(native, corpus):
    raw = corpus["raw"]
    with native.open(corpus["path"], parallelization=1) as f:
        # with ' ' as the delimiter "\n" is a byte like any other; no $ here: Python's also matches in front of a final "\n"
        for pattern in (rb"^err", rb"[0-9]{3}", rb"^\n", rb"e\n\n?x"):
            numbers, lines = reference(raw, pattern, nl=b" ")
            got_numbers, got_lines = f.grep_regex(pattern, newline=b" ")
            assert got_numbers.tolist() == numbers and got_lines == lines, pattern
            assert f.count_matching_lines_regex(pattern, newline=b" ") == len(numbers)
        # no NUL anywhere: the whole file is one line
        numbers, lines = f.grep_regex(rb"FATAL", newline=b"\0")
        assert numbers.tolist() == [0] and lines == [raw]


def small_file(native, folder, name, raw, level=9):
    path = folder / name
    path.write_bytes(datagen.compress(raw, level))
    return str(path)


def test_tails_empty_files_and_one_long_line(native, corpus):
    folder = corpus["folder"]
    # a tail without a final delimiter that matches only by $
    raw = b"beta\nalpha beta\nalpha"
    with native.open(small_file(native, folder, "tail.bz2", raw), parallelization=1) as f:
        assert f.grep_regex(rb"alpha$")[0].tolist() == [2] and f.grep_regex(rb"alpha$")[1] == [b"alpha"]
        assert f.count_matching_lines_regex(rb"alpha$") == 1
        assert f.grep_regex(rb"^$")[0].tolist() == [] and f.count_matching_lines_regex(rb"a*") == 3
    # a file that ends in the delimiter has no further line, whatever the pattern matches
    with native.open(small_file(native, folder, "closed.bz2", b"beta\n\n"), parallelization=1) as f:
        assert f.grep_regex(rb"^$")[0].tolist() == [1] and f.count_matching_lines_regex(rb"a*") == 2
    with native.open(small_file(native, folder, "empty.bz2", b""), parallelization=1) as f:
        assert f.count_matching_lines_regex(rb"a*") == 0 and f.grep_regex(rb"^$") [1] == []
    with native.open(small_file(native, folder, "newline.bz2", b"\n"), parallelization=1) as f:
        assert f.count_matching_lines_regex(rb"^$") == 1 and f.grep_regex(rb"^$")[1] == [b"\n"]
        assert f.count_matching_lines_regex(rb".") == 0
    # one line of 300 kB across several launches: x near its start, z near its end
    rng = random.Random(3)
    line = bytearray(rng.choice(b"abcdefgh ") for _ in range(300_000))
    line[10], line[150_000], line[299_990] = ord("x"), ord("y"), ord("z")
    raw = bytes(line)
    path = small_file(native, folder, "line.bz2", raw, level=1)
    for parallelization in (1, 0):
        with native.open(path, parallelization=parallelization) as f:
            assert len(f.block_offsets()) >= 4
            assert f.count_matching_lines_regex(rb"^[a-h ]*x.*y.*z[a-h ]*$") == 1
            assert f.grep_regex(rb"x.*y.*z")[1] == [raw]
            assert f.count_matching_lines_regex(rb"z.*x") == 0 and f.count_matching_lines_regex(rb"^x") == 0


def test_tool(native, corpus):
    raw = corpus["raw"]
    for pattern, options in ((rb"^[0-9]{4}-[0-9]{2}-[0-9]{2} .*(ERROR|FATAL)", []), (rb"(error|warning|fatal)", ["--line-number"]),
                             (rb"^get /", ["--ignore-case"]), (rb"\.$", ["--line-number", "--ignore-case"]),
                             (rb"never-there", ["--line-number"])):
        numbers, lines = reference(raw, pattern, "--ignore-case" in options)
        run = subprocess.run([CLI, "--grep-regex", pattern.decode()] + options + ["-P", "1", corpus["path"]],
                             capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr
        if "--line-number" in options:
            wanted = b"".join(b"%d:" % (k + 1) + line for k, line in zip(numbers, lines))
        else:
            wanted = b"".join(lines)
        assert run.stdout == wanted, pattern
