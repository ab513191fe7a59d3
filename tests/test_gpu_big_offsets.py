"""Offsets beyond 2^32 on the GPU: one batch with more than 2^32 bytes of output, the reader and its searches on a file
that decodes past 2^32 (bigfiles.far_file), and a file whose compressed bits pass 2^32 (bigfiles.deep_file).

Every expected value comes from tests/bigfiles.py: the decoded bytes as parts (VirtualRaw), the block map by arithmetic on
the stitching, the CRC of a concatenation in plain integers.  A block written to a truncated offset passes its own CRC
(k_rle and k_crc take the offset from one record) and fillers of one value look alike, so the content is checked where the
CRC cannot tell: every filler is counted, neighbouring fillers differ, and no filler above 2^32 has its own value 2^32 below.

The four line queries -- regular expressions, line hashes, field spans and field hashes -- meet the same offsets: their
kernels on spans of the batch around, across and above 2^32 and on the whole output as one span (A2), the reader's
stitching on far_file() with one line of 4.29 GB that runs through 94 launches (B), and, because no closed line of
far_file() reaches 2^32 bytes, the same blocks decoded in another order, where one field of one closed line does
(test_field_of_more_than_4_gib).

One module-scoped fixture per file does the decode; the tests ask what is resident.  No test copies more than a few MB to
the host.

Measured on an MI355X ("Offsets beyond 2^32"): the figures are printed by the fixtures."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import ROOT
import bigfiles

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")
CUT = 1 << 32
NEAR = CUT - (1 << 27)
NL = 10


@pytest.fixture(scope="module")
def far():
    return bigfiles.far_file()


@pytest.fixture(scope="module")
def deep():
    return bigfiles.deep_file()


def decode_all(native, far, flags=0):
    """A context made as the reader makes its own (scratch for one block, growing), the whole file in one batch."""
    dec = native.Decoder(device=0, max_batch_blocks=1, flags=flags)
    dec.set_input(far.enc)
    began = time.time()
    results, total = dec.decode_batch([bit for bit, _, _, _ in far.blocks])
    seconds = time.time() - began
    return dec, results, total, seconds


@pytest.fixture(scope="module")
def far_batch(native, far):
    dec, results, total, seconds = decode_all(native, far)
    print(f"\nfar batch: {len(results)} blocks, {total} bytes in {seconds:.2f} s; timings {dec.timings()}; "
          f"device memory {dec.device_memory()}")
    yield dec, results, total
    dec.close()


def check_records(far, results, total):
    assert total == far.raw.size > CUT
    assert [r["status"] for r in results] == [0] * len(far.blocks)
    assert all(r["computed_crc"] == r["header_crc"] for r in results)
    assert [r["encoded_offset_bits"] for r in results] == [bit for bit, _, _, _ in far.blocks]
    assert [r["data_offset"] for r in results] == [at for _, at, _, _ in far.blocks]          # the arithmetic prefix sum
    assert [r["decoded_size"] for r in results] == [size for _, _, size, _ in far.blocks]
    assert sum(1 for r in results if r["data_offset"] >= CUT) >= 2 + 10


def check_texts(far, dec):
    """All of T1 (around 2^32) and all of T2 (above it, T0's bytes), byte for byte, and T0."""
    assert dec.copy_output(far.t1_at, len(far.t1)) == far.t1
    assert dec.copy_output(far.t2_at, len(far.t0)) == far.t0
    assert dec.copy_output(0, len(far.t0)) == far.t0
    assert dec.copy_output(CUT - 70_000, 140_000) == far.raw.slice(CUT - 70_000, CUT + 70_000)


# ------------------------------------------------------------------------- A. one batch with more than 2^32 bytes of output

def test_magic_scan_far(native, far, far_batch):
    dec, _, _ = far_batch
    blocks = [bit for bit, _, _, _ in far.blocks]
    assert dec.find_magic() == blocks
    assert dec.find_magic(native._native.MAGIC_EOS) == far.eos
    assert native.find_magic(far.enc) == blocks
    assert native.find_magic(far.enc, native._native.MAGIC_EOS) == far.eos


def test_batch_records(far, far_batch):
    dec, results, total = far_batch
    check_records(far, results, total)
    # the buffer chosen before the sizes were known holds 900 000 bytes per block (a fresh context has no larger hint): the
    # batch took the branch of decode_batch_end that lays the blocks out on the host and expands once more
    assert total + 256 > len(results) * 900_000
    memory = dec.device_memory()
    assert total + 256 <= memory["output_bytes"] <= 2 * (total + total // 8) + (4 << 20)
    assert memory["scratch_bytes"] + memory["output_bytes"] < 32 << 30


def test_batch_content(far, far_batch):
    dec, results, total = far_batch
    fillers = [(at, size, value) for _, at, size, value in far.blocks if value is not None]
    assert len(fillers) >= 96
    # every filler holds its value and nothing else -- all of them: a block written 2^32 too low lands in one of the first
    for value in sorted({value for _, _, value in fillers}):
        spans = [(at, size) for at, size, v in fillers if v == value]
        assert dec.count_byte(value, spans) == [size for _, size in spans], hex(value)
    near = [(at, size) for _, at, size, _ in far.blocks if at >= NEAR or at + size >= NEAR]
    assert len(near) >= 5
    for at, size in near:
        assert dec.copy_output(at, min(4096, size)) == far.raw.slice(at, at + min(4096, size)), at
        assert dec.copy_output(at + size - min(4096, size), min(4096, size)) == far.raw.slice(at + size - min(4096, size), at + size)
    check_texts(far, dec)
    # no byte of a filler's value outside it, next to its edges
    for at, size, value in fillers[-4:]:
        assert dec.count_byte(value, [(at - 4096, size + 8192)]) == [size]


def gather_pieces(far):
    """[(source, destination, size)] and the destination's size: every source misalignment 0..15 with the sizes of
    test_gpu_ranges.test_device_destination, sources in [2^32 - 70 000, 2^32 + 70 000) -- the small ones around 2^32 itself,
    the long ones ending on or behind it -- and in T2."""
    pieces, at = [], 0
    for sm in range(16):
        for size in (0, 1, 15, 16, 17, 40, 70_000):
            for base in (CUT - 70_000 if size == 70_000 else CUT - 16 * (size // 32), (far.t2_at + 1600) & ~15):
                at += 1 + sm % 3
                pieces.append((base + sm, at, size))
                at += size
    return pieces, at


def test_gather_to_host(far, far_batch):
    dec, _, _ = far_batch
    pieces, end = gather_pieces(far)
    assert all(CUT - 70_000 <= s and s + n <= CUT + 70_000 or s >= far.t2_at for s, _, n in pieces)
    assert {s % 16 for s, _, n in pieces if s < CUT < s + n} == set(range(16)) and any(s == CUT for s, _, n in pieces)
    assert len({d % 16 for _, d, _ in pieces}) == 16
    want = bytearray(end)
    for s, d, n in pieces:
        want[d:d + n] = far.raw.slice(s, s + n)
    assert dec.gather_output(pieces) == bytes(want)


def test_gather_to_device(native, far, far_batch):
    """k_gather into device memory.  No torch is needed for the destination, so no child process either: libamdhip64.so is
    already in this process (libmi355x_bz2.so links to it, and the far_batch fixture has loaded that), so the loader hands
    CDLL the same runtime, and the pointer it allocates is one the library's kernels can write."""
    dec, _, _ = far_batch
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    pieces, end = gather_pieces(far)
    device = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(device), end + 16) == 0
    try:
        assert hip.hipMemset(device, 0xCD, end + 16) == 0
        dec.gather_output_to_device(pieces, device.value)
        host = ctypes.create_string_buffer(end + 16)
        assert hip.hipMemcpy(host, device, end + 16, 2) == 0          # hipMemcpyDeviceToHost
    finally:
        hip.hipFree(device)
    want = bytearray(b"\xcd" * (end + 16))
    for s, d, n in pieces:
        want[d:d + n] = far.raw.slice(s, s + n)
    assert host.raw == bytes(want)


def test_newlines_across_the_cut(far, far_batch):
    dec, _, total = far_batch
    newlines = far.raw.newline_offsets()
    assert newlines.dtype == np.uint64
    below, above = int(newlines[newlines < CUT][-1]), int(newlines[newlines >= CUT][0])
    assert below < CUT - 100 and above > CUT + 100

    def count(a, b):
        return int(np.count_nonzero((newlines >= a) & (newlines < b)))

    end = far.t1_at + len(far.t1)
    spans = [(CUT - 40_000 - k, 80_000 + k + 3 * k) for k in range(16)]             # 16 alignments below, ends above
    spans += [(CUT, 70_000), (CUT + 1, end - CUT - 1), (far.t2_at, len(far.t0)), (CUT - 1, 2), (far.t1_at, total - far.t1_at),
              (0, total)]
    assert dec.count_byte(NL, spans) == [count(a, a + n) for a, n in spans]
    # the last newline below 2^32 and the first above it, by rank
    queries = []
    for a, n in spans[:16] + [(far.t1_at, len(far.t1)), (0, total)]:
        k = count(a, CUT)
        queries += [(a, n, k), (a, n, k + 1), (a, n, 1), (a, n, count(a, a + n)), (a, n, count(a, a + n) + 1)]
    got = dec.find_byte(NL, queries)
    for (a, n, rank), position in zip(queries, got):
        inside = newlines[(newlines >= a) & (newlines < a + n)]
        assert position == (int(inside[rank - 1]) if rank <= len(inside) else None), (a, n, rank)
    assert below in got and above in got
    # rank_byte at positions on both sides
    asked = []
    for a, n in spans[:16] + [(far.t1_at, total - far.t1_at), (0, total)]:
        for position in (a, a + 1, below, below + 1, CUT - 1, CUT, CUT + 1, above, above + 1, a + n - 1, a + n):
            if a <= position <= a + n:
                asked.append((a, n, position))
    assert dec.rank_byte(asked, NL) == [count(a, position) for a, n, position in asked]


@pytest.mark.parametrize("ignore_case", [False, True])
def test_strings_across_the_cut(far, far_batch, ignore_case):
    dec, _, total = far_batch
    raw, n = far.raw, bigfiles.needles()
    start, end = far.t1_at, far.t1_at + len(far.t1)
    long_at = CUT - 100                                      # the 256-byte needle; the 2-byte one starts at CUT - 1
    reached = 0
    for name in ("n2", "n16", "n17", "n256", "aXa", "abab", "n1"):
        pattern = n[name]
        m = len(pattern)
        at = {"n256": long_at, "n2": CUT - 1, "n1": CUT - 1}.get(name)
        spans = [(start, len(far.t1)), (CUT - 50_000, 100_000), (CUT, end - CUT), (far.t2_at, len(far.t0)), (0, len(far.t0))]
        if at is not None:
            # ends inside the needle at 2^32 (the end rule cuts it), exactly at its end, one byte further
            spans += [(start, CUT - start), (start, at + m - 1 - start), (start, at + m - start), (start, at + m + 1 - start),
                      (at, m), (at + 1, m), (at, m - 1)]
        want = [raw.find_all(pattern, a, a + size, ignore_case) for a, size in spans]
        assert dec.count_bytes(pattern, spans, ignore_case=ignore_case) == [len(w) for w in want], name
        positions, counts = dec.find_bytes(pattern, spans, ignore_case=ignore_case)
        assert counts == [len(w) for w in want] and positions == [p for w in want for p in w], name
        if at is not None:
            assert at in want[0] and at not in want[6] and at in want[7] and at in want[8] and want[9] == [at]
        # a capacity that is reached above 2^32: T1's matches below the cut and two more
        first = want[0]
        lower = sum(1 for p in first if p < CUT)
        if len(first) >= lower + 3:
            positions, counts = dec.find_bytes(pattern, spans[:1], capacity=lower + 2, ignore_case=ignore_case)
            assert positions == first[:lower + 2] and counts == [len(first)] and positions[-1] > CUT
            reached += 1
        # T2 gives T0's answers plus the shift
        assert [p - far.shift for p in want[3]] == want[4] and len(want[4]) > 0
    assert reached >= 4
    # the sets
    patterns = [n["n256"], n["n2"], n["n16"], n["aXa"], n["n17"]]
    spans = [(start, len(far.t1)), (start, CUT + 155 - start), (start, CUT + 156 - start), (start, CUT + 157 - start),
             (start, CUT - start), (CUT - 1, 2), (far.t2_at, len(far.t0)), (0, len(far.t0))]
    want = []
    for a, size in spans:
        pairs = sorted((p, i) for i, pattern in enumerate(patterns) for p in raw.find_all(pattern, a, a + size, ignore_case))
        want.append(pairs)
    counts, each = dec.count_bytes_set(patterns, spans, ignore_case=ignore_case)
    assert counts == [len(w) for w in want]
    assert each == [sum(1 for w in want for _, i in w if i == k) for k in range(len(patterns))]
    positions, ids, counts = dec.find_bytes_set(patterns, spans, ignore_case=ignore_case)
    assert list(zip(positions, ids)) == [pair for w in want for pair in w] and counts == [len(w) for w in want]
    assert (long_at, 0) in want[2] and (long_at, 0) not in want[1] and (CUT - 1, 1) in want[5]
    lower = sum(1 for p, _ in want[0] if p < CUT)
    assert len(want[0]) >= lower + 3
    positions, ids, counts = dec.find_bytes_set(patterns, spans[:1], capacity=lower + 2, ignore_case=ignore_case)
    assert list(zip(positions, ids)) == want[0][:lower + 2] and positions[-1] > CUT and counts == [len(want[0])]
    assert [(p - far.shift, i) for p, i in want[6]] == want[7]


def plain_crc(data):
    """bzip2's CRC-32 of data, bit by bit through a table made here."""
    table = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
        table.append(c)
    crc = 0xFFFFFFFF
    for byte in data:
        crc = ((crc << 8) & 0xFFFFFFFF) ^ table[(crc >> 24) ^ byte]
    return crc ^ 0xFFFFFFFF


def test_crc32_of_pieces_beyond_4_gib(far, far_batch):
    """k_crc over pieces of the batch's output: per block, the whole output as ONE piece of more than 2^32 bytes (its
    checksum folded from libbz2's own per-block checksums with bigfiles.crc_concat), and pieces that meet around 2^32."""
    dec, results, total = far_batch
    sizes = [r["decoded_size"] for r in results]
    assert dec.crc32_device(dec.output_device_ptr(), sizes) == [r["header_crc"] for r in results]

    def folded(parts):
        crc = 0                                              # bzip2's CRC of no bytes
        for value, size in parts:
            crc = bigfiles.crc_concat(crc, value, size)
        return crc

    blocks = [(r["header_crc"], r["decoded_size"]) for r in results]
    whole = folded(blocks)
    began = time.time()
    assert dec.crc32_device(dec.output_device_ptr(), [total]) == [whole]
    print(f"\ncrc32_device of one piece of {total} bytes: {time.time() - began:.2f} s")
    # [2^32 - 16, 32, rest]: the middle piece from the bytes themselves, the outer ones by taking the whole apart
    got = dec.crc32_device(dec.output_device_ptr(), [CUT - 16, 32, total - CUT - 16])
    assert got[1] == plain_crc(far.raw.slice(CUT - 16, CUT + 16))
    assert folded([(got[0], CUT - 16), (got[1], 32), (got[2], total - CUT - 16)]) == whole
    # the head alone: the blocks in front of T1's block around the cut, and that block's bytes below 2^32 - 16
    k = next(i for i, (_, at, size, _) in enumerate(far.blocks) if at < CUT < at + size)
    at = far.blocks[k][1]
    piece = far.raw.slice(at, CUT - 16)
    assert got[0] == folded(blocks[:k] + [(plain_crc(piece), len(piece))])


def test_batch_with_kept_stages(native, far):
    """Once more on a context that keeps its stages: the records and the bytes of T1 and T2."""
    dec, results, total, seconds = decode_all(native, far, flags=native.Decoder.KEEP_STAGES)
    try:
        print(f"\nfar batch, stages kept: {seconds:.2f} s; device memory {dec.device_memory()}")
        check_records(far, results, total)
        check_texts(far, dec)
    finally:
        dec.close()


# ------------------------------------------------- A2. the line queries on the batch: regex, line hashes, field spans, keys
#
# Decoder.match_lines, hash_lines, field_spans and field_hashes over spans of the resident batch.  Every expected value is
# VirtualRaw's (tests/bigfiles.py): summaries, hashes, keys, starts and sizes exactly.  For the regular expressions the
# matching lines are Python's re (VirtualRaw.regex_lines); the head map and the exit state are the compiled table walked
# over the span's first and last line alone (regexgen.chunk_summary), as test_gpu_regex.py walks it over whole spans; a
# witness may be any byte of its line, so the witnesses are compared as the numbers of the lines they lie in.

QUERY_SIZES = (1, 255, 256, 257, 65_535, 65_536, 65_537, 140_000)
ONES, UNTOUCHED = 2**64 - 1, -1 - 2**62
FIELD_KEYS = ("count", "has_delimiter", "first_nl", "head_positions", "tail_start", "tail_delims", "tail_field_start",
              "tail_field_end", "tail_non_empty")
HASH_KEYS = ("head", "tail", "head_hashes", "tail_start_hash", "tail_end_hash")
WANTED = {}                      # the reference of a span, computed once, shared by the tests, never changed


def wanted(raw, kind, *arguments):
    key = (id(raw), kind) + arguments
    if key not in WANTED:
        WANTED[key] = getattr(raw, kind)(*arguments)
    return WANTED[key]


def query_spans(far):
    """(aligned, fixed): every size at all 16 start misalignments, ending below 2^32, across it and starting at or above
    it; and the fixed ones: from and to 2^32 exactly, empty at 2^32, in T2, and 2^32 on a tile edge, on a chunk edge that is
    no tile edge and inside a chunk of the span (tiles and chunks are counted from the span's start)."""
    aligned = []
    for sm in range(16):
        for size in QUERY_SIZES:
            aligned.append((((CUT - size - 32) & ~15) + sm, size))
            across = ((CUT - size // 2 - 16) & ~15) + sm
            if across < CUT < across + size:
                aligned.append((across, size))
            aligned.append((CUT + sm, size))
    fixed = [(CUT, 70_000), (CUT - 70_000, 70_000), (CUT, 0), (far.t2_at + 5_000, 70_001), (CUT - 65_536, 140_000),
             (CUT - 3 * 256, 65_537), (CUT - 2 * 65_536 - 100, 140_000)]
    return aligned, fixed


def test_query_spans_cover_what_they_claim(native, far):
    aligned, fixed = query_spans(far)
    below = [(a, n) for a, n in aligned if a + n < CUT]
    across = [(a, n) for a, n in aligned if a < CUT < a + n]
    above = [(a, n) for a, n in aligned if a >= CUT]
    assert len(below) + len(across) + len(above) == len(aligned)
    for group, sizes in ((below, QUERY_SIZES), (across, QUERY_SIZES[1:]), (above, QUERY_SIZES)):
        assert {(a % 16, n) for a, n in group} == {(sm, n) for sm in range(16) for n in sizes}
    N = native._native
    assert N.regex_chunk_bytes() == N.line_hash_chunk_bytes() == N.field_chunk_bytes() == 256
    edge = lambda span, unit: span[0] < CUT < span[0] + span[1] and (CUT - span[0]) % unit == 0
    assert edge(fixed[4], 65_536) and edge(fixed[5], 256) and not edge(fixed[5], 65_536) and not edge(fixed[6], 256)
    assert fixed[6][0] < CUT < fixed[6][0] + fixed[6][1]
    assert all(a + n <= far.t1_at + len(far.t1) and a >= far.t1_at for a, n in aligned + fixed[:3] + fixed[4:])


def check_hash_lines(dec, raw, spans, newline=b"\n", seed=0, capacity=None, room=None):
    want = [wanted(raw, "hash_summary", a, n, newline, seed) for a, n in spans]
    summaries, hashes = dec.hash_lines(spans, newline, seed, capacity, room)
    assert hashes.dtype == np.uint64
    for span, got, (summary, _) in zip(spans, summaries, want):
        assert got == summary, (span, newline, seed)
    flat = [h for _, closed in want for h in closed]
    written = len(flat) if capacity is None else min(capacity, len(flat))
    assert hashes[:written].tolist() == flat[:written], (spans[:3], newline, seed)
    assert (hashes[written:] == ONES).all(), "written at or beyond the capacity"
    return want


def check_fields(dec, raw, spans, field, delimiter=b" ", newline=b"\n", seed=None, capacity=None, room=None):
    """Decoder.field_spans (seed None) or Decoder.field_hashes against VirtualRaw, exactly."""
    if seed is None:
        want = [wanted(raw, "field_summary", a, n, field, delimiter, newline) for a, n in spans]
        summaries, starts, sizes = dec.field_spans(spans, field, delimiter, newline, capacity, room)
        keys, names = None, FIELD_KEYS
    else:
        want = [wanted(raw, "field_hash_summary", a, n, field, delimiter, newline, seed) for a, n in spans]
        summaries, keys, starts, sizes = dec.field_hashes(spans, field, delimiter, newline, seed, capacity, room)
        names = FIELD_KEYS + HASH_KEYS
    assert starts.dtype == np.uint64 and sizes.dtype == np.int64
    for span, got, model in zip(spans, summaries, want):
        assert got == {name: model[name] for name in names}, (span, field, delimiter, newline, seed)
    flat = [pair for model in want for pair in model["fields"]]
    written = len(flat) if capacity is None else min(capacity, len(flat))
    assert starts[:written].tolist() == [s for s, _ in flat[:written]], (spans[:3], field)
    assert sizes[:written].tolist() == [n for _, n in flat[:written]], (spans[:3], field)
    assert (starts[written:] == ONES).all() and (sizes[written:] == UNTOUCHED).all(), "written at or beyond the capacity"
    if keys is not None:
        assert keys.dtype == np.uint64
        assert keys[:written].tolist() == [k for model in want for k in model["keys"]][:written], (spans[:3], field, seed)
        assert (keys[written:] == ONES).all()
    return want, flat


def check_match_lines(native, dec, raw, spans, pattern, newline=b"\n", ignore_case=False, capacity=None):
    """The spans begin and end in lines without a filler; the lines in between may hold any."""
    import regexgen as G
    compiled = native.compile_regex(pattern, ignore_case)
    transitions, accepts = compiled.transitions.tolist(), compiled.accepts_at_end.tolist()
    cuts = raw.byte_offsets(newline[0])
    bounds = raw.line_bounds(newline)
    matching = raw.regex_lines(pattern, newline, ignore_case)
    head_maps, has_delimiter, exits, positions, counts = dec.match_lines(spans, compiled, newline, capacity)
    want_lines = []
    for i, (a, n) in enumerate(spans):
        inside = raw._within(cuts, a, a + n)
        # the head map: every entry state walked over the span's first line (regexgen.chunk_summary's rule, all states at once)
        states = np.arange(compiled.states)
        for byte in raw.slice(a, inside[0] if inside else a + n):
            states = compiled.transitions[states, byte]
        assert head_maps[i].tolist() == states.tolist() + [0] * (64 - compiled.states) and has_delimiter[i] == bool(inside), (pattern, a, n)
        lines = []
        if inside:
            first, last = raw.line_of(inside[0] + 1, newline), raw.line_of(inside[-1] + 1, newline)
            lines = [k for k in matching[np.searchsorted(matching, first):np.searchsorted(matching, last)]]
            tail = G.chunk_summary(transitions, accepts, newline + raw.slice(inside[-1] + 1, a + n), newline[0])
            assert exits[i] == tail.exit, (pattern, a, n)
            lines += [last] if tail.witnesses else []
            assert all(bounds[k][0] > a for k in lines)
        else:
            assert exits[i] == 0
        assert counts[i] == len(lines), (pattern, a, n)
        want_lines += lines
    written = len(want_lines) if capacity is None else min(capacity, len(want_lines))
    assert len(positions) == written
    got_lines = np.searchsorted(cuts, np.array(positions, dtype=np.uint64), "left").tolist()
    assert got_lines == want_lines[:written], (pattern, spans[:3])
    # one witness per line, inside the span that lists it, ascending within it
    at = 0
    for (a, n), count in zip(spans, counts):
        mine = positions[at:at + count]
        assert all(a <= p < a + n for p in mine) and mine == sorted(set(mine))
        at += count
    return positions, want_lines


def test_hash_lines_around_2_32(far, far_batch):
    dec, _, total = far_batch
    aligned, fixed = query_spans(far)
    check_hash_lines(dec, far.raw, aligned)
    check_hash_lines(dec, far.raw, fixed + aligned[::5], seed=1)
    check_hash_lines(dec, far.raw, fixed + aligned[3::7], newline=b" ")
    # a capacity that is reached above 2^32
    span = [(far.t1_at + 100, len(far.t1) - 100)]
    lower = far.raw.line_of(CUT) - far.raw.line_of(span[0][0])
    want = check_hash_lines(dec, far.raw, span, capacity=lower + 2, room=lower + 50)
    assert len(want[0][1]) > lower + 50


def test_hash_lines_of_the_whole_output(far, far_batch):
    dec, _, total = far_batch
    raw = far.raw
    t1_line = raw.line_of(far.t1_at)
    for seed in (0, 1):
        (summary, hashes), = check_hash_lines(dec, raw, [(0, total)], seed=seed)
        assert hashes == raw.line_hashes(b"\n", seed) and summary["count"] == len(hashes) == 39_214
        assert hashes[t1_line] == raw.part(len(far.t0), raw.line_bounds()[t1_line][1], bigfiles.linehash.base(seed))[0]
        # no delimiter from the first filler's first byte to the end: the head is (h, x^len) of more than 2^32 bytes
        span = (len(far.t0), total - len(far.t0))
        (summary, hashes), = check_hash_lines(dec, raw, [span], newline=b"\0", seed=seed)
        x = bigfiles.linehash.base(seed)
        assert span[1] > CUT and hashes == [] and summary["count"] == 0 and not summary["has_delimiter"]
        assert summary["head"][1] == pow(x, span[1], bigfiles.linehash.P) and summary["tail"] == (0, 1)
    print(f"\ndevice memory after the whole-output span: {dec.device_memory()}")


@pytest.mark.parametrize("seed", [None, 0, 1], ids=["spans", "keys-seed0", "keys-seed1"])
def test_fields_around_2_32(far, far_batch, seed):
    dec, _, total = far_batch
    raw = far.raw
    aligned, fixed = query_spans(far)
    if seed != 1:
        check_fields(dec, raw, aligned, 3, seed=seed)
    for field in (0, 3, 4, 8, 9, 1023):
        check_fields(dec, raw, fixed + aligned[field % 5::5 if seed is None else 11], field, seed=seed)
    check_fields(dec, raw, fixed + aligned[2::9], 1, delimiter=b"e", seed=seed)
    check_fields(dec, raw, fixed + aligned[4::9], 2, delimiter=b"\n", newline=b" ", seed=seed)
    # the line across 2^32 closed by a span that starts in front of it: its field 4 starts below 2^32 and ends above
    k = raw.line_of(CUT)
    a, b = raw.line_bounds()[k]
    for field, pair in ((4, (CUT - 101, 257)), (8, (CUT + 169, 8)), (9, (CUT + 177, -1))):
        want, flat = check_fields(dec, raw, [(a - 1, b - a + 2)], field, seed=seed)
        assert flat[1:] == [pair]
    # a capacity that is reached above 2^32
    span = [(far.t1_at + 100, len(far.t1) - 100)]
    lower = k - raw.line_of(span[0][0])
    want, flat = check_fields(dec, raw, span, 4, seed=seed, capacity=lower + 2, room=lower + 50)
    assert len(flat) > lower + 50 and flat[lower - 1][0] < CUT < flat[lower + 1][0]


@pytest.mark.parametrize("seed", [None, 0, 1], ids=["spans", "keys-seed0", "keys-seed1"])
def test_fields_of_the_whole_output(far, far_batch, seed):
    dec, _, total = far_batch
    raw = far.raw
    t1_line, k = raw.line_of(far.t1_at), raw.line_of(CUT)
    for field in (0, 3) if seed is None else (0, 4):
        (summary,), flat = check_fields(dec, raw, [(0, total)], field, seed=seed)
        assert flat == raw.field_spans(field, b" ") and len(flat) == 39_214
        assert sum(1 for start, _ in flat if start > CUT) > 13_000
        if seed is not None:
            assert summary["keys"] == raw.field_keys(field, b" ", b"\n", seed)
        if field == 0:
            assert flat[t1_line] == (len(far.t0), 4_293_517_388)           # the largest field of the file
        if field == 4:
            assert flat[k] == (CUT - 101, 257)
    # no newline from the first filler's first byte to the end: nothing is closed, the tail is the span, all above 2^31
    span = (len(far.t0), total - len(far.t0))
    (summary,), flat = check_fields(dec, raw, [span], 0, delimiter=b"\t", newline=b"\0", seed=seed)
    assert flat == [] and summary["count"] == 0 and summary["tail_field_start"] == 0 and summary["tail_field_end"] is None
    # ... and with the spaces as delimiters: field 1 starts behind the 94 fillers, above 2^32 - 2^21 of the span
    (summary,), flat = check_fields(dec, raw, [span], 1, newline=b"\0", seed=seed)
    assert summary["tail_field_start"] == far.t1_at + 17 - span[0] and summary["tail_field_end"] > summary["tail_field_start"]
    # the last line of the whole output is closed: the tail starts at the end, above 2^32
    (summary,), _ = check_fields(dec, raw, [(5, total - 5)], 0, seed=seed)
    assert summary["tail_start"] == total - 5 > CUT and summary["tail_field_start"] == total - 5
    # a span that ends inside the line across 2^32, behind its field 4: the tail's positions are above 2^32 of the span
    (summary,), _ = check_fields(dec, raw, [(0, CUT + 170)], 4, seed=seed)
    assert summary["tail_start"] == CUT - 131 and summary["tail_field_start"] == CUT - 101 and summary["tail_field_end"] == CUT + 156
    (summary,), _ = check_fields(dec, raw, [(7, CUT + 170)], 8, seed=seed)
    assert summary["tail_field_start"] == CUT + 169 - 7 > CUT and summary["tail_field_end"] is None
    print(f"\ndevice memory after the whole-output span: {dec.device_memory()}")


@pytest.mark.parametrize("ignore_case", [False, True], ids=["exact", "ignore-case"])
def test_match_lines_around_2_32(native, far, far_batch, ignore_case):
    dec, _, total = far_batch
    raw = far.raw
    aligned, fixed = query_spans(far)
    k = raw.line_of(CUT)
    check_match_lines(native, dec, raw, aligned, bigfiles.FAR_PATTERNS["class"], ignore_case=ignore_case)
    for name in ("caret", "dollar", "across", "short", "nowhere"):
        check_match_lines(native, dec, raw, fixed + aligned[len(name)::7], bigfiles.FAR_PATTERNS[name], ignore_case=ignore_case)
    # the line across 2^32 as a body line, and entered in its middle (then the head map carries it)
    a, b = raw.line_bounds()[k]
    for name in ("caret", "dollar", "across"):
        positions, lines = check_match_lines(native, dec, raw, [(a - 1, b - a + 2), (CUT, b - CUT + 1)], bigfiles.FAR_PATTERNS[name],
                                             ignore_case=ignore_case)
        assert lines == [k] and a <= positions[0] <= b
    # a capacity that is reached above 2^32
    span = [(far.t1_at + 100, len(far.t1) - 100)]
    _, lines = check_match_lines(native, dec, raw, span, bigfiles.FAR_PATTERNS["class"], ignore_case=ignore_case)
    lower = sum(1 for n in lines if n < k)
    positions, _ = check_match_lines(native, dec, raw, span, bigfiles.FAR_PATTERNS["class"], ignore_case=ignore_case, capacity=lower + 2)
    assert len(lines) > lower + 5 and positions[-1] > CUT > positions[lower - 1]


def test_match_lines_of_the_whole_output(native, far, far_batch):
    import regexgen as G
    dec, _, total = far_batch
    raw = far.raw
    k, t1_line = raw.line_of(CUT), raw.line_of(far.t1_at)
    # (a pass over the 4.39 GB takes about a second -- every chunk of a filler is all head, walked for every state -- so
    # the patterns that need no filler are left to test_match_lines_around_2_32)
    for name in ("across", "t2-only", "ascii-tail"):
        pattern = bigfiles.FAR_PATTERNS[name]
        positions, lines = check_match_lines(native, dec, raw, [(0, total)], pattern)
        assert lines == [n for n in raw.regex_lines(pattern) if n > 0] and len(lines) == 1
        if name == "across":
            assert lines == [k] and CUT - 131 <= positions[0] <= CUT + 177
        if name in ("across", "t2-only"):
            assert positions[0] >= CUT                                      # the witness does not fit 32 bits
        if name == "ascii-tail":
            assert lines == [t1_line] and far.t1_at - 256 < positions[0] < far.t1_at + 100       # (a chunk's first byte may stand for it)
    # X in T0, every filler, Y in T1, one line under another delimiter: the state behind X survives 66 000 tiles
    pattern, newline = bigfiles.FAR_CARRIED
    positions, lines = check_match_lines(native, dec, raw, [(0, total)], pattern, newline)
    assert lines == [3] and far.t1_at - 256 < positions[0] < CUT
    # no delimiter from the first filler's first byte to the end
    span = (len(far.t0), total - len(far.t0))
    for pattern, matched in ((rb"N3eDLe#16-MiXed\. qtl", True), (bigfiles.FAR_PATTERNS["nowhere"], False)):
        head_maps, has_delimiter, exits, positions, counts = dec.match_lines([span], pattern, b"\0")
        assert (head_maps[0][G.START] == G.MATCHED) == matched and has_delimiter == [False] and positions == [] and counts == [0]
    print(f"\ndevice memory after the whole-output span: {dec.device_memory()}")


def test_field_of_more_than_4_gib(native, far, far_batch):
    """The same blocks in another order (bigfiles.long_field_batch): between T0's last byte and T2's first lie all 96 fillers,
    more than 2^32 bytes of one line, closed inside the span.  Under newline b" " and delimiter b"\\n" its field 1 is larger
    than 2^32 and does not start the line: k_fieldhash_finish raises x to a size with bits above 31 and multiplies a P(start)
    that is not 0 by it; k_field_sizes subtracts across 2^32; the line's hash is carried over 66 000 tiles."""
    blocks, raw = bigfiles.long_field_batch(far)
    dec = native.Decoder(device=0, max_batch_blocks=1)
    try:
        dec.share_input(far_batch[0])
        results, total = dec.decode_batch([bit for bit, _, _, _ in blocks])
        assert total == raw.size and [r["status"] for r in results] == [0] * len(blocks)
        span = (len(far.t0) - 3_000, total - 2 * len(far.t0) + 6_000)
        at = raw.line_of(len(far.t0), b" ") - raw.line_of(span[0], b" ") - 1           # of the long line among the closed ones
        for seed in (0, 1):
            x = bigfiles.linehash.base(seed)
            (summary, hashes), = check_hash_lines(dec, raw, [span], newline=b" ", seed=seed)
            a, b = raw.line_bounds(b" ")[raw.line_of(len(far.t0), b" ")]
            assert b - a > CUT and hashes[at + 1] == raw.part(a, b, x)[0]
            for field in (0, 1, 2):
                (summary,), flat = check_fields(dec, raw, [span], field, delimiter=b"\n", newline=b" ", seed=seed)
                if field == 1:
                    assert flat[at + 1] == (len(far.t0), b - len(far.t0)) and flat[at + 1][1] > CUT
                    assert summary["keys"][at + 1] == raw.part(len(far.t0), b, x)[0] not in (0, bigfiles.fieldhash.MISSING)
        (summary,), flat = check_fields(dec, raw, [span], 1, delimiter=b"\n", newline=b" ")
        assert flat[at + 1][1] > CUT
        memory = dec.device_memory()
        print(f"\nthe batch with one field of {flat[at + 1][1]} bytes: device memory {memory}")
        assert memory["scratch_bytes"] + memory["output_bytes"] < 32 << 30
    finally:
        dec.close()


def test_device_memory_after_the_line_queries(far_batch):
    memory = far_batch[0].device_memory()
    print(f"\nfar batch after the line queries: device memory {memory}")
    assert memory["scratch_bytes"] + memory["output_bytes"] < 32 << 30


# ----------------------------------------------------------------------------------------- B. the reader on far_file()

@pytest.fixture(scope="module")
def far_path(far, tmp_path_factory):
    path = tmp_path_factory.mktemp("far") / "far.bz2"
    path.write_bytes(far.enc)
    return str(path)


def device_free():
    """Free bytes on the current device, asked of the HIP runtime the library itself has loaded."""
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


@pytest.fixture(scope="module", params=[(1, "fly"), (4, "fly"), (1, "map"), (4, "map")], ids=lambda p: f"p{p[0]}-{p[1]}")
def reader(request, native, far, far_path):
    """The reader at parallelization 1 and 4: on the fly (block_offsets() is the one full pass, which finds the block
    map), and with the arithmetic map imported."""
    parallelization, mode = request.param
    free_before = device_free()
    f = native.open(far_path, parallelization=parallelization)
    began = time.time()
    if mode == "map":
        f.set_block_offsets(far.map)
    else:
        assert f.block_offsets() == far.map
        print(f"\nfar on the fly at parallelization {parallelization}: block map after {time.time() - began:.2f} s; "
              f"{f.statistics()}")
    yield f, mode
    # the reader's buffers only grow, so what it holds after its tests is its peak
    held = free_before - device_free()
    print(f"\nfar reader at parallelization {parallelization} ({mode}): {held / 2**30:.2f} GiB held on the device after its tests")
    assert held < 32 << 30
    f.close()


def short_lines(far, positions):
    """The matches (positions) whose lines are short: not the lines that hold a filler."""
    newlines = far.raw.newline_offsets()
    keep = []
    for p in positions:
        k = int(np.searchsorted(newlines, p, "left"))
        start = int(newlines[k - 1]) + 1 if k > 0 else 0
        end = int(newlines[k]) + 1 if k < len(newlines) else far.raw.size
        if end - start < 100_000:
            keep.append(p)
    return keep


def test_reader_positions(far, reader):
    f, mode = reader
    raw = far.raw
    assert f.size() == raw.size
    if mode == "fly":
        assert f.block_offsets_complete() and f.block_offsets() == far.map
    assert f.seek(CUT - 1000) == CUT - 1000
    assert f.read(2000) == raw.slice(CUT - 1000, CUT + 1000)
    assert f.tell() == CUT + 1000
    assert f.seek(-3000, os.SEEK_CUR) == CUT - 2000 and f.tell() == CUT - 2000
    assert f.seek(-(raw.size - CUT) - 5, os.SEEK_END) == CUT - 5
    buffer = bytearray(70_000)
    assert f.readinto(buffer) == 70_000 and bytes(buffer) == raw.slice(CUT - 5, CUT + 69_995)
    assert f.tell() == CUT + 69_995
    assert f.seek(far.t2_at + 17) == far.t2_at + 17 and f.read(5000) == far.t0[17:5017]
    assert f.seek(-100, os.SEEK_END) == raw.size - 100 and f.read() == far.t0[-100:]
    assert f.tell() == raw.size and f.read(10) == b""
    assert f.seek(0) == 0 and f.read(3000) == far.t0[:3000]


def seeded_ranges(far, seed=0xFA12, count=50):
    """(offset, size): at least one end within 2^20 of 2^32 or in T2; empty ones, ones beyond the end, duplicates."""
    r = np.random.default_rng(seed)
    size = far.raw.size
    ranges = [(CUT - 1, 2), (CUT, 1), (CUT - 1, 1), (CUT, 0), (CUT - 70_000, 140_000), (size - 10, 100), (size, 5),
              (size + 7, 3), (far.t2_at - 5, 10), (far.t1_at - 3, 6), (CUT - 100, 256), (CUT - 100, 256)]
    while len(ranges) < count:
        kind = len(ranges) % 4
        if kind == 0:      # ends near the cut
            end = CUT - (1 << 20) + int(r.integers(0, 2 << 20))
            ranges.append((end - int(r.integers(0, 300_000)), 0))
            ranges[-1] = (ranges[-1][0], end - ranges[-1][0])
        elif kind == 1:    # starts near the cut
            ranges.append((CUT - (1 << 20) + int(r.integers(0, 2 << 20)), int(r.integers(0, 300_000))))
        elif kind == 2:    # in T2
            ranges.append((far.t2_at + int(r.integers(0, len(far.t0))), int(r.integers(0, 200_000))))
        else:              # from T0 or a low filler into T2: a start far below 2^32 in the same call as an end far above it
            start = int(r.integers(0, 2 * len(far.t0)))
            ranges.append((start, 0))
            ranges += [(far.t2_at + start, int(r.integers(1, 5000)))] if len(ranges) < count else []
    near = lambda p: CUT - (1 << 20) <= p < CUT + (1 << 20) or p >= far.t2_at
    assert all(near(o) or near(o + s) or s == 0 for o, s in ranges)
    return ranges


def test_reader_ranges(far, reader):
    f, mode = reader
    ranges = seeded_ranges(far)
    assert len(ranges) == 50 and len(set(ranges)) < 50 and any(s == 0 for _, s in ranges)
    f.seek(CUT + 12345)
    got = f.read_ranges(ranges)
    for (offset, size), piece in zip(ranges, got):
        assert piece == far.raw.slice(offset, offset + size), (offset, size)
    assert f.tell() == CUT + 12345                                     # positionless
    assert f.read(100) == far.raw.slice(CUT + 12345, CUT + 12445)


def test_only_touched_blocks_are_decoded(native, far, far_path):
    """With the imported map, reads and range reads around 2^32 and in T2 decode the blocks they overlap (and what prefetch
    may add to a sequential read), not the 4 GiB in front of them."""
    starts = sorted((at, at + size) for _, at, size, _ in far.blocks)

    def overlapped(ranges):
        return {a for a, b in starts for offset, size in ranges if size > 0 and a < offset + size and offset < b}

    for parallelization in (1, 4):
        with native.open(far_path, parallelization=parallelization) as f:
            f.set_block_offsets(far.map)
            before = f.statistics()["blocks_decoded"]
            ranges = [(CUT - 1000, 2000), (far.t2_at + 5, 100), (CUT - 70_000, 140_000), (far.raw.size - 50, 50)]
            assert f.read_ranges(ranges) == [far.raw.slice(o, o + s) for o, s in ranges]
            assert f.statistics()["blocks_decoded"] - before == len(overlapped(ranges))
            before = f.statistics()["blocks_decoded"]
            f.seek(CUT - 1000)
            assert f.read(2000) == far.raw.slice(CUT - 1000, CUT + 1000)
            decoded = f.statistics()["blocks_decoded"] - before
            # the block read and some look-ahead behind it, not the hundred blocks in front of it
            assert 1 <= decoded <= 16, decoded


def test_reader_lines(far, reader):
    f, mode = reader
    raw = far.raw
    newlines = raw.newline_offsets()
    starts = raw.line_starts()
    n = len(newlines)
    index = f.line_offsets()
    block_starts = sorted(at for _, at, size, _ in far.blocks)
    assert sorted(index) == block_starts + [raw.size]
    assert list(index) == sorted(index)                                  # ascending as it comes
    assert all(index[at] == raw.line_of(at) for at in index)
    assert index[raw.size] == n and max(index) > CUT and f.count_lines() == n
    k = raw.line_of(CUT)                                                 # the line that straddles 2^32
    assert int(starts[k]) < CUT < int(newlines[k])
    t2_line = raw.line_of(far.t2_at + 5000)
    asked = [0, 1, k - 1, k, k + 1, t2_line, n - 1, n, n + 1, n + 50]
    got = f.line_starts(asked)
    assert got.dtype == np.uint64
    assert list(got) == [int(starts[i]) if i <= n else raw.size for i in asked]
    ranges = [(k, 1), (k - 1, 3), (k + 1, 2), (t2_line, 2), (0, 2), (n - 2, 5), (n + 3, 1), (k, 0)]
    want = [raw.slice(a, b) for a, b in raw.line_ranges(ranges)]
    assert f.read_line_ranges(ranges) == want
    assert f.read_lines(k) == want[0] and len(want[0]) > 256 and bigfiles.needles()["n256"] in want[0]
    offsets = [0, 5, int(starts[k]), CUT - 1, CUT, CUT + 1, int(newlines[k]), int(newlines[k]) + 1, far.t2_at, far.t2_at + 5000,
               raw.size - 1, raw.size, raw.size + 9, CUT - 1]
    numbers = f.line_numbers(offsets)
    assert numbers.dtype == np.uint64 and list(numbers) == [raw.line_of(p) for p in offsets]


def test_imported_line_index(native, far, far_path):
    """set_line_offsets with the arithmetic index: lines around 2^32 and in T2 without the pass that builds it."""
    raw = far.raw
    index = {at: raw.line_of(at) for _, at, _, _ in far.blocks}
    index[raw.size] = len(raw.newline_offsets())
    k = raw.line_of(CUT)
    with native.open(far_path, parallelization=4) as f:
        f.set_block_offsets(far.map)
        f.set_line_offsets(index)
        before = f.statistics()["blocks_decoded"]
        assert f.line_offsets() == index
        ranges = [(k, 1), (raw.line_of(far.t2_at + 70_000), 3)]
        assert f.read_line_ranges(ranges) == [raw.slice(a, b) for a, b in raw.line_ranges(ranges)]
        assert list(f.line_numbers([CUT, far.t2_at + 70_000])) == [k, raw.line_of(far.t2_at + 70_000)]
        assert f.statistics()["blocks_decoded"] - before <= 8
        with pytest.raises((ValueError, native.Bz2Error)):
            f.set_line_offsets({**index, raw.size: index[raw.size] + 2**33})


@pytest.mark.parametrize("ignore_case", [False, True], ids=["exact", "ignore-case"])
def test_reader_search(far, reader, ignore_case):
    f, mode = reader
    raw, n = far.raw, bigfiles.needles()
    t1_end = far.t1_at + len(far.t1)
    bounds = [(0, None), (far.t1_at, t1_end), (CUT - 100, CUT + 156), (CUT - 100, CUT + 155), (CUT - 99, None), (CUT, None),
              (far.t1_at, CUT), (far.t2_at, None), (CUT - 1, CUT + 1), (far.t2_at + 5, raw.size + 99)]
    for name in ("n2", "n16", "n256", "aXa"):
        pattern = n[name]
        for start, end in bounds if name == "n256" else bounds[1:]:      # (the whole file once: every block is decoded)
            want = raw.find_all(pattern, start, end, ignore_case)
            assert f.count_matches(pattern, start, end, ignore_case=ignore_case) == len(want), (name, start, end)
        for start, end in bounds[1:4] + bounds[5:]:
            want = raw.find_all(pattern, start, end, ignore_case)
            got = f.find_all(pattern, start, end, ignore_case=ignore_case)
            assert got.dtype == np.uint64 and list(got) == want, (name, start, end)
            assert f.find(pattern, start, end, ignore_case=ignore_case) == (want[0] if want else -1)
        # a limit that is reached above 2^32
        want = raw.find_all(pattern, far.t1_at, None, ignore_case)
        lower = sum(1 for p in want if p < CUT)
        assert len(want) > lower + 2
        assert list(f.find_all(pattern, far.t1_at, None, lower + 2, ignore_case=ignore_case)) == want[:lower + 2]
    # T2's answers are T0's plus the shift
    assert [p - far.shift for p in f.find_all(n["n17"], far.t2_at, None, ignore_case=ignore_case)] == \
        raw.find_all(n["n17"], 0, len(far.t0), ignore_case)
    # the set
    patterns = [n["n256"], n["n2"], n["n16"], n["aXa"], n["n17"]]
    for start, end in bounds[1:]:
        each = [raw.find_all(pattern, start, end, ignore_case) for pattern in patterns]
        assert list(f.count_matches_each(patterns, start, end, ignore_case=ignore_case)) == [len(e) for e in each]
        pairs = sorted((p, i) for i, e in enumerate(each) for p in e)
        positions, ids = f.find_all_any(patterns, start, end, ignore_case=ignore_case)
        assert positions.dtype == np.uint64 and list(zip(positions.tolist(), ids.tolist())) == pairs, (start, end)
        assert f.find_any(patterns, start, end, ignore_case=ignore_case) == (pairs[0] if pairs else (-1, -1))
    # the limit rule: the 256-byte pattern crosses 2^32 from 2^32 - 100, the 2-byte one lies at 2^32 - 1 behind it in the order
    # and inside whatever front ends at a block boundary behind: every limit around them gives the first pairs of the whole
    each = [raw.find_all(pattern, far.t1_at, None, ignore_case) for pattern in patterns]
    pairs = sorted((p, i) for i, e in enumerate(each) for p in e)
    at = pairs.index((CUT - 100, 0))
    assert (CUT - 1, 1) in pairs[at + 1:]
    for limit in (at, at + 1, at + 2, pairs.index((CUT - 1, 1)) + 1, len(pairs) - 1):
        positions, ids = f.find_all_any(patterns, far.t1_at, None, limit, ignore_case=ignore_case)
        assert list(zip(positions.tolist(), ids.tolist())) == pairs[:limit], limit


@pytest.mark.parametrize("ignore_case", [False, True], ids=["exact", "ignore-case"])
def test_reader_grep(far, reader, ignore_case):
    """Matches from behind T1's first newline on: the line in front of it holds the fillers, 4 GiB of them."""
    f, mode = reader
    raw, n = far.raw, bigfiles.needles()
    newlines = raw.newline_offsets()
    first = int(newlines[newlines > far.t1_at][0]) + 1
    t1_end = far.t1_at + len(far.t1)
    second = int(newlines[newlines > far.t2_at][0]) + 1
    for name in ("n256", "n16", "n2"):
        pattern = n[name]
        for start, end, limit in ((first, t1_end, None), (first, CUT + 156, None), (first, CUT + 155, None), (CUT - 1, t1_end, 3),
                                  (second, None, None), (second, None, 2), (CUT, t1_end, None)):
            numbers, ranges = raw.grep(pattern, start, end, limit, ignore_case=ignore_case)
            assert all(b - a < 100_000 for a, b in ranges)
            got_numbers, lines = f.grep(pattern, start, end, limit, ignore_case=ignore_case)
            assert got_numbers.dtype == np.uint64 and list(got_numbers) == numbers, (name, start, end, limit)
            assert lines == [raw.slice(a, b) for a, b in ranges]
            assert f.count_matching_lines(pattern, start, end, ignore_case=ignore_case) == len(
                raw.grep(pattern, start, end, None, ignore_case=ignore_case)[0])
    patterns = [n["n256"], n["n16"], n["abab"]]
    for start, end, limit in ((first, t1_end, None), (CUT - 1, t1_end, 4), (second, None, None)):
        matches = sorted(p for pattern in patterns for p in raw.find_all(pattern, start, end, ignore_case))
        numbers = sorted({raw.line_of(p) for p in matches})[:limit]
        got_numbers, lines = f.grep_any(patterns, start, end, limit, ignore_case=ignore_case)
        assert list(got_numbers) == numbers
        assert lines == [raw.slice(a, b) for a, b in raw.line_ranges([(k, 1) for k in numbers])]
    k = raw.line_of(CUT)
    assert k in f.grep(n["n256"], first, t1_end, ignore_case=ignore_case)[0]


# The line queries of the reader.  A whole-file call is one pass over all 129 blocks (at parallelization 1 one launch per
# block: about 2 s); every test makes at most two of them per reader and addresses line ranges otherwise.

REGEX_CASES = ("caret", "dollar", "across", "t2-only", "ascii-tail", "carried")


@pytest.mark.parametrize("name", REGEX_CASES)
def test_reader_regex(far, reader, name):
    """count_matching_lines_regex, exact and folded: two passes.  `carried` has X in T0 and Y in T1 of one line under
    another delimiter: "X was seen" must survive every launch in between."""
    f, mode = reader
    pattern, newline = bigfiles.FAR_CARRIED if name == "carried" else (bigfiles.FAR_PATTERNS[name], b"\n")
    for ignore_case in (False, True):
        want = far.raw.regex_lines(pattern, newline, ignore_case)
        assert len(want) >= 1
        assert f.count_matching_lines_regex(pattern, newline, ignore_case=ignore_case) == len(want), (name, ignore_case)


def test_reader_grep_regex(far, reader):
    """grep_regex returns lines, so the pattern is one whose matching lines are all short: once with a limit that is
    reached above 2^32, once folded and without one -- the last lines then lie in T2, whose launches start above 2^32, so the
    witnesses of those launches are moved to file offsets that do not fit 32 bits before they are ranked."""
    f, mode = reader
    raw = far.raw
    bounds = raw.line_bounds()
    pattern = bigfiles.FAR_PATTERNS["short"]
    for ignore_case in (False, True):
        want = raw.regex_lines(pattern, b"\n", ignore_case)
        assert all(bounds[k][1] - bounds[k][0] < 1000 for k in want)
        lower = sum(1 for k in want if bounds[k][1] < CUT)
        in_t2 = sum(1 for k in want if bounds[k][0] > far.t2_at)
        assert lower >= 3 and in_t2 >= 3 and len(want) > lower + 2 + in_t2
        limit = None if ignore_case else lower + 2
        numbers, lines = f.grep_regex(pattern, limit, ignore_case=ignore_case)
        assert numbers.dtype == np.uint64 and numbers.tolist() == want[:limit]
        assert lines == [raw.slice(bounds[k][0], bounds[k][1] + 1) for k in want[:limit]]
        assert bounds[int(numbers[-1])][1] > (far.t2_at if ignore_case else CUT)


def line_windows(far):
    """(first, count) around the line across 2^32, in T2 and clipped at the end; none holds a line with a filler."""
    raw = far.raw
    n, k, t2_line = len(raw.line_bounds()), raw.line_of(CUT), raw.line_of(far.t2_at)
    windows = [(k - 2, 5), (k, 1), (k + 1, 300), (t2_line + 1, 40), (t2_line + 3_000, 2_000), (n - 3, 10), (n, 4), (k - 700, 701)]
    t1_line = raw.line_of(far.t1_at)
    assert all(not first <= line < first + count for first, count in windows for line in (t1_line, t2_line))
    return windows


def test_reader_line_hashes(far, reader):
    f, mode = reader
    raw = far.raw
    for seed in (0, 1):
        want = raw.line_hashes(b"\n", seed)
        got = f.line_hashes(seed=seed)                       # the one whole-file pass of this seed
        assert got.dtype == np.uint64 and got.tolist() == want
        for first, count in line_windows(far):
            assert f.line_hashes(first, count, seed=seed).tolist() == want[first:first + count], (first, count, seed)
    t1_line = raw.line_of(far.t1_at)
    a, b = raw.line_bounds()[t1_line]
    assert b - a > CUT - (1 << 21) and int(got[t1_line]) == raw.part(a, b, bigfiles.linehash.base(1))[0]      # the closed form


def test_reader_distinct_lines(far, reader):
    f, mode = reader
    raw = far.raw
    assert f.count_distinct_lines() == len(raw.first_occurrences(b"\n", 0)) == 26_130
    got = f.first_occurrences(seed=1)
    want = raw.first_occurrences(b"\n", 1)
    assert got.dtype == np.uint64 and got.tolist() == want
    t2_line = raw.line_of(far.t2_at)
    assert [k for k in want if k >= t2_line] == [t2_line]            # T2 repeats T0: only its first line is new


def test_reader_fields(far, reader):
    f, mode = reader
    raw = far.raw
    k, t1_line = raw.line_of(CUT), raw.line_of(far.t1_at)
    for field in (0, 3):                                             # the two whole-file passes
        want = raw.field_spans(field, b" ")
        starts, sizes = f.field_spans(field, delimiter=b" ")
        assert starts.dtype == np.uint64 and sizes.dtype == np.int64
        assert list(zip(starts.tolist(), sizes.tolist())) == want, field
    assert far.t1_at < want[t1_line][0] < CUT                        # field 3 of the line with the 94 fillers lies in T1
    want = raw.field_spans(0, b" ")
    starts, sizes = f.field_spans(0, t1_line, 1, delimiter=b" ")
    assert (int(starts[0]), int(sizes[0])) == want[t1_line] == (len(far.t0), 4_293_517_388)
    # field 0 starts where its line starts
    asked = [0, 1, k - 1, k, k + 1, len(want) - 1]
    starts, _ = f.field_spans(0, k - 1, 3, delimiter=b" ")
    assert starts.tolist() == f.line_starts([k - 1, k, k + 1]).tolist() == [raw.line_bounds()[i][0] for i in (k - 1, k, k + 1)]
    assert f.line_starts(asked).tolist() == [want[i][0] for i in asked]
    for field in (3, 4, 8, 9, 1023):
        want = raw.field_spans(field, b" ")
        for first, count in line_windows(far):
            starts, sizes = f.field_spans(field, first, count, delimiter=b" ")
            assert list(zip(starts.tolist(), sizes.tolist())) == want[first:first + count], (field, first, count)
            if field in (3, 4, 9) and count <= 300:
                values = [None if n < 0 else raw.slice(s, s + n) for s, n in want[first:first + count]]
                assert f.read_fields(field, first, count, delimiter=b" ") == values, (field, first, count)
    assert f.read_fields(4, k, 1, delimiter=b" ") == [b"." + bigfiles.needles()["n256"]]            # across 2^32
    want = raw.field_spans(1, b"e")
    for first, count in line_windows(far)[:4]:
        starts, sizes = f.field_spans(1, first, count, delimiter=b"e")
        assert list(zip(starts.tolist(), sizes.tolist())) == want[first:first + count], (first, count)


@pytest.mark.parametrize("seed", [0, 1])
def test_reader_field_hashes(far, reader, seed):
    f, mode = reader
    raw = far.raw
    for field in (0, 3):                                             # the two whole-file passes
        want = raw.field_keys(field, b" ", b"\n", seed)
        got = f.field_hashes(field, delimiter=b" ", seed=seed)
        assert got.dtype == np.uint64 and got.tolist() == want, (field, seed)
    for field in (4, 8, 9, 1023):
        want = raw.field_keys(field, b" ", b"\n", seed)
        for first, count in line_windows(far):
            assert f.field_hashes(field, first, count, delimiter=b" ", seed=seed).tolist() == want[first:first + count], (field, first)
    k = raw.line_of(CUT)
    assert int(f.field_hashes(4, k, 1, delimiter=b" ", seed=seed)[0]) == bigfiles.linehash.line_hash(b"." + bigfiles.needles()["n256"], seed)
    assert int(f.field_hashes(9, k, 1, delimiter=b" ", seed=seed)[0]) == bigfiles.fieldhash.MISSING


def test_reader_field_groups(far, reader):
    f, mode = reader
    raw = far.raw
    k, t2_line = raw.line_of(CUT), raw.line_of(far.t2_at)
    lines, counts, missing, spans = raw.field_groups(3, b" ")
    got = f.count_by_field(3, delimiter=b" ")                        # one whole-file pass
    assert got[0].dtype == got[1].dtype == np.uint64
    assert (got[0].tolist(), got[1].tolist(), got[2]) == (lines, counts, missing)
    assert any(start > CUT for start, _ in spans) and sum(counts) + missing == 39_214
    for field, first, count, seed in ((4, k - 700, 1_400, 0), (0, t2_line + 1, 5_000, 1), (9, k - 5, 10, 0), (3, 39_000, 1_000, 1)):
        lines, counts, missing, spans = raw.field_groups(field, b" ", b"\n", seed, first, count)
        got = f.count_by_field(field, first, count, delimiter=b" ", seed=seed)
        assert (got[0].tolist(), got[1].tolist(), got[2]) == (lines, counts, missing), (field, first, count)
        # value_counts fetches the chosen groups' values: none of them is the field of 4.3 GB
        assert all(size < 1000 for _, size in spans)
        ranked = raw.value_counts(field, None, b" ", b"\n", seed, first, count)
        assert f.value_counts(field, 7, first, count, delimiter=b" ", seed=seed) == ranked[:7], (field, first, count)
        assert f.value_counts(field, None, first, count, delimiter=b" ", seed=seed) == ranked
    ranked = raw.value_counts(4, 3, b" ", b"\n", 0, k - 700, 1_400)
    assert len(ranked) == 3 and (b"." + bigfiles.needles()["n256"], 1) in raw.value_counts(4, None, b" ", b"\n", 0, k - 700, 1_400)


def test_reader_columns_numbers_and_selections(far, reader):
    """read_columns, field_ints, where_field / select_lines / count_where_field and sum_by_field around 2^32 and in T2, whose
    file offsets all lie above it, against VirtualRaw.field_values.  The field across 2^32 under b" " is b"." + n256, 257
    bytes, one more than a value of where_field may have: it comes back from read_columns and is refused as a value, and
    the selection takes the piece of it that b"k" delimits, 20 bytes from 2^32 - 1 on.  One whole-file pass
    (count_where_field); 5.2 - 5.9 s at parallelization 1 and 2.0 s at 4 on an MI355X."""
    import fieldnum
    f, mode = reader
    raw = far.raw
    n256 = bigfiles.needles()["n256"]
    k, t2_line = raw.line_of(CUT), raw.line_of(far.t2_at)
    bounds = raw.line_bounds()
    for first, count in line_windows(far):
        want = [raw.field_values(j, b" ", b"\n", first, count) for j in (4, 9, 0)]
        assert f.read_columns([4, 9, 0], first, count, delimiter=b" ") == want, (first, count)
        for j in (0, 9):
            got = f.field_ints(j, first, count, delimiter=b" ")
            assert got.dtype == np.int64 and got.tolist() == [fieldnum.word(v) for v in raw.field_values(j, b" ", b"\n", first, count)], (j, first, count)
    assert f.read_columns([4], k, 1, delimiter=b" ") == [[b"." + n256]]                             # across 2^32
    assert any(start > CUT for start, _ in raw.field_spans(4, b" ")[t2_line + 1:t2_line + 41])
    with pytest.raises(ValueError):
        f.where_field(4, values=[b"." + n256], first=k - 700, count=1_400, delimiter=b" ")
    # the field of line k that holds byte 2^32 under the delimiter b"k"
    j, (start, size) = next((j, span) for j, span in ((j, raw.field_spans(j, b"k")[k]) for j in range(12)) if span[0] <= CUT < span[0] + span[1])
    value = raw.slice(start, start + size)
    assert start < CUT < start + size <= start + 256 and value in n256 and raw.field_values(j, b"k", b"\n", k, 1) == [value]
    window = raw.field_values(j, b"k", b"\n", k - 700, 1_400)
    assert [k - 700 + i for i, v in enumerate(window) if v == value] == [k]
    got = f.where_field(j, values=[value], first=k - 700, count=1_400, delimiter=b"k")
    assert got.dtype == np.uint64 and got.tolist() == [k]
    numbers, lines = f.select_lines(j, values=[value, b"never"], first=k - 700, count=1_400, delimiter=b"k")
    assert numbers.tolist() == [k] and lines == [raw.slice(bounds[k][0], bounds[k][1] + 1)]
    assert f.where_field(j, values=[value], invert=True, first=k - 2, count=5, delimiter=b"k").tolist() == [k - 2, k - 1, k + 1, k + 2]
    assert f.count_where_field(j, values=[value], invert=True, first=k - 2, count=5, delimiter=b"k") == 4
    # five values of T2's lines, counted over the whole file in one pass: from the groups and their spans, so that the field
    # of 4.3 GB is never sliced
    values = []
    for v in raw.field_values(3, b" ", b"\n", t2_line + 1, 400):
        if v is not None and v not in values and len(values) < 5:
            values.append(v)
    lines, counts, missing, spans = raw.field_groups(3, b" ")
    want = sum(count for count, (start, size) in zip(counts, spans) if 0 <= size <= 256 and raw.slice(start, start + size) in values)
    assert len(values) == 5 and want > 100
    assert f.count_where_field(3, values=values, delimiter=b" ") == want
    # sums per key in T2
    first, count = t2_line + 1, 5_000
    lines, counts, missing, _ = raw.field_groups(3, b" ", b"\n", 0, first, count)
    keys = raw.field_values(3, b" ", b"\n", first, count)
    words = [fieldnum.word(v) for v in raw.field_values(0, b" ", b"\n", first, count)]
    groups = {}
    for key, word in zip(keys, words):
        if key is not None:
            g = groups.setdefault(key, {"numbers": 0, "sum": 0, "min": fieldnum.NOT_A_NUMBER, "max": fieldnum.NOT_A_NUMBER})
            if word not in (fieldnum.NOT_A_NUMBER, fieldnum.MISSING):
                g["min"] = word if g["numbers"] == 0 else min(g["min"], word)
                g["max"] = word if g["numbers"] == 0 else max(g["max"], word)
                g["numbers"] += 1
                g["sum"] += word
    got = f.sum_by_field(3, 0, first, count, delimiter=b" ")
    assert (got[0].tolist(), got[1].tolist(), got[6]) == (lines, counts, missing) and len(lines) == len(groups) > 100
    ordered = [groups[keys[line - first]] for line in lines]
    assert got[2].tolist() == [g["numbers"] for g in ordered] and got[3] == [g["sum"] for g in ordered]
    assert got[4].tolist() == [g["min"] for g in ordered] and got[5].tolist() == [g["max"] for g in ordered]


def test_reader_one_line_of_more_than_4_gib(native, far, far_path):
    """Under a delimiter that is in no text the whole file is one unterminated line of more than 2^32 bytes: its hash is
    composed on the host from every launch's (h, x^len), its field 0 has a size above 2^32 and the same key."""
    raw = far.raw
    with native.open(far_path, parallelization=4) as f:
        f.set_block_offsets(far.map)
        for seed in (0, 1):
            whole = raw.part(0, raw.size, bigfiles.linehash.base(seed))[0]
            assert f.line_hashes(newline=b"\0", seed=seed).tolist() == [whole] == raw.line_hashes(b"\0", seed)
            assert f.field_hashes(0, delimiter=b"\t", newline=b"\0", seed=seed).tolist() == [whole]
        starts, sizes = f.field_spans(0, delimiter=b"\t", newline=b"\0")
        assert (starts.tolist(), sizes.tolist()) == ([0], [raw.size]) and raw.size > CUT
        starts, sizes = f.field_spans(1, delimiter=b" ", newline=b"\0")
        assert list(zip(starts.tolist(), sizes.tolist())) == raw.field_spans(1, b" ", b"\0")
        assert f.count_matching_lines_regex(bigfiles.FAR_PATTERNS["t2-only"], b"\0") == 1
        assert f.count_matching_lines_regex(bigfiles.FAR_PATTERNS["nowhere"], b"\0") == 0


DEVICE_CHILD = r"""
import pickle, sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import numpy as np
import indexed_bzip2_amd as m

with open(sys.argv[3], "rb") as f:
    case = pickle.load(f)
free_before, total_memory = torch.cuda.mem_get_info()
with m.open(sys.argv[2], parallelization=4) as f:
    f.set_block_offsets(case["map"])
    offsets, sizes = [o for o, _ in case["ranges"]], [s for _, s in case["ranges"]]
    for dm in (0, 3):
        dev = torch.full((sum(sizes) + 3,), 0xCD, dtype=torch.uint8, device="cuda")
        counts = f.read_ranges_into(offsets, sizes, dev[dm:])
        assert list(counts) == [len(w) for w in case["range_bytes"]]
        got = bytes(dev.cpu().numpy())
        at = dm
        for size, want in zip(sizes, case["range_bytes"]):
            assert got[at:at + len(want)] == want and got[at + len(want):at + size] == b"\xcd" * (size - len(want))
            at += size
    for ignore_case, (start, end, numbers, lines) in case["grep"].items():
        got_numbers, data, bounds = f.grep_to_tensor(case["pattern"], start, end, ignore_case=ignore_case)
        assert list(got_numbers) == numbers and data.is_cuda
        host = bytes(data.cpu().numpy())
        assert [host[int(bounds[i]):int(bounds[i + 1])] for i in range(len(numbers))] == lines
    free_after, _ = torch.cuda.mem_get_info()
    print("held on the device with the reader open:", (free_before - free_after) >> 20, "MiB")
print("device destinations ok")
"""


def test_device_destinations(far, far_path, tmp_path):
    """read_ranges_into a device tensor and grep_to_tensor, in a process that starts torch first; the expected bytes come
    from this process."""
    import pickle
    import sys
    raw, n = far.raw, bigfiles.needles()
    ranges = seeded_ranges(far, seed=0xDE7, count=30)
    newlines = raw.newline_offsets()
    first = int(newlines[newlines > far.t1_at][0]) + 1
    grep = {}
    for ignore_case in (False, True):
        end = far.t1_at + len(far.t1)
        numbers, line_ranges = raw.grep(n["n256"], first, end, None, ignore_case=ignore_case)
        assert raw.line_of(CUT) in numbers and all(b - a < 100_000 for a, b in line_ranges)
        grep[ignore_case] = (first, end, numbers, [raw.slice(a, b) for a, b in line_ranges])
    case = {"map": far.map, "ranges": ranges, "range_bytes": [raw.slice(o, o + s) for o, s in ranges], "pattern": n["n256"],
            "grep": grep}
    (tmp_path / "case.pickle").write_bytes(pickle.dumps(case))
    run = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT, far_path, str(tmp_path / "case.pickle")],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "device destinations ok" in run.stdout
    print("\n" + run.stdout.strip())


QUERY_CHILD = r"""
import pickle, sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import indexed_bzip2_amd as m

with open(sys.argv[3], "rb") as f:
    case = pickle.load(f)
with m.open(sys.argv[2], parallelization=4) as f:
    f.set_block_offsets(case["map"])
    pattern, limit, numbers, lines = case["grep_regex"]
    got_numbers, data, bounds = f.grep_regex_to_tensor(pattern, limit)
    assert got_numbers.tolist() == numbers and data.is_cuda and data.dtype == torch.uint8
    host = bytes(data.cpu().numpy())
    assert [host[int(bounds[i]):int(bounds[i + 1])] for i in range(len(numbers))] == lines
    for first, count, seed, want in case["line_hashes"]:
        got = f.line_hashes_to_tensor(first, count, seed=seed)
        assert got.is_cuda and got.dtype == torch.int64 and got.tolist() == want, (first, count, seed)
    for field, first, count, seed, spans, keys, values in case["fields"]:
        starts, sizes = f.field_spans_to_tensor(field, first, count, delimiter=b" ")
        assert starts.is_cuda and sizes.is_cuda and starts.dtype == sizes.dtype == torch.int64
        assert list(zip(starts.tolist(), sizes.tolist())) == spans, (field, first, count)
        got = f.field_hashes_to_tensor(field, first, count, delimiter=b" ", seed=seed)
        assert got.is_cuda and got.dtype == torch.int64 and got.tolist() == keys, (field, first, count, seed)
        if values is not None:
            data, bounds = f.read_fields_to_tensor(field, first, count, delimiter=b" ")
            host = bytes(data.cpu().numpy())
            assert data.is_cuda and [host[int(bounds[i]):int(bounds[i + 1])] for i in range(len(values))] == values, (field, first)
print("query destinations ok")
"""


def test_query_device_destinations(far, far_path, tmp_path):
    """grep_regex_to_tensor, line_hashes_to_tensor, field_spans_to_tensor, read_fields_to_tensor and
    field_hashes_to_tensor at parallelization 4 with the imported map, in a process that starts torch first; the
    expected values are computed here, from VirtualRaw."""
    import pickle
    import sys
    raw = far.raw
    bounds = raw.line_bounds()
    k = raw.line_of(CUT)
    pattern = bigfiles.FAR_PATTERNS["short"]
    matching = raw.regex_lines(pattern)
    limit = sum(1 for n in matching if bounds[n][1] < CUT) + 2
    assert len(matching) > limit and all(bounds[n][1] - bounds[n][0] < 1000 for n in matching)
    case = {"map": far.map,
            "grep_regex": (pattern, limit, matching[:limit], [raw.slice(bounds[n][0], bounds[n][1] + 1) for n in matching[:limit]]),
            "line_hashes": [(0, None, 1, raw.line_hashes(b"\n", 1))], "fields": []}
    for first, count in line_windows(far):
        case["line_hashes"].append((first, count, 0, raw.line_hashes(b"\n", 0)[first:first + count]))
    for field, first, count, seed in ((0, 0, None, 0), (3, 0, None, 1), (4, k - 2, 5, 1), (9, k - 2, 5, 0), (4, k + 1, 300, 0)):
        spans, keys = raw.field_spans(field, b" "), raw.field_keys(field, b" ", b"\n", seed)
        last = len(spans) if count is None else first + count
        values = None if count is None else [b"" if n < 0 else raw.slice(s, s + n) for s, n in spans[first:last]]     # a missing field has size 0
        case["fields"].append((field, first, count, seed, spans[first:last], keys[first:last], values))
    (tmp_path / "case.pickle").write_bytes(pickle.dumps(case))
    run = subprocess.run([sys.executable, "-c", QUERY_CHILD, ROOT, far_path, str(tmp_path / "case.pickle")],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "query destinations ok" in run.stdout


def tool_queries_on_far(far, far_path):
    """--grep-regex, --count-distinct-lines and --count-by-field: one pass over the file each."""
    raw = far.raw
    bounds = raw.line_bounds()
    pattern = bigfiles.FAR_PATTERNS["short"]
    matching = raw.regex_lines(pattern)
    assert all(bounds[n][1] - bounds[n][0] < 1000 for n in matching) and bounds[matching[-1]][0] > CUT
    run = subprocess.run([CLI, "-P", "4", "--grep-regex", pattern.decode(), "--line-number", far_path], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"".join(b"%d:" % (n + 1) + raw.slice(bounds[n][0], bounds[n][1] + 1) for n in matching)
    run = subprocess.run([CLI, "-P", "4", "--count-distinct-lines", far_path], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b"%d\n" % len(raw.first_occurrences()), run.stderr[-2000:]
    lines, counts, missing, spans = raw.field_groups(3, b" ")
    assert all(size < 1000 for _, size in spans)                     # the tool prints the values
    run = subprocess.run([CLI, "-P", "4", "--count-by-field", "3", "--field-delimiter", " ", far_path], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"".join(b"%d\t%s\n" % (count, value) for value, count in raw.value_counts(3, None, b" "))


def test_tool_on_far(far, far_path, tmp_path):
    raw, n = far.raw, bigfiles.needles()
    newlines = raw.newline_offsets()
    run = subprocess.run([CLI, "-P", "4", "--count-lines", far_path], capture_output=True, timeout=600)
    assert run.returncode == 0 and int(run.stdout) == len(newlines), run.stderr[-2000:]
    # a needle whose every line is short (none lies in the first line of T1 or T2, which the fillers belong to)
    pattern = n["n17"]
    matches = raw.find_all(pattern)
    assert matches == short_lines(far, matches) and any(p > CUT for p in matches)
    numbers, ranges = raw.grep(pattern)
    run = subprocess.run([CLI, "-P", "4", "--grep", pattern.decode(), "--line-number", far_path], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == b"".join(str(k + 1).encode() + b":" + raw.slice(a, b) for k, (a, b) in zip(numbers, ranges))
    listing = tmp_path / "offsets.txt"
    run = subprocess.run([CLI, "-P", "4", "-L", str(listing), "--", far_path], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stdout == b"", run.stderr[-2000:]
    pairs = [tuple(int(x) for x in line.split(",")) for line in listing.read_text().split()]
    assert dict(pairs) == far.map and pairs == sorted(pairs)
    # -t acts on a decode (-d or -L; by itself it is no mode, as in the reference): the magics and every stream CRC
    tested = tmp_path / "tested.txt"
    run = subprocess.run([CLI, "-P", "4", "-t", "-L", str(tested), "--", far_path], capture_output=True, timeout=600)
    assert run.returncode == 0 and tested.read_text() == listing.read_text(), run.stderr[-2000:]
    damaged = bytearray(far.enc)
    damaged[far.blocks[-3][0] // 8 + 20] ^= 0x10                          # inside a block that decodes above 2^32
    (tmp_path / "damaged.bz2").write_bytes(bytes(damaged))
    run = subprocess.run([CLI, "-P", "4", "-t", "-L", str(tmp_path / "damaged.txt"), "--", str(tmp_path / "damaged.bz2")],
                         capture_output=True, timeout=600)
    assert run.returncode != 0
    tool_queries_on_far(far, far_path)


# ------------------------------------------------------------------- C. deep_file(): bit offsets of 2^32 and more

DEEP_NEAR = CUT - (1 << 26)


def check_deep_blocks(deep, dec, offsets):
    """Records and payload of the blocks at `offsets` of the resident deep file: sizes in bits exact, every CRC right (the
    output offsets are small here, so a CRC says what it seems to), the first and last bytes of every block, the block
    that straddles bit 2^32 and the texts whole."""
    results, total = dec.decode_batch(offsets)
    following = sorted(deep.map)
    known = {bit: (at, size) for bit, at, size, _ in deep.blocks}
    assert total == sum(known[bit][1] for bit in offsets)
    at_output = 0
    for bit, r in zip(offsets, results):
        at, size = known[bit]
        end_bits = following[following.index(bit) + 1]                   # the next magic: a block's, or the end of stream's
        assert r["status"] == 0 and r["computed_crc"] == r["header_crc"], bit
        assert r["encoded_offset_bits"] == bit and r["encoded_size_bits"] == end_bits - bit, bit
        assert r["decoded_size"] == size and r["data_offset"] == at_output, bit
        whole = bit in deep.straddling or at >= deep.prefix_decoded
        for a, b in [(0, size)] if whole else [(0, min(size, 4096)), (max(0, size - 4096), size)]:
            assert dec.copy_output(at_output + a, b - a) == bigfiles.deep_slice(deep, at + a, at + b), (bit, a, b)
        at_output += size
    return results


@pytest.fixture(scope="module")
def deep_decoder(native, deep):
    dec = native.Decoder(device=0, max_batch_blocks=1)
    began = time.time()
    dec.set_input(deep.enc)
    print(f"\ndeep file: {len(deep.enc)} bytes resident after {time.time() - began:.2f} s")
    yield dec
    dec.close()


def test_magic_scan_deep(native, deep, deep_decoder):
    blocks = [bit for bit, _, _, _ in deep.blocks]
    straddling = deep.straddling[0]
    assert straddling < CUT < blocks[blocks.index(straddling) + 1] and blocks[-1] > CUT + (1 << 26)
    assert deep_decoder.find_magic() == blocks
    assert deep_decoder.find_magic(native._native.MAGIC_EOS) == deep.eos
    for threads in (1, 8):
        assert native.find_magic(deep.enc, threads=threads) == blocks
        assert native.find_magic(deep.enc, native._native.MAGIC_EOS, threads=threads) == deep.eos


@pytest.mark.parametrize("variant", ["default", "scan-1", "spec-4", "spec-8"])
def test_blocks_above_bit_2_32(native, deep, deep_decoder, variant, monkeypatch):
    """The blocks from 2^26 bits below 2^32 on -- the straddling one among them -- under the Huffman scan a batch of this
    size selects, under k_hscan<1> and under k_hscan_spec<4> and <8>."""
    offsets = [bit for bit, _, _, _ in deep.blocks if bit >= DEEP_NEAR]
    assert deep.straddling[0] in offsets and sum(1 for bit in offsets if bit < CUT) >= 5
    assert sum(1 for bit in offsets if bit > CUT) >= 15
    if variant == "default":
        began = time.time()
        check_deep_blocks(deep, deep_decoder, offsets)
        print(f"\ndeep blocks, default scan: {time.time() - began:.2f} s with the checks; batch {deep_decoder.timings()['ms_total']:.1f} ms; "
              f"device memory {deep_decoder.device_memory()}")
        return
    monkeypatch.setenv("MI355X_BZ2_SCAN_WAVES", variant.split("-")[1])
    dec = native.Decoder(device=0, max_batch_blocks=1)
    try:
        dec.share_input(deep_decoder)
        began = time.time()
        check_deep_blocks(deep, dec, offsets)
        print(f"\ndeep blocks, {variant}: {time.time() - began:.2f} s with the checks; batch {dec.timings()['ms_total']:.1f} ms; "
              f"device memory {dec.device_memory()}")
    finally:
        dec.close()


@pytest.fixture(scope="module")
def deep_path(deep, tmp_path_factory):
    path = tmp_path_factory.mktemp("deep") / "deep.bz2"
    path.write_bytes(deep.enc)
    return str(path)


def check_deep_tail(deep, f):
    """Ranges, matches and lines in the texts behind the prefix, whose blocks all lie above bit 2^32."""
    tail, base, n = deep.tail, deep.prefix_decoded, bigfiles.needles()
    ranges = [(base - 500, 1000), (base + 100_000, 70_000), (deep.size - 100, 500), (base, 0), (base + 299_990, 20)]
    assert f.read_ranges(ranges) == [bigfiles.deep_slice(deep, o, o + s) for o, s in ranges]
    for ignore_case in (False, True):
        want = [base + p for p in tail.find_all(n["n256"], ignore_case=ignore_case)]
        assert len(want) >= 8 and list(f.find_all(n["n256"], base, None, ignore_case=ignore_case)) == want
        assert f.count_matches(n["n16"], base + 5, None, ignore_case=ignore_case) == len(tail.find_all(n["n16"], 5, None, ignore_case))
    # the prefix holds no newline: line k of the file is line k of the texts, but for line 0, which starts in the prefix.
    # The line index is imported (arithmetic again): building it would decode the whole prefix
    index = {at: tail.line_of(at - base) if at > base else 0 for _, at, _, _ in deep.blocks}
    index[deep.size] = len(tail.newline_offsets())
    f.set_line_offsets(index)
    lines = [(3, 2), (1000, 1), (len(tail.newline_offsets()) - 1, 5)]
    assert f.read_line_ranges(lines) == [tail.slice(a, b) for a, b in tail.line_ranges(lines)]
    assert list(f.line_starts([1, 7])) == [base + int(s) for s in tail.line_starts()[[1, 7]]]


def test_reader_on_deep_file(native, deep, deep_path):
    began = time.time()
    with native.open(deep_path, parallelization=4) as f:
        f.seek(deep.prefix_decoded - 1000)
        assert f.read(3000) == bigfiles.deep_slice(deep, deep.prefix_decoded - 1000, deep.prefix_decoded + 2000)
        available = f.available_block_offsets()                      # after a partial read: a prefix of the map
        assert available and all(deep.map[bit] == at for bit, at in available.items())
        assert max(available) > CUT
        # (the buffered reader reads ahead by up to 1 MiB: tell_compressed() speaks of the position underneath)
        assert f.tell_compressed() == max(bit for bit, at, _, _ in deep.blocks if at <= f.bz2reader.tell()) > CUT
        assert f.block_offsets() == deep.map and f.size() == deep.size
        print(f"\ndeep on the fly at parallelization 4: block map after {time.time() - began:.2f} s; {f.statistics()}")
        # block_offsets() has read to the end underneath the buffered reader (as the reference's does): a seek out of the
        # buffer first, so that the next one reaches the reader
        f.seek(0)
        f.seek(deep.prefix_decoded)
        assert f.read() == deep.tail.slice(0, deep.tail.size)
        assert f.tell_compressed() == sorted(deep.map)[-1]


@pytest.mark.parametrize("budget", [None, 1 << 20], ids=["resident", "bounded"])
def test_reader_on_deep_file_with_its_map(native, deep, deep_path, budget, monkeypatch):
    """With the arithmetic map; once more with bounded residency, where every launch packs the bytes of its own blocks, which
    here start at word offsets above 2^27."""
    if budget is not None:
        monkeypatch.setenv("MI355X_BZ2_INPUT_BUDGET", str(budget))
    with native.open(deep_path, parallelization=4) as f:
        f.set_block_offsets(deep.map)
        before = f.statistics()
        check_deep_tail(deep, f)
        f.seek(deep.prefix_decoded + 150_000)
        assert f.read(100) == deep.tail.slice(150_000, 150_100)
        assert f.tell_compressed() == max(bit for bit, at, _, _ in deep.blocks if at <= f.bz2reader.tell()) > CUT
        # the block that straddles bit 2^32
        bit = deep.straddling[0]
        at, size = next((at, size) for b, at, size, _ in deep.blocks if b == bit)
        assert f.read_ranges([(at + 17, 5000), (at + size - 100, 200)]) == [bigfiles.deep_slice(deep, at + 17, at + 5017),
                                                                            bigfiles.deep_slice(deep, at + size - 100, at + size + 100)]
        after = f.statistics()
        print(f"\ndeep with its map ({'resident' if budget is None else 'bounded'}): "
              f"{after['input_bytes_uploaded'] - before['input_bytes_uploaded']} bytes uploaded, "
              f"{after['blocks_decoded'] - before['blocks_decoded']} blocks decoded in {after['batches'] - before['batches']} launches")
        assert after["input_resident"] == (1 if budget is None else 0)
        if budget is not None:
            assert 0 < after["input_bytes_uploaded"] - before["input_bytes_uploaded"] < len(deep.enc) // 20
        assert after["blocks_decoded"] - before["blocks_decoded"] < 200


def test_decompress_buffers_beyond_4_gib(native, far):
    """[far, small, far] in one call: the third buffer's output offset lies above 2^32, and so do all its bytes."""
    import bz2
    small_raw = b"between the two\n" * 1000
    small = bz2.compress(small_raw, 9)
    dec = native.Decoder(device=0, max_batch_blocks=1)
    try:
        began = time.time()
        results, total = dec.decompress_buffers([far.enc, small, far.enc], max_launch_blocks=len(far.blocks))
        print(f"\ndecompress_buffers of {total} bytes: {time.time() - began:.2f} s; device memory {dec.device_memory()}")
        size = far.raw.size
        assert total == 2 * size + len(small_raw)
        assert [r["status"] for r in results] == [0, 0, 0]
        assert [r["output_offset"] for r in results] == [0, size, size + len(small_raw)]
        assert [r["decoded_size"] for r in results] == [size, len(small_raw), size]
        assert [r["n_streams"] for r in results] == [len(far.streams), 1, len(far.streams)]
        assert [r["n_blocks"] for r in results] == [len(far.blocks), 1, len(far.blocks)]
        third = results[2]["output_offset"]
        assert third > CUT
        assert dec.copy_output(size, len(small_raw)) == small_raw
        assert dec.copy_output(third + far.t2_at, len(far.t0)) == far.t0
        # and on the device: T2 of the third buffer from its first 16-byte aligned byte on (the allocation is aligned)
        skip = -(third + far.t2_at) % 16
        assert dec.output_device_ptr() % 16 == 0
        assert dec.crc32_device(dec.output_device_ptr() + third + far.t2_at + skip, [len(far.t0) - skip]) == [plain_crc(far.t0[skip:])]
        n = bigfiles.needles()
        for pattern in (n["n256"], n["n2"]):
            positions, counts = dec.find_bytes(pattern, [(third + far.t2_at, len(far.t0))])
            assert [p - third - far.t2_at for p in positions] == far.raw.find_all(pattern, 0, len(far.t0)) and counts[0] > 0
        assert dec.copy_output(third + far.t1_at, len(far.t1)) == far.t1
        assert dec.copy_output(CUT - 70_000, 140_000) == far.raw.slice(CUT - 70_000, CUT + 70_000)
        # the third buffer's fillers, counted where they lie
        fillers = [(third + at, n, value) for _, at, n, value in far.blocks if value is not None]
        for value in sorted({value for _, _, value in fillers}):
            spans = [(at, n) for at, n, v in fillers if v == value]
            assert dec.count_byte(value, spans) == [n for _, n in spans]
        memory = dec.device_memory()
        assert memory["scratch_bytes"] + memory["output_bytes"] < 32 << 30
    finally:
        dec.close()
