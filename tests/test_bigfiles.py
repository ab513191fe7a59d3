"""tests/bigfiles.py on the CPU: VirtualRaw against the same parts held in memory, crc_concat against the oracle's CRC, and
the two builders against CPython's bz2 decoder and the oracle's block map -- at full scale where that takes seconds
(far_file's promises, the streams around 2^32), at a shrunken scale where it would not (the whole block map).

VirtualRaw's answers for the line queries (line hashes, field spans and keys, groups, span summaries, regular expressions)
are checked on shrunken layouts whose bytes fit in memory, against linehash.py, fields.py, fieldhash.py, regexgen.py and
re; what the GPU tests rely on at full scale is asserted at full scale."""
import bz2
import time

import numpy as np

import bigfiles
import datagen


def lines_of(raw, newline=b"\n"):
    pieces = raw.split(newline)
    return [piece + newline for piece in pieces[:-1]] + [pieces[-1]]


def plain_find_all(raw, pattern, start, end, ignore_case):
    if ignore_case:
        raw, pattern = raw.lower(), pattern.lower()
    end = min(end, len(raw))
    found, p = [], raw.find(pattern, start, end)
    while p != -1:
        found.append(p)
        p = raw.find(pattern, p + 1, end)
    return found


def test_virtual_raw_agrees_with_bytes():
    """Runs of 1 000 bytes instead of 45 MB, texts of 5 000 bytes: every method against plain loops over the bytes.  CUT
    plays 2^32's role: it lies inside the 256-byte needle of the second text."""
    n = bigfiles.needles()
    t0 = bigfiles.make_text(5000, 1)
    t1 = bigfiles.make_text(5000, 2, cut=2500)
    parts = [t0, (0x81, 1000), (0x93, 1000), (0xA5, 317), t1[:2000], t1[2000:], (0xB7, 1000), t0]
    virtual = bigfiles.VirtualRaw(parts)
    raw = b"".join(bytes([p[0]]) * p[1] if isinstance(p, tuple) else p for p in parts)
    cut = 5000 + 2317 + 2500
    assert virtual.size == len(raw) and raw[cut - 100:cut + 156] == n["n256"]
    assert len(virtual.literals()) == 3                      # the two halves of t1 are one part

    r = datagen.rng(0xB16)
    cuts = [0, 1, 4999, 5000, 5001, 7317, cut - 1, cut, cut + 1, len(raw) - 1, len(raw), len(raw) + 5]
    for a in cuts:
        for b in cuts:
            assert virtual.slice(a, b) == raw[a:b], (a, b)
    newlines = np.flatnonzero(np.frombuffer(raw, dtype=np.uint8) == 10)
    assert virtual.newline_offsets().dtype == np.uint64
    assert np.array_equal(virtual.newline_offsets(), newlines.astype(np.uint64))
    for offset in cuts + [int(p) for p in newlines[:3]] + [int(newlines[5]) + 1]:
        assert virtual.line_of(offset) == raw[:offset].count(b"\n"), offset
    lines = lines_of(raw)
    asked = [(0, 1), (3, 2), (len(lines) - 1, 1), (len(lines) - 2, 5), (len(lines), 1), (7, 0), (raw[:cut].count(b"\n"), 1)]
    for (first, count), (start, end) in zip(asked, virtual.line_ranges(asked)):
        assert raw[start:end] == b"".join(lines[first:first + count]), (first, count)

    planted = plain_find_all(raw, n["n256"], 0, len(raw), True)
    assert len(planted) >= 3
    ranges = [(0, len(raw)), (cut - 100, cut + 156), (cut - 100, cut + 155), (cut - 99, cut + 156), (cut, len(raw)),
              (0, cut), (cut - 1, cut + 1), (cut - 1, cut), (len(raw) - 3, 2**64), (len(raw) + 1, 2**64), (700, 600)]
    for p in planted:                                        # ranges that start and end inside needles
        ranges += [(p + int(r.integers(0, 256)), len(raw)), (0, p + int(r.integers(0, 257))), (p, p + 256)]
    for _ in range(20):
        a = int(r.integers(0, len(raw)))
        ranges.append((a, a + int(r.integers(0, 4000))))
    for name, pattern in n.items():
        for ignore_case in (False, True):
            for start, end in ranges:
                want = plain_find_all(raw, pattern, start, end, ignore_case)
                assert virtual.find_all(pattern, start, end, ignore_case) == want, (name, ignore_case, start, end)
            numbers, found = virtual.grep(pattern, 0, None, None, ignore_case=ignore_case)
            want = sorted({raw[:p].count(b"\n") for p in plain_find_all(raw, pattern, 0, len(raw), ignore_case)})
            assert numbers == want and [raw[a:b] for a, b in found] == [lines[k] for k in want], name
            assert virtual.grep(pattern, cut - 50, None, 2, ignore_case=ignore_case)[0] == sorted(
                {raw[:p].count(b"\n") for p in plain_find_all(raw, pattern, cut - 50, len(raw), ignore_case)})[:2]
    assert len(virtual.find_all(b"aXa", ignore_case=True)) > len(virtual.find_all(b"aXa")) > 8      # overlapping ones


def test_virtual_raw_refuses_what_it_cannot_answer():
    virtual = bigfiles.VirtualRaw([b"abc\n", (0x81, 10), b"def"])
    for call in (lambda: virtual.find_all(b"a\x81"), lambda: virtual.newline_offsets(b"\x81"),
                 lambda: bigfiles.VirtualRaw([(0x41, 5)]), lambda: bigfiles.VirtualRaw([b"\x90"])):
        try:
            call()
        except AssertionError:
            continue
        raise AssertionError("accepted")


def test_magic_offsets_agree_with_datagen():
    enc = bz2.compress(datagen.text_like(250_000, 5), 1) + bz2.compress(b"\x81" * 5000, 9)
    assert bigfiles.magic_offsets(enc, bigfiles.MAGIC_BLOCK) == datagen._block_offsets(enc)
    assert len(bigfiles.magic_offsets(enc, bigfiles.MAGIC_EOS)) == 2


def test_crc_concat(oracle):
    data = datagen.random_bytes(70_001, 0xC4C)
    crc = lambda piece: oracle.crc32(piece) ^ 0xFFFFFFFF      # orc_crc32_update leaves the final inversion to the caller
    assert crc(b"123456789") == 0xFC891918                   # CRC-32/BZIP2's check value
    for split in (0, 1, 3, 255, 256, 257, 65_535, 65_536, 65_537, 70_000, 70_001):
        a, b = data[:split], data[split:]
        assert bigfiles.crc_concat(crc(a), crc(b), len(b)) == crc(data), split
    folded = crc(b"")
    for k in range(0, len(data), 9973):
        piece = data[k:k + 9973]
        folded = bigfiles.crc_concat(folded, crc(piece), len(piece))
    assert folded == crc(data)
    # the polynomial is primitive: x has order 2^32 - 1 exactly
    order = 2**32 - 1
    assert bigfiles.x_pow(order) == 1
    assert all(bigfiles.x_pow(order // p) != 1 for p in (3, 5, 17, 257, 65537))
    # an exponent beyond 2^32 - 1, reduced by hand: 8 (2^32 - 1 + k) = 8 k modulo the order
    k = 4099
    a, b = data[:1000], data[1000:1000 + k]
    long = 2**32 - 1 + k
    assert 8 * long > order and (8 * long) % order == 8 * k
    assert bigfiles.x_pow(8 * long) == bigfiles.x_pow(8 * k)
    assert bigfiles.crc_concat(crc(a), crc(b), long) == bigfiles.crc_concat(crc(a), crc(b), k) == crc(a + b)
    # and one that reduces to another length: 2^32 + 5 bytes shift like 2^32 + 5 - (2^32 - 1) = 6 bytes
    assert bigfiles.crc_concat(crc(a), crc(b[:6]), 2**32 + 5) == crc(a + b[:6])


def test_full_block_is_the_largest_single_block_run():
    one = bz2.compress(b"\x81" * bigfiles.FULL_BLOCK, 9)
    two = bz2.compress(b"\x81" * (bigfiles.FULL_BLOCK + 1), 9)
    assert len(bigfiles.magic_offsets(one, bigfiles.MAGIC_BLOCK)) == 1
    assert len(bigfiles.magic_offsets(two, bigfiles.MAGIC_BLOCK)) == 2


def test_far_file_keeps_its_promises(oracle):
    began = time.time()
    far = bigfiles.far_file()
    deep = bigfiles.deep_file()
    print(f"\nCPU preparation of far_file and deep_file: {time.time() - began:.1f} s "
          f"(far: {len(far.enc)} bytes for {far.raw.size}; deep: {len(deep.enc)} bytes for {deep.size})")
    enc, raw, block_map = far
    cut = 2**32
    assert raw.size > cut + 2 * bigfiles.FULL_BLOCK and raw.size <= int(4.45 * 2**30)
    assert far.t1_at < cut < far.t1_at + len(far.t1) and far.t2_at > cut + 2 * bigfiles.FULL_BLOCK
    assert raw.slice(far.t2_at, raw.size) == raw.slice(0, len(far.t0)) == far.t0
    # (the other promises are asserted by the builder: bigfiles.far_file)
    assert sorted(block_map) == sorted([b for b, _, _, _ in far.blocks] + far.eos + [8 * len(enc)])
    assert block_map[8 * len(enc)] == raw.size and len(far.blocks) > 100
    assert oracle.find_magic(enc) == [b for b, _, _, _ in far.blocks]
    assert oracle.find_magic(enc, bigfiles.MAGIC_EOS) == far.eos

    # CPython's decoder on T1's stream and its two neighbours
    index = next(i for i, (_, _, at, _) in enumerate(far.streams) if at == far.t1_at)
    for first, size, at, decoded in far.streams[index - 1:index + 2]:
        got = bz2.BZ2Decompressor().decompress(enc[first:first + size])
        assert len(got) == decoded and got == raw.slice(at, at + decoded)
    # the streams lie back to back, in the file and in the decoded bytes; the last two decode to the file's end
    at_byte = at_decoded = 0
    for first, size, at, decoded in far.streams:
        assert (first, at) == (at_byte, at_decoded)
        at_byte, at_decoded = first + size, at + decoded
    assert (at_byte, at_decoded) == (len(enc), raw.size)
    for first, size, at, decoded in far.streams[-2:]:
        assert bz2.BZ2Decompressor().decompress(enc[first:first + size]) == raw.slice(at, at + decoded)


def test_far_file_block_map_on_a_shrunken_layout(oracle):
    """The same builder with fillers of 90 000 bytes, texts of 300 000 and the cut at 2^20: small enough for the oracle."""
    far = bigfiles.far_file(cut=1 << 20, filler=90_000, text_size=300_000, tail_fillers=2)
    status, decoded, block_map, garbage = oracle.decode_file(far.enc)
    assert status == 0 and not garbage
    assert block_map == far.map
    assert len(decoded) == far.raw.size
    for a in range(0, len(decoded), 1 << 18):
        assert far.raw.slice(a, a + (1 << 18)) == decoded[a:a + (1 << 18)]
    assert oracle.find_magic(far.enc) == [b for b, _, _, _ in far.blocks]
    assert oracle.find_magic(far.enc, bigfiles.MAGIC_EOS) == far.eos
    for bit, at, size, value in far.blocks:
        assert decoded[at:at + size] == (bytes([value]) * size if value is not None else far.raw.slice(at, at + size))


QUERY_LAYOUTS = ({"cut": 1 << 18, "filler": 3_000, "text_size": 60_000}, {"cut": 1 << 18, "filler": 5_000, "text_size": 60_000})


def materialised(layout):
    far = bigfiles.far_file(**layout)
    data = far.raw.slice(0, far.raw.size)
    assert len(data) == far.raw.size and (layout["filler"] > bigfiles.VirtualRaw.RUN_SHRINK) == (layout["filler"] == 5_000)
    return far, data


def query_spans(far):
    """Spans of the shrunken layouts: whole, empty, around the cut, from and into fillers, from a filler to the end."""
    size, cut = far.raw.size, far.cut
    first_filler = len(far.t0)
    return [(0, size), (cut, 0), (cut - 131, 308), (cut - 1, 2), (0, len(far.t0)), (first_filler, size - first_filler),
            (first_filler - 500, 4_000), (first_filler + 7, far.t1_at + 90 - first_filler - 7), (far.t2_at - 6_000, 9_000), (far.t2_at + 11, 3_000)]


def test_virtual_raw_line_hashes_on_shrunken_layouts():
    import fields as F
    import linehash as LH
    import readershapes
    for layout in QUERY_LAYOUTS:
        far, data = materialised(layout)
        raw = far.raw
        for newline in (b"\n", b"_", b"\0"):
            lines = F.lines_of(data, newline[0])
            assert [data[a:b] for a, b in raw.line_bounds(newline)] == lines
            assert raw.first_occurrences(newline) == readershapes.first_occurrences_of(lines)
            for seed in (0, 1):
                assert raw.line_hashes(newline, seed) == LH.direct(data, newline[0], seed), (layout, newline, seed)
                x = LH.base(seed)
                for start, n in query_spans(far):
                    model = LH.summarise_chunk(data[start:start + n], newline[0], x)
                    summary, hashes = raw.hash_summary(start, n, newline, seed)
                    assert hashes == model["hashes"] and summary["count"] == len(hashes), (start, n)
                    assert summary == {key: model[key] for key in ("head", "tail", "has_delimiter", "tail_non_empty")} | {"count": len(hashes)}
        assert len(raw.first_occurrences()) < len(raw.line_bounds())          # T2 repeats T0
        for a, b, x in ((0, raw.size, LH.base(0)), (len(far.t0) - 3, far.t1_at + 3, LH.base(1)), (far.cut, far.cut, 300)):
            assert raw.part(a, b, x) == LH.part(data[a:b], x)


def test_virtual_raw_fields_on_shrunken_layouts():
    import collections
    import fieldhash as FH
    import fields as F
    import linehash as LH
    for layout in QUERY_LAYOUTS:
        far, data = materialised(layout)
        raw = far.raw
        for delimiter, newline in ((b" ", b"\n"), (b"e", b"\n"), (b"\n", b" "), (b"\t", b"\0"), (b" ", b"_")):
            dl, nl = delimiter[0], newline[0]
            for j in (0, 1, 3, 8, 9, 1023):
                spans = F.direct(data, nl, dl, j)
                assert raw.field_spans(j, delimiter, newline) == spans, (layout, delimiter, newline, j)
                if max(size for _, size in spans) < raw.MATERIALISE_MAX:
                    values = F.fields_of(data, nl, dl, j)
                    assert raw.field_values(j, delimiter, newline) == values
                    assert raw.field_values(j, delimiter, newline, 7, 30) == values[7:37] and raw.field_values(j, delimiter, newline, len(values), 3) == []
                if (j, delimiter) not in ((0, b" "), (3, b" "), (1, b"\n"), (0, b"\t")):
                    continue
                for seed in (0, 1):
                    keys = FH.keys_of(data, nl, dl, j, seed)
                    assert raw.field_keys(j, delimiter, newline, seed) == keys
                    # groups: the first line, the count and the missing ones, from the values themselves
                    values = F.fields_of(data, nl, dl, j)
                    tally = collections.Counter(v for v in values if v is not None)
                    firsts = {}
                    for k, v in enumerate(values):
                        if v is not None:
                            firsts.setdefault(v, k)
                    lines, counts, missing, where = raw.field_groups(j, delimiter, newline, seed)
                    assert lines == sorted(firsts.values()) and missing == sum(1 for v in values if v is None)
                    assert counts == [tally[values[k]] for k in lines] and where == [spans[k] for k in lines]
                    lines, counts, missing, _ = raw.field_groups(j, delimiter, newline, seed, 5, 40)
                    part = values[5:45]
                    assert missing == sum(1 for v in part if v is None) and sum(counts) + missing == len(part)
                    assert lines == sorted({5 + part.index(v) for v in part if v is not None})
                    if newline == b"\n" and delimiter == b" " and j == 3:
                        first = len(F.lines_of(data[:far.t1_at], nl))                # behind the line that holds the fillers
                        ordered = sorted(collections.Counter(v for v in values[first:first + 200] if v is not None).items(),
                                         key=lambda item: (-item[1], values.index(item[0], first)))
                        assert raw.value_counts(j, 7, delimiter, newline, seed, first, 200) == ordered[:7]
                    x = LH.base(seed)
                    for start, n in query_spans(far):
                        model = FH.Text(data[start:start + n], x, prefixes=False).summary(0, n, nl, dl, j)
                        got = raw.field_hash_summary(start, n, j, delimiter, newline, seed)
                        assert {key: got[key] for key in FH.FIELD_KEYS + FH.HASH_KEYS} == {key: model[key] for key in FH.FIELD_KEYS + FH.HASH_KEYS}, (start, n, j)
                        assert got["keys"] == model["keys"] and got["fields"] == [(start + a, size) for a, size in model["fields"]]
                        plain = raw.field_summary(start, n, j, delimiter, newline)
                        assert plain == {key: got[key] for key in FH.FIELD_KEYS + ("fields",)}


def test_virtual_raw_regex_on_shrunken_layouts():
    """Every pattern of the GPU tests, and the same patterns over the shrunken layouts' own first words, against re on the
    materialised bytes: with fillers of 3 000 bytes regex_lines sees the runs whole, with 5 000 it sees them cut."""
    import regexgen as G
    import readershapes
    for layout in QUERY_LAYOUTS:
        far, data = materialised(layout)
        raw = far.raw
        own = [b"^.+N3eDLe#16-MiXed\\. [a-z]", b"." + far.t0[:22].replace(b".", b"\\."), b"MiXed\\.$", b"^[^ ]* [^ ]*$",
               far.t0[-30:-24] + b".*" + far.t1[20:26], b"^.{0,255}N3eDLe", b".{200,255}N3eDLe", b"[^a]*N3eDLe#16-MiXed\\. [a-z]"]
        for pattern in list(bigfiles.FAR_PATTERNS.values()) + [bigfiles.FAR_CARRIED[0]] + own:
            for ignore_case in (False, True):
                assert raw.regex_lines(pattern, b"\n", ignore_case) == readershapes.reference_regex(data, pattern, ignore_case)[0], pattern
                for newline in (b"_", b"\0", bigfiles.FAR_CARRIED[1]):
                    assert raw.regex_lines(pattern, newline, ignore_case) == G.expected_lines(pattern, data, newline, ignore_case), pattern
        # the lines that hold fillers do match some of them: the rule is exercised, not vacuous
        filler_lines = {k for k, (a, b) in enumerate(raw.line_bounds()) if raw.holds_run(a, b)}
        assert len(filler_lines) == 2 and filler_lines <= set(raw.regex_lines(own[0])) and filler_lines <= set(raw.regex_lines(own[7]))
        assert set(raw.regex_lines(own[1])) & filler_lines and set(raw.regex_lines(own[4], b"\0")) == {0}


def test_far_file_placement_for_the_line_queries():
    """At full scale, what the GPU tests of the line queries rely on."""
    import fieldhash as FH
    far = bigfiles.far_file()
    raw, cut = far.raw, 1 << 32
    bounds = raw.line_bounds()
    assert len(raw.byte_offsets(10)) == len(bounds) == 39_214
    assert far.t0.count(b"\n") == 13_085 and far.t1.count(b"\n") == 13_044 and far.t0[-1:] == far.t1[-1:] == b"\n"
    # the line that straddles 2^32: 308 bytes, 8 spaces; its field 4 is the 256-byte needle with the '.' in front of it
    k = raw.line_of(cut)
    assert bounds[k] == (cut - 131, cut + 177)
    line = raw.slice(*bounds[k])
    assert line.count(b" ") == 8 and line.split(b" ")[4] == b"." + bigfiles.needles()["n256"]
    spans = {j: raw.field_spans(j, b" ")[k] for j in (0, 3, 4, 8, 9, 1023)}
    assert spans[4] == (cut - 101, 257) and spans[3][0] + spans[3][1] < cut < spans[8][0]
    assert spans[8][0] + spans[8][1] == cut + 177 and spans[9] == spans[1023] == (cut + 177, -1)
    # the first line of T1 begins with all 94 fillers; it and its field 0 are the largest of the file, 1.45 MB short of 2^32
    # (T0 and the fillers together are 2^32 - 449 924 bytes, and T0 ends in a newline)
    first = raw.line_of(far.t1_at)
    assert first == 13_085 and bounds[first][0] == len(far.t0) and bounds[first][1] - bounds[first][0] == 4_293_517_451 < cut
    assert raw.field_spans(0, b" ")[first] == (len(far.t0), 4_293_517_388)
    assert max(b - a for a, b in bounds) == 4_293_517_451
    # ... and no byte value is absent from both T0 and T1's bytes below 2^32, so no other delimiter gives a longer closed line
    assert set(far.t0) & set(far.t1[:cut - far.t1_at]) == set(far.t0) == set(far.t1)
    # under a byte that is in no text the whole file is one unterminated line of more than 2^32 bytes
    assert raw.line_bounds(b"\0") == [(0, raw.size)] and raw.field_spans(0, b"\t", b"\0") == [(0, raw.size)] and raw.size > cut
    # the first line of T2 begins with the two tail fillers; every other line of T2 is a duplicate of T0's
    second = raw.line_of(far.t2_at)
    assert bounds[second] == (far.t2_at - 2 * bigfiles.FULL_BLOCK, far.t2_at + far.t0.index(b"\n"))
    for seed in (0, 1):
        hashes = raw.line_hashes(b"\n", seed)
        assert hashes[second + 1:] == hashes[1:13_085] and hashes[second] not in hashes[:second]
        firsts = raw.first_occurrences(b"\n", seed)
        assert [n for n in firsts if n >= second] == [second] and first in firsts
    assert far.shift == cut + 92_348_546
    # the patterns are what their names say
    lines = {name: raw.regex_lines(pattern) for name, pattern in bigfiles.FAR_PATTERNS.items()}
    assert k in lines["caret"] and k in lines["dollar"] and lines["across"] == [k]
    assert lines["t2-only"] == [second] and lines["ascii-tail"] == [first] and {first, second} <= set(lines["behind-fillers"])
    assert lines["nowhere"] == [] and len(lines["class"]) > 100
    assert lines["short"] and all(b - a < 1000 for a, b in (bounds[n] for n in lines["short"]))
    assert any(bounds[n][0] > cut for n in lines["short"]) and any(bounds[n][0] < cut for n in lines["short"])
    pattern, newline = bigfiles.FAR_CARRIED
    carried = raw.line_bounds(newline)
    assert raw.regex_lines(pattern, newline) == [3] and carried[3][0] < len(far.t0) and far.t1_at < carried[3][1] < cut
    # the batch in another order: one field of more than 2^32 bytes in a closed line, not the line's first
    blocks, other = bigfiles.long_field_batch(far)
    at = other.line_of(len(far.t0), b" ")
    start, size = other.field_spans(1, b"\n", b" ")[at]
    assert size > cut and start == len(far.t0) and other.line_bounds(b" ")[at][0] < start
    assert other.field_keys(1, b"\n", b" ")[at] not in (0, FH.MISSING)


def test_deep_file_on_a_shrunken_layout(oracle):
    """The prefix (here 1 MB, two blocks) three times, the cut inside the second copy."""
    deep = bigfiles.deep_file(min_bits=20_000_000, cut_bits=12_000_000, prefix_size=1_000_000, text_size=300_000)
    assert deep.copies == 3 and len(deep.straddling) == 1
    status, decoded, block_map, garbage = oracle.decode_file(deep.enc)
    assert status == 0 and not garbage
    assert block_map == deep.map and len(decoded) == deep.size
    assert oracle.find_magic(deep.enc) == [b for b, _, _, _ in deep.blocks]
    assert oracle.find_magic(deep.enc, bigfiles.MAGIC_EOS) == deep.eos
    straddling = deep.straddling[0]
    following = min(b for b in deep.map if b > straddling)
    assert straddling + 48 <= deep.cut_bits < following
    for a, b in ((0, 100), (len(deep.body) - 50, len(deep.body) + 50), (deep.prefix_decoded - 1000, deep.prefix_decoded + 1000),
                 (deep.size - 70_000, deep.size + 10)):
        assert bigfiles.deep_slice(deep, a, b) == decoded[a:b]
    assert decoded[deep.prefix_decoded:] == deep.tail.slice(0, deep.tail.size)


def test_deep_file_keeps_its_promises():
    deep = bigfiles.deep_file()
    bits = 8 * len(deep.enc)
    assert bits > 2**32 + 2**26 and 8 * deep.copies * len(deep.body_stream) >= 2**32 + 2**26
    straddling = deep.straddling[0]
    assert straddling + 48 <= 2**32 < min(b for b in deep.map if b > straddling)
    assert deep.map[bits] == deep.size == deep.copies * len(deep.body) + deep.tail.size
    # every copy's offsets are the first copy's plus 8 x the bytes in front
    per_copy = len([b for b, _, _, _ in deep.blocks if b < 8 * len(deep.body_stream)])
    for k in (1, deep.copies - 1):
        for i in range(per_copy):
            assert deep.blocks[k * per_copy + i][0] == deep.blocks[i][0] + 8 * k * len(deep.body_stream)
    assert bz2.BZ2Decompressor().decompress(deep.body_stream) == deep.body


# ------------------------------------------------------------------------------------------------ inputs of the encoder

def header_constants():
    """The planner's constants, read from csrc/bz2_compress.hpp."""
    import os
    import re
    from conftest import ROOT
    with open(os.path.join(ROOT, "indexed_bzip2_amd", "csrc", "bz2_compress.hpp")) as f:
        text = f.read()
    blocks = int(re.search(r"DEFAULT_LAUNCH_BLOCKS = (\d+);", text).group(1))
    gib = int(re.search(r"DEFAULT_LAUNCH_BYTES = uint64_t\( (\d+) \) << 30;", text).group(1))
    terms = re.search(r"BYTES_PER_POSITION = ([0-9 +]+);", text).group(1)
    group = int(re.search(r"GROUP_SIZE = (\d+);", text).group(1))
    assert "(uint64_t)b.rle * BYTES_PER_POSITION + b.size + selectorSlots( b.rle ) * 8" in text
    assert "( symbolSlots( rle ) + GROUP_SIZE - 1 ) / GROUP_SIZE" in text and "return (uint64_t)rle + 1;" in text
    assert "return 100000 * (uint64_t)level - 19;" in text
    return blocks, gib << 30, sum(int(t) for t in terms.split("+")), group


def far_blocks():
    """[(piece, input offset in the launch, size, rle)] of far_pieces() at level 9, by bigfiles.plan_blocks."""
    far = bigfiles.far_file()
    cuts = {}
    out, at = [], 0
    for index, (_, value, data, length) in enumerate(far.raw.parts):
        key = data if value is None else (value, length)
        if key not in cuts:
            cuts[key] = bigfiles.plan_blocks(key, 9)
        for start, size, rle in cuts[key]:
            assert size > 0 and start + size <= length
            out.append((index, at + start, size, rle))
        at += length
    return out


def test_far_pieces_are_one_launch_beyond_4_gib(native):
    assert header_constants() == (bigfiles.LAUNCH_BLOCKS, bigfiles.LAUNCH_BYTES, bigfiles.BYTES_PER_POSITION, bigfiles.GROUP_SIZE)
    assert (bigfiles.LAUNCH_BLOCKS, bigfiles.LAUNCH_BYTES, bigfiles.BYTES_PER_POSITION) == (512, 12 << 30, 45)
    far, pieces, cut = bigfiles.far_file(), bigfiles.far_pieces(), 1 << 32
    # T0, 93 full fillers, the partial one, T1, two fillers, T2: 99 buffers, nine distinct filler arrays and texts
    full = [p for p in pieces if isinstance(p, np.ndarray) and len(p) == bigfiles.FULL_BLOCK]
    assert len(pieces) == 99 and len(full) == 95 and len({id(p) for p in full}) == 7
    assert [isinstance(p, bytes) for p in pieces] == [True] + [False] * 94 + [True] + [False] * 2 + [True]
    assert pieces[0] == far.t0 == pieces[98] and pieces[95] == far.t1 and 0 < len(pieces[94]) < bigfiles.FULL_BLOCK
    assert sum(len(p) for p in pieces) == far.raw.size == 4_388_315_842
    assert all(int(p[0]) == int(p[-1]) == value and len(p) == length
               for p, (_, value, _, length) in zip(pieces, far.raw.parts) if value is not None)
    assert sum(p.nbytes for p in {id(p): p for p in pieces if isinstance(p, np.ndarray)}.values()) < 420 << 20
    # the cuts: the product's planner on each distinct piece agrees with the restatement; a full filler is ONE block of
    # exactly 899 985 RLE1 bytes, a text two blocks
    for piece in {id(p): p for p in pieces}.values():
        key = piece if isinstance(piece, bytes) else (int(piece[0]), len(piece))
        assert native.plan_compress_blocks(piece, 9) == [size for _, size, _ in bigfiles.plan_blocks(key, 9)]
    assert bigfiles.plan_blocks((0x81, bigfiles.FULL_BLOCK), 9) == [(0, bigfiles.FULL_BLOCK, 899_985)]
    assert len(bigfiles.plan_blocks((0x81, bigfiles.FULL_BLOCK + 1), 9)) == 2
    assert bigfiles.block_bytes(bigfiles.FULL_BLOCK, 899_985) == 86_542_560
    blocks = far_blocks()
    assert len(blocks) == 102 and [index for index, _, _, _ in blocks[:3]] == [0, 0, 1]
    # inOff: the running sum of the sizes, every block inside its piece
    at = 0
    for index, offset, size, rle in blocks:
        assert offset == at and rle <= 899_985
        at += size
    assert at == far.raw.size
    # one launch: 102 blocks, 8.4 GB of the 12 GiB budget -- the budget is by blockBytes, not by input bytes
    launches = bigfiles.plan_launches([(size, rle) for _, _, size, rle in blocks])
    assert launches == [(0, 102, 0, far.raw.size, sum(bigfiles.block_bytes(size, rle) for _, _, size, rle in blocks))]
    assert launches[0][4] == 8_406_950_504 < bigfiles.LAUNCH_BYTES and launches[0][3] > cut
    # the first inOff at or above 2^32 is block 97's: T1's second block, 450 057 bytes above; five blocks start above
    above = [k for k, (_, offset, _, _) in enumerate(blocks) if offset >= cut]
    assert above == [97, 98, 99, 100, 101] and blocks[97][1] == cut + 450_057 and blocks[96][1] == far.t1_at < cut
    # a block read at inOff - 2^32 would read other bytes: the fillers another value (assert_no_alias), the texts other text
    bigfiles.assert_no_alias(far.raw, cut)
    for k in above:
        index, offset, size, _ = blocks[k]
        n = min(size, 4096)
        assert far.raw.slice(offset, offset + n) != far.raw.slice(offset - cut, offset - cut + n), k
        assert far.raw.slice(offset + size - n, offset + size) != far.raw.slice(offset + size - n - cut, offset + size - cut), k
        if isinstance(pieces[index], np.ndarray):
            low = far.raw.slice(offset - cut, offset - cut + 1) + far.raw.slice(offset + size - 1 - cut, offset + size - cut)
            assert int(pieces[index][0]) not in low
    # 148 fillers fit one launch by the budget, 6.8 GB of input; the 149th does not
    filler = (bigfiles.FULL_BLOCK, 899_985)
    assert [l[1] for l in bigfiles.plan_launches([filler] * 200)] == [148, 52]
    assert bigfiles.plan_launches([filler] * 200)[1][2] == 148 * bigfiles.FULL_BLOCK > cut


def test_deep_input_is_incompressible():
    """libbz2's ratio on 4.5 MB of deep_input()'s generator is at least 1, so the stream of the 550 000 000 bytes has more
    than 2^32 + 2^26 bits whatever the encoder (deep_file relies on the same)."""
    sample = datagen.random_bytes(4_500_000, bigfiles.DEEP_INPUT_SEED)
    assert len(bz2.compress(sample, 9)) >= len(sample)
    assert 8 * bigfiles.DEEP_INPUT_SIZE >= 2**32 + 2**26
    blocks = -(-bigfiles.DEEP_INPUT_SIZE // 899_981)
    assert 611 <= blocks <= 613 and blocks * bigfiles.block_bytes(899_981, 899_981) > bigfiles.LAUNCH_BYTES      # two launches
