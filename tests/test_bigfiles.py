"""tests/bigfiles.py on the CPU: VirtualRaw against the same parts held in memory, crc_concat against the oracle's CRC, and
the two builders against CPython's bz2 decoder and the oracle's block map -- at full scale where that takes seconds
(far_file's promises, the streams around 2^32), at a shrunken scale where it would not (the whole block map)."""
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
