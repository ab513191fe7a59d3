"""The encoder on offsets beyond 2^32: a launch whose input passes 2^32 bytes (EncBlock::inOff, the CRC's pieces, the
staging copy), output bit positions beyond 2^32 (hBitPos, BitWriter, FrameJob::bit, the zeroing and growing of the result
buffer) and the stream-relative block map beyond 2^32 bits.

A truncated inOff or bit position does not fault: it reads another block's bytes or ORs bits into the front of the output,
and the call returns status 0.  So every expected value comes from somewhere the offsets are small: the same buffers
compressed in calls of their own (the output does not depend on the launch split), CPython's bz2, the oracle's
decoder on blocks cut out by bit offset, and plain integer arithmetic on the stream (bits, the rotl-xor fold of the CRCs).
The inputs are tests/bigfiles.py's (far_pieces, deep_input); test_bigfiles.py checks their arithmetic without a GPU.

Every test uses a context of its own and closes it: a call leaves gigabytes of encoder scratch and staging on its context.
Measured figures: DESIGN.md 5, "The encoder beyond 2^32"."""
import bz2
import io

import pytest

import bigfiles
import datagen

pytestmark = pytest.mark.gpu

CUT = 1 << 32
LEVEL = 9


def bits(blob, a, b):
    """Bits [a, b) of blob, MSB first, as a Python integer."""
    first, last = a // 8, (b + 7) // 8
    return (int.from_bytes(blob[first:last], "big") >> (8 * last - b)) & ((1 << (b - a)) - 1)


def cut_out(blob, a, b):
    """Bits [a, b) of blob moved to bit 0 of a byte string of their own, zero padded."""
    n = b - a
    return (bits(blob, a, b) << (-n % 8)).to_bytes((n + 7) // 8, "big")


def fold(crcs):
    """bzip2's stream CRC of its blocks' CRCs: rotate left by one, xor."""
    crc = 0
    for c in crcs:
        crc = (((crc << 1) | (crc >> 31)) & 0xFFFFFFFF) ^ c
    return crc


def compress_on(dec, buffers, cap=0):
    """What buffers.compress_many does, on the context `dec`: ([stream], [block map], results)."""
    results, total = dec.compress_buffers(buffers, LEVEL, cap)
    at = 0
    for r in results:
        assert r["status"] == 0 and r["output_offset"] == at
        at += r["compressed_size"]
    assert total == at
    blob = dec.copy_output(0, total)
    maps = [dec.compress_block_map(i) for i in range(len(buffers))]
    return [blob[r["output_offset"]:r["output_offset"] + r["compressed_size"]] for r in results], maps, results


def result_requests(bounds, counts, size):
    """The sizes runCall asks the result buffer for (zeroTo): after each launch of counts[i] blocks the bytes up to the end
    of its last block, rounded up to a word, plus 8; at the end the same of the whole output.  `bounds`: the blocks' bits
    and the end-of-stream bit of ONE stream at output offset 0."""
    ends, at = [], 0
    for count in counts:
        at += count
        ends.append((bounds[at] + 7) // 8)
    return [(end + 3) // 4 * 4 + 8 for end in ends + [size]]


def result_capacities(requests):
    """The capacities mi355x::resultBuffer of a fresh context passes through: a request that does not fit (with 256 bytes
    of slack) allocates max(request + 256, 1.5 x capacity, 1 MiB) and copies what is kept -> [(capacity, bytes kept)]."""
    grown, capacity, kept = [], 0, 0
    for request in requests:
        if request + 256 > capacity:
            capacity = max(request + 256, capacity + capacity // 2, 1 << 20)
            grown.append((capacity, kept))
        kept = max(kept, request)
    return grown


def check_stream(out, index, data, oracle, around):
    """A stream and its returned block map against the input, by plain arithmetic: the map's layout, every block's magic and
    header CRC at its map bit, the fold of the header CRCs against the trailer, zero padding; and, for the block that holds
    bit `around` and two neighbours on each side, the block cut out by bit offset and decoded by the oracle against the
    input slice and its CRC.  Returns the blocks' bits (ascending), the end-of-stream bit and the straddling block's number."""
    entries = sorted(index)
    blocks, eos, end = entries[:-2], entries[-2], entries[-1]
    assert end == 8 * len(out) and index[end] == index[eos] == len(data) and out[:4] == b"BZh9"
    assert blocks[0] == 32 and index[blocks[0]] == 0
    assert all(index[a] < index[b] for a, b in zip(blocks, blocks[1:] + [eos]))
    crcs = []
    for bit in blocks:
        assert bits(out, bit, bit + 48) == bigfiles.MAGIC_BLOCK, bit
        crcs.append(bits(out, bit + 48, bit + 80))
    assert bits(out, eos, eos + 48) == bigfiles.MAGIC_EOS
    assert bits(out, eos + 48, eos + 80) == fold(crcs)
    assert 0 <= end - (eos + 80) < 8 and bits(out, eos + 80, end) == 0
    k = max(j for j, bit in enumerate(blocks) if bit <= around)
    bounds = blocks + [eos]
    assert blocks[k] < around < bounds[k + 1] and 2 <= k < len(blocks) - 2
    for j in range(k - 2, k + 3):
        piece = cut_out(out, bounds[j], bounds[j + 1]) + bytes(16)
        want = data[index[bounds[j]]:index[bounds[j + 1]]]
        record, decoded = oracle.decode_block(piece, 0)
        assert record["status"] == 0 and decoded == want, j
        assert record["header_crc"] == record["computed_crc"] == crcs[j] == oracle.crc32(want) ^ 0xFFFFFFFF, j
    return blocks, eos, k


# ------------------------------------------------------------------------------------- a launch's input beyond 2^32 bytes

def test_launch_input_beyond_4_gib(native):
    """far_pieces() -- 99 buffers, 102 blocks, 4 388 315 842 bytes -- in ONE launch: block 97's inOff is the first at or
    above 2^32 (test_bigfiles.py).  Every stream must be the one the same buffer gives in a call of the ten distinct
    buffers alone (every inOff there is below 350 MB, and CPython's bz2 decodes each of those streams to its input), and the
    streams decode, on the same context, to the fillers' values where they must lie and to the texts."""
    N = native._native
    far, pieces = bigfiles.far_file(), bigfiles.far_pieces()
    dec = N.Decoder(device=0)
    try:
        distinct = list({id(p): p for p in pieces}.values())      # seven full fillers, the partial one, T0 (= T2) and T1
        assert len(distinct) == 10
        streams, _, _ = compress_on(dec, distinct)          # one launch of 348 MB (why not one block per launch: DESIGN.md 5)
        reference = {}
        for piece, stream in zip(distinct, streams):
            assert bz2.decompress(stream) == (piece if isinstance(piece, bytes) else piece.tobytes())
            reference[id(piece)] = stream

        results, total = dec.compress_buffers(pieces, LEVEL)
        at = 0
        for piece, r in zip(pieces, results):
            assert r["status"] == 0 and r["output_offset"] == at and r["compressed_size"] == len(reference[id(piece)])
            assert r["n_blocks"] == (2 if isinstance(piece, bytes) else 1)
            at += r["compressed_size"]
        assert total == at and sum(r["n_blocks"] for r in results) == 102
        got = [dec.copy_output(r["output_offset"], r["compressed_size"]) for r in results]
        for k, (piece, stream) in enumerate(zip(pieces, got)):
            assert stream == reference[id(piece)], k
        # the map of T1, whose second block's input lies above 2^32 in the launch, and of T2
        for k in (95, 98):
            blocks = sorted(dec.compress_block_map(k).items())
            assert [at for _, at in blocks] == [0, 899_981, 1_000_000, 1_000_000] and blocks[0][0] == 32
            assert blocks[-1][0] == 8 * len(got[k])

        # back through the decoder on the same context: the content where it must lie
        decoded, size = dec.decompress_buffers(got)
        assert size == far.raw.size and [r["status"] for r in decoded] == [0] * len(pieces)
        assert [(r["output_offset"], r["decoded_size"]) for r in decoded] == [(o, n) for o, _, _, n in far.raw.parts]
        fillers = [(offset, length, value) for offset, value, _, length in far.raw.parts if value is not None]
        assert len(fillers) == 96 and sum(1 for o, _, _ in fillers if o > CUT) == 2
        for value in sorted({v for _, _, v in fillers}):
            spans = [(o, n) for o, n, v in fillers if v == value]
            assert dec.count_byte(value, spans) == [n for _, n in spans], hex(value)
            # below, across and above 2^32: the value occurs nowhere else
            whole = [(0, CUT), (CUT - (200 << 20), 280 << 20), (CUT, size - CUT), (0, size)]
            want = [sum(max(0, min(a + n, o + m) - max(a, o)) for o, m in spans) for a, n in whole]
            assert dec.count_byte(value, whole) == want, hex(value)
        for o, n, value in fillers[-4:]:
            assert dec.count_byte(value, [(o - 4096, n + 8192)]) == [n]
        assert dec.copy_output(far.t1_at, len(far.t1)) == far.t1
        assert dec.copy_output(far.t2_at, len(far.t0)) == far.t0 == dec.copy_output(0, len(far.t0))
        assert dec.copy_output(CUT - 70_000, 140_000) == far.raw.slice(CUT - 70_000, CUT + 70_000)
    finally:
        dec.close()


# --------------------------------------------------------------------------------------------- output bits beyond 2^32

def test_output_bits_beyond_2_32(native, oracle):
    """One stream of more than 2^32 + 2^26 bits, in two launches at the default cap and, on a second fresh context, in ten
    at 64 blocks.  Each context's result buffer starts empty, so it grows inside the call with written content kept: its final
    capacity must be the one the growth rule reaches through the requests of that launch split (result_capacities)."""
    N = native._native
    data = bigfiles.deep_input()
    dec = N.Decoder(device=0)
    try:
        (out,), (index,), results = compress_on(dec, [data])
        capacity = dec.device_memory()["output_bytes"]       # before any later call on this context can grow it
        # a condition of the input (incompressible bytes: test_bigfiles.py), not of the code under test
        assert 8 * len(out) >= CUT + (1 << 26)
        assert results[0]["n_blocks"] == len(index) - 2 and 611 <= results[0]["n_blocks"] <= 613
        assert sum(1 for bit in index if bit < CUT) >= 500 and sum(1 for bit in index if bit > CUT) >= 10

        blocks, eos, k = check_stream(out, index, data, oracle, CUT)
        # the result buffer of this call: the blocks' RLE1 sizes lie in [899 981, 899 985] (incompressible bytes), and both
        # ends give the same launch split; the last growth -- the trailer's few bytes -- copies more than 512 MiB of stream
        sizes = [index[b] - index[a] for a, b in zip(blocks, blocks[1:] + [eos])]
        split = [count for _, count, _, _, _ in bigfiles.plan_launches([(n, min(n, 899_981)) for n in sizes])]
        assert split == [count for _, count, _, _, _ in bigfiles.plan_launches([(n, min(n, 899_985)) for n in sizes])]
        assert len(split) == 2 and split[0] < k < sum(split)
        grown = result_capacities(result_requests(blocks + [eos], split, len(out)))
        assert capacity == grown[-1][0] and len(grown) == 3 and grown[-1][1] > 512 << 20 > grown[-2][1] > 0
        # the reader's own scan of the stream (pinned past 2^32 by deep_file) finds the same map
        with native.open(io.BytesIO(out), 0) as f:
            assert f.block_offsets() == index
        with native.open(io.BytesIO(out), 4) as f:
            f.set_block_offsets(index)
            assert f.read() == data

        # the low-offset twin: the input from eight blocks before the crossing on, in a call of its own.  A block starts at
        # a piece boundary, so the cuts are the same, and every block's bits must be the big stream's
        k0 = k - 8
        base = index[blocks[k0]]
        (twin,), (twin_index,), _ = compress_on(dec, [data[base:]])
        twin_blocks, twin_eos, _ = check_stream(twin, twin_index, data[base:], oracle, sorted(twin_index)[8] + 1000)
        assert 8 * len(twin) < 1 << 28 and len(twin_blocks) == len(blocks) - k0 >= 12
        ours, theirs = blocks[k0:] + [eos], twin_blocks + [twin_eos]
        assert [index[bit] - base for bit in ours] == [twin_index[bit] for bit in theirs]
        for j in range(len(twin_blocks)):
            assert ours[j + 1] - ours[j] == theirs[j + 1] - theirs[j], j
            assert bits(out, ours[j], ours[j + 1]) == bits(twin, theirs[j], theirs[j + 1]), j
        assert sum(1 for bit in ours[:-1] if bit > CUT) >= 10 and ours[8] < CUT < ours[9]
    finally:
        dec.close()

    # another launch split on a context of its own, whose result buffer is empty: ten launches, the crossing in the tenth,
    # and the buffer reallocated six times with the stream written so far copied into the new one
    other = N.Decoder(device=0)
    try:
        (again,), (again_index,), _ = compress_on(other, [data], cap=64)
        capacity = other.device_memory()["output_bytes"]
        assert again == out and again_index == index
        split = [64] * (len(blocks) // 64) + [len(blocks) % 64]
        assert len(split) == 10 and sum(split[:9]) <= k
        grown = result_capacities(result_requests(blocks + [eos], split, len(out)))
        assert capacity == grown[-1][0] and len({c for c, _ in grown}) == len(grown) >= 5
        assert sum(1 for _, kept in grown if kept > 0) >= 4 and grown[-1][0] > len(out) + 256
    finally:
        other.close()


# ------------------------------------------------------------------------------- many streams, a frame at output bit 2^32

def test_many_streams_across_2_32_bits(native):
    """Sixty-two incompressible buffers, most of 9 MiB, with two sizes chosen so that one stream's "BZh9" is the first thing
    written at or above output bit 2^32 and its predecessor's end-of-stream frame starts below.  The sizes come from
    arithmetic on the streams of the same buffers compressed alone (where every offset is small): the output of a call is
    those streams back to back."""
    N = native._native
    size = 9 << 20
    distinct = [datagen.random_bytes(size, 0x62_00 + j) for j in range(8)]
    source = datagen.random_bytes(12 << 20, 0x62_FE)
    dec = N.Decoder(device=0)
    try:
        alone = {}

        def stream_of(buffer):
            if buffer not in alone:
                alone[buffer] = compress_on(dec, [buffer])[0][0]
            return alone[buffer]

        target = CUT // 8
        standard = [distinct[i % 8] for i in range(62)]
        total, m = 0, 0
        while total + len(stream_of(standard[m])) <= target - (1 << 20):
            total += len(stream_of(standard[m]))
            m += 1
        # one buffer of another size brings the end to a few thousand bytes below 2^29 (the ratio of incompressible bytes is
        # that of the buffers just compressed; the slack covers its scatter), then one small buffer to [2^29, 2^29 + 9]
        gap = target - total
        ratio = len(stream_of(standard[0])) / size
        assert (1 << 20) <= gap <= (11 << 20) and 1.0 <= ratio <= 1.01
        shortened = source[:int((gap - 4_000) / ratio)]
        rest = gap - len(stream_of(shortened))
        assert 1_000 <= rest <= 8_000, rest
        noise = datagen.random_bytes(rest + 64, 0x62_FF)
        candidates = [noise[:n] for n in range(max(1, rest - 1_200), rest + 1)]
        sizes = [len(s) for s in compress_on(dec, candidates)[0]]
        fitting = [c for c, n in zip(candidates, sizes) if rest <= n <= rest + 9]
        assert fitting, (rest, sizes[0], sizes[-1])
        small = fitting[0]
        alone[small] = compress_on(dec, [small])[0][0]
        buffers = standard[:m] + [shortened, small] + standard[m + 2:]
        assert len(buffers) == 62 and all(a != b for a, b in zip(buffers, buffers[1:]))
        for buffer in buffers:
            stream_of(buffer)

        outs, maps, results = compress_on(dec, buffers)
        # every frame job's bit: 8 x the stream's offset ("BZh9") and that plus the stream's end-of-stream bit
        frames = []
        for r, index in zip(results, maps):
            frames += [(8 * r["output_offset"], "header"), (8 * r["output_offset"] + sorted(index)[-2], "trailer")]
        frames.sort()
        first = next(i for i, (bit, _) in enumerate(frames) if bit >= CUT)
        assert frames[first][1] == "header" and frames[first - 1][1] == "trailer" and frames[first - 1][0] < CUT
        assert CUT <= frames[first][0] <= CUT + 72 and frames[first][0] == 8 * results[m + 2]["output_offset"]
        assert frames[-1][0] > CUT + (1 << 26)
        for k, (buffer, out) in enumerate(zip(buffers, outs)):
            assert out == alone[buffer], k
        for buffer in (distinct[0], shortened, small):
            assert bz2.decompress(alone[buffer]) == buffer
        decoded, total = dec.decompress_buffers(outs)
        assert total == sum(len(b) for b in buffers) and [r["status"] for r in decoded] == [0] * 62
        blob = dec.copy_output(0, total)
        for k, (buffer, r) in enumerate(zip(buffers, decoded)):
            assert r["decoded_size"] == len(buffer) and blob[r["output_offset"]:r["output_offset"] + len(buffer)] == buffer, k
    finally:
        dec.close()
