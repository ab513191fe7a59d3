"""Crafted last columns for the decoder's back half (table build, k_walk, k_link2, k_emit, k_replicate, k_rle, k_crc).

Every full-size block that libbz2 writes is the BWT of data: its segments are geometric, its LF permutation is one cycle
(or N/c equal ones), its RLE1 stream never ends inside a run.  The format lets a block carry ANY last column and origPtr,
and the reference decodes them all (bzip2.hpp:810-910).  This module holds
  - model_decode: that part of the reference restated in plain integers (no oracle, no product),
  - walk_geometry: the segment cut rule of bz2_walk.hip.h restated, so that every case can assert ON THE CPU that it
    reaches the branch it is there for (a changed KMAX / STASH_BYTES / EMIT_STAGE / LINK_SPLIT fails the CPU test
    instead of silently leaving a branch unreached),
  - the cases, and their streams (bz2enc.encode_block_from_bwt), memoised per process.
"""
import functools
import zlib

import numpy as np

import bz2enc

# the constants of bz2_scratch.hpp / bz2_walk.hip.h that the geometry below restates
KMAX = 32768
MIN_SEG_STRIDE = 16
STASH_BYTES = 128
EMIT_THREADS = 256
EMIT_STAGE = 16384
LINK_SPLIT = 128
RLE_CHUNK, RLE_WAVE, RLE_TILE = 32, 2048, 16384

_BITREV = bytes(int(f"{b:08b}"[::-1], 2) for b in range(256))


def crc32_bzip2(data):
    """bzip2's CRC-32 (MSB first) of `data`, complemented as the block header stores it: zlib's CRC-32 is the same
    polynomial bit-reversed, so reverse every byte going in and the 32 bits coming out."""
    return int(f"{zlib.crc32(bytes(data).translate(_BITREV)):032b}"[::-1], 2)


def inverse_tables(last):
    """(T, LF) of the column: T[j] = index in `last` of the j-th byte of the stably sorted column (what prepare() scatters
    into dbuf, bzip2.hpp:817-831), LF = T^-1."""
    a = np.frombuffer(bytes(last), dtype=np.uint8)
    T = np.argsort(a, kind="stable")
    LF = np.empty(len(a), dtype=np.int64)
    LF[T] = np.arange(len(a))
    return T, LF


def rle1_decode(pre):
    """bzip2.hpp:881-896: after four equal bytes the next byte is a count; after a count nothing equals its predecessor;
    the block simply ends wherever the bytes run out."""
    out = bytearray()
    run = 0          # equal bytes seen so far (0: nothing to be equal to)
    prev = -1
    for b in pre:
        if run == 4:
            out += bytes([prev]) * b
            run, prev = 0, -1
            continue
        out.append(b)
        run = run + 1 if b == prev else 1
        prev = b
    return bytes(out)


def model_decode(last, orig_ptr):
    """(pre-RLE1 bytes, decoded bytes, CRC) of a block with this column: bzip2.hpp:810-910 in plain integers."""
    n = len(last)
    assert 0 <= orig_ptr < n
    T = inverse_tables(last)[0].tolist()
    pre = bytearray(n)
    pos = T[orig_ptr]
    for i in range(n):
        pre[i] = last[pos]
        pos = T[pos]
    out = rle1_decode(pre)
    return bytes(pre), out, crc32_bzip2(out)


def walk_geometry(last, orig_ptr):
    """How bz2_walk.hip.h cuts this column: segments start at every stride-th table index and at origPtr and run along LF
    to the next start.  Statistics over ALL segments (k_walk follows every one) and over those on the origPtr cycle in
    cycle order (k_link2's chain, k_emit's pieces of EMIT_THREADS consecutive ones)."""
    n = len(last)
    LF = inverse_tables(last)[1].tolist()
    stride = max(MIN_SEG_STRIDE, -(-n // KMAX))
    k0 = -(-n // stride)
    extra = orig_ptr % stride != 0
    nseg = k0 + (1 if extra else 0)
    first = k0 if extra else orig_ptr // stride
    marked = bytearray(n)
    marked[::stride] = b"\x01" * k0
    marked[orig_ptr] = 1

    def seg_id(p):
        return k0 if (p == orig_ptr and extra) else p // stride

    def seg_len(p):
        length = 1
        p = LF[p]
        while not marked[p] and length < n:
            p = LF[p]
            length += 1
        return length, p
    lengths = {}
    for j in range(k0):
        lengths[j] = seg_len(j * stride)[0]
    if extra:
        lengths[k0] = seg_len(orig_ptr)[0]
    # the chain: from origPtr until LF comes back (or N steps have passed)
    chain = []
    p, c = orig_ptr, 0
    while True:
        length, q = seg_len(p)
        chain.append((seg_id(p), length))
        c += length
        p = q
        if p == orig_ptr or c >= n:
            break
    chain_lengths = [l for _, l in chain]
    pieces = [sum(chain_lengths[i:i + EMIT_THREADS]) for i in range(0, len(chain), EMIT_THREADS)]
    all_lengths = list(lengths.values())
    return {
        "n": n, "stride": stride, "k0": k0, "nseg": nseg, "first": first, "first_extra": first % LINK_SPLIT != 0,
        "c": c, "n_mod_c": n % c, "nchain": len(chain), "chain": chain,
        "longest": max(all_lengths), "over_stash": sum(1 for l in all_lengths if l > STASH_BYTES),
        "ones": sum(1 for l in all_lengths if l == 1),
        "chain_longest": max(chain_lengths), "worst_piece": max(pieces),
    }


def segment_of(geometry, k):
    """Which chain segment holds byte k of the backward walk from origPtr (k < c): (position in the chain, segment id,
    length, offset inside)."""
    off = 0
    for rank, (seg, length) in enumerate(geometry["chain"]):
        if k < off + length:
            return rank, seg, length, k - off
        off += length
    raise AssertionError(k)


def describe(geometry, pre_index):
    """For failure messages: the segment that wrote byte `pre_index` of the pre-RLE1 stream."""
    # the reference's byte j is the backward walk's byte (N - 1 - j - N mod c) mod c (k_replicate's comment)
    k = (geometry["n"] - 1 - pre_index - geometry["n_mod_c"]) % geometry["c"]
    rank, seg, length, inside = segment_of(geometry, k)
    return (f"pre-RLE1 byte {pre_index}: chain position {rank} (k_emit piece {rank // EMIT_THREADS}), segment {seg} of "
            f"length {length}, byte {inside} of it; stride {geometry['stride']}, nseg {geometry['nseg']}, "
            f"first {geometry['first']}, c {geometry['c']}, N % c {geometry['n_mod_c']}")


# ---------------------------------------------------------------------------------------------------------------------
# columns
# ---------------------------------------------------------------------------------------------------------------------
def comb(n, fill=0):
    """The first `stride` entries are the distinct values 0x80 + (k + 1) % stride, the rest is `fill`: LF moves the table
    index by -stride inside a residue class and the teeth chain the classes (when stride divides the fill count)."""
    stride = max(MIN_SEG_STRIDE, -(-n // KMAX))
    return bytes(0x80 + (k + 1) % stride for k in range(stride)) + bytes([fill]) * (n - stride)


def rot(n):
    """The pure rotation: LF[i] = i - 1."""
    return b"b" + b"a" * (n - 1)


def random_column(n, symbols, seed):
    return np.random.default_rng(seed).integers(0, symbols, n, dtype=np.uint8).tobytes()


def sorted_column(n=30_000):
    values = np.array([0, 1, 2, 3, 5, 8, 13], dtype=np.uint8)
    return np.sort(values[np.random.default_rng(7).integers(0, 7, n)]).tobytes()


def filler(n, seed):
    """Bytes over 6 values (1..6), no two adjacent equal."""
    steps = np.random.default_rng(seed).integers(1, 6, n)
    steps[0] = 0
    return (np.cumsum(steps) % 6 + 1).astype(np.uint8).tobytes()


def with_runs(n, runs, seed):
    """Filler of n bytes with `value` four times and then `count`, the count byte at index p, for (p, value, count) in
    `runs`."""
    s = bytearray(filler(n, seed))
    for p, value, count in runs:
        assert p >= 4 and p < n
        s[p - 4:p + 1] = bytes([value]) * 4 + bytes([count])
    return bytes(s)


RLE_EDGE_POSITIONS = [31, 32, 33, 34, 35, 36, 2047, 2048, 2049, 2050, 2051, 2052,
                      16383, 16384, 16385, 16386, 16387, 16388]


def rle_streams():
    """name -> the pre-RLE1 stream s; the column is bwt_numpy(s)."""
    out = {}
    for i, p in enumerate(RLE_EDGE_POSITIONS):
        count = (0, 1, 255)[i % 3]
        out[f"rle-count{count}-at-{p}"] = with_runs(p + 41, [(p, 0x71, count)], 100 + i)
    out["rle-run-at-every-edge"] = with_runs(33_000, [(32, 0x71, 3), (2048, 0x72, 0), (16384, 0x73, 255),
                                                      (32768, 0x74, 7)], 200)
    # 16 404 bytes, the last four equal and no count behind them; a count of 66 on the last byte of the first tile
    out["rle-ends-in-four-equal"] = with_runs(16_400, [(16383, 0x71, 66)], 201) + b"wwww"
    out["rle-ends-in-three-equal-16385"] = filler(16_382, 202) + b"www"
    out["rle-ends-in-three-equal-16384"] = filler(16_381, 203) + b"www"
    # the count equals the run's value and that value follows again: it starts a new run (state 0 -> 1 on an "equal" byte)
    out["rle-count-equals-value"] = filler(50, 204) + b"0000" + b"\x30" + b"0000" + b"\x02" + b"000" + filler(40, 205)
    out["rle-back-to-back"] = b"qqqq\x00" * 3400 + b"qqqq\x02q"
    return out


# name -> (kind, column, origPtr) for the inverse-BWT cases; kind selects the geometry check of test_crafted_streams
def _ibwt_columns():
    cases = {}
    for n, orig in ((40_000, 5), (40_000, 0), (65_537, 5), (65_537, 0), (4_096, 2_048), (2_048, 7), (544_000, 5)):
        cases[f"comb-{n}-{orig}"] = (comb(n), orig)
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 2047, 2048, 2049):
        cases[f"rot-{n}"] = (rot(n), n - 1)
    for n, orig in ((524_288, 0), (524_288, 5), (524_289, 5), (900_000, 5)):
        cases[f"rot-{n}-{orig}"] = (rot(n), orig)
    cases["sorted-30000"] = (sorted_column(), 777)
    cases["random4-50000"] = (random_column(50_000, 4, 1), 1_234)
    cases["random256-50000"] = (random_column(50_000, 256, 3), 4_096)
    cases["random2-3000"] = (random_column(3_000, 2, 4), 17)
    cases["random4-524288"] = (random_column(524_288, 4, 2), 99)
    return cases


IBWT_NAMES = sorted(_ibwt_columns())
RLE_NAMES = sorted(rle_streams())
NAMES = IBWT_NAMES + RLE_NAMES
SMALL_N = 70_000      # cases up to this N go into the golden file, the table-build variants and the crafted batch


@functools.lru_cache(maxsize=None)
def column(name):
    """(last column, origPtr) of a case."""
    if name in RLE_NAMES:
        return bz2enc.bwt_numpy(rle_streams()[name])
    return _ibwt_columns()[name]


def small_names():
    return [name for name in NAMES if case_n(name) <= SMALL_N]


def case_n(name):
    return len(rle_streams()[name]) if name in RLE_NAMES else int(name.split("-")[1])


@functools.lru_cache(maxsize=None)
def model(name):
    return model_decode(*column(name))


@functools.lru_cache(maxsize=None)
def geometry(name):
    return walk_geometry(*column(name))


def flat_lengths(t, alphabet, freq):
    """A complete code of near-equal lengths, the shorter ones on the frequent symbols: keeps the streams small."""
    extra = max(1, (alphabet - 1).bit_length())
    short = (1 << extra) - alphabet
    ranking = sorted(range(alphabet), key=lambda s: (-freq[s], s))
    lengths = [0] * alphabet
    for i, s in enumerate(ranking):
        lengths[s] = extra - 1 if i < short else extra
    return lengths


@functools.lru_cache(maxsize=None)
def stream(name):
    """The single-block .bz2 of a case."""
    last, orig_ptr = column(name)
    return bz2enc.encode_block_from_bwt(last, orig_ptr, model(name)[2], length_fn=flat_lengths)


@functools.lru_cache(maxsize=None)
def tiny_blocks_file():
    """130 single-block streams in one file, decoded sizes 1 ... 130: decoded as one batch, the blocks' output offsets take
    every residue mod 64.  -> (file, the decoded parts)."""
    rng = np.random.default_rng(130)
    parts = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for size in range(1, 131)]
    return b"".join(bz2enc.encode_block(p) for p in parts), parts


@functools.lru_cache(maxsize=None)
def crafted_batch():
    """Every case with N <= SMALL_N in one file, and a shuffled list of (name, block bit offset) that names each block
    twice (>= 64 entries): one k_walk claim of 256 segments then spans many blocks of 1-3 segments, next to blocks with
    thousands.  Every stream is whole bytes long, so block k starts 32 bits into stream k."""
    names = small_names()
    data = bytearray()
    entries = []
    for name in names:
        entries.append((name, len(data) * 8 + 32))
        data += stream(name)
    entries = entries * 2
    order = np.random.default_rng(0xBA7C4).permutation(len(entries))
    entries = [entries[i] for i in order]
    assert len(entries) >= 64
    return bytes(data), entries


def parse_probe(line):
    """A line of the reference probe (oracle/ref_harness.cpp: "OK offset size headerCRC calcCRC decoded fnv64 eos eof" or
    "EXC type what") as the record that tests/golden/crafted_vectors.json holds."""
    f = line.strip().split()
    if f[0] != "OK":
        return {"verdict": f[0], "what": " ".join(f[1:])[:160]}
    return {"verdict": "OK", "size": int(f[2]), "header_crc": int(f[3], 16), "calc_crc": int(f[4], 16),
            "decoded": int(f[5]), "fnv64": f[6]}
