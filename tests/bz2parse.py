"""A plain bzip2 block PARSER for tests, and the plain references of the encoder's stages.

An emitted stream is its own stage dump: the block header holds the CRC, origPtr, the byte values in use, the table
count, the selectors and every table's code lengths; the symbols behind it are the MTF/RUNA/RUNB/EOB stream.  With the
oracle's L column and pre-RLE1 bytes (`oracle.decode_block(..., want_stages=True)`) every stage of an encoder can be
compared with a reference of that stage alone.  Pure Python + numpy; nothing here knows the product."""
import bz2
import functools
import heapq

import numpy as np

import bz2enc

MAGIC_BLOCK = 0x314159265359
MAGIC_EOS = 0x177245385090
GROUP_SIZE = 50
MAX_FORMAT_LENGTH = 20      # what the format's decoders accept; libbz2 writes at most 17
_WINDOW = MAX_FORMAT_LENGTH

_CHUNK = 1 << 18             # bits of a stream that the symbol loop holds as a Python list at a time


def _unpacked(data):
    """(bits, windows) of `data` as numpy arrays: bits[i] is bit i (MSB first), windows[i] the 20 bits from i on
    (zero padded).  Five bytes per bit of the stream; the loops below turn short stretches into Python lists."""
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8))
    padded = np.concatenate([bits, np.zeros(_WINDOW, dtype=np.uint8)]).astype(np.uint32)
    windows = np.zeros(len(bits), dtype=np.uint32)
    for k in range(_WINDOW):
        windows |= padded[k:k + len(bits)] << (_WINDOW - 1 - k)
    return bits, windows


class _Reader:
    def __init__(self, bits, pos):
        self.bits = bits
        self.pos = pos

    def get(self, n):
        if self.pos + n > len(self.bits):
            raise ValueError("the stream ends inside a field")
        v = 0
        for b in self.bits[self.pos:self.pos + n].tolist():
            v = (v << 1) | b
        self.pos += n
        return v


def _decode_table(lengths):
    """(longest, symbol by prefix, length by prefix) of the canonical code: a prefix is the next `longest` bits.
    A prefix no code covers (an incomplete code) maps to symbol -1."""
    longest = max(lengths)
    codes = bz2enc.canonical_codes(lengths)
    symbol = np.full(1 << longest, -1, dtype=np.int32)
    length = np.zeros(1 << longest, dtype=np.int32)
    for s, (l, c) in enumerate(zip(lengths, codes)):
        lo = c << (longest - l)
        hi = lo + (1 << (longest - l))
        if hi > (1 << longest):
            raise ValueError("the code lengths are oversubscribed")
        symbol[lo:hi] = s
        length[lo:hi] = l
    return longest, symbol.tolist(), length.tolist()


def parse_block(data, bit_offset):
    """The block whose 48-bit magic starts at `bit_offset`, taken apart without judging it (beyond what makes it
    undecodable: ValueError).  Returns a dict: crc, randomized, orig_ptr, used (sorted byte values of the 16 x 16 map),
    n_groups, n_selectors, selectors (their MTF undone), lengths (one list per table), symbols (MTF positions + 1,
    RUNA = 0, RUNB = 1, end of block = len(used) + 1, which ends the list), header_bits (magic up to the first symbol)
    and end_bit (the bit behind the end-of-block code)."""
    return _parse_block(*_unpacked(data), bit_offset)


def _parse_block(bits, windows, bit_offset):
    r = _Reader(bits, bit_offset)
    if r.get(48) != MAGIC_BLOCK:
        raise ValueError("no block magic at bit %d" % bit_offset)
    out = {"bit_offset": bit_offset, "crc": r.get(32), "randomized": r.get(1), "orig_ptr": r.get(24)}
    ranges = r.get(16)
    used = []
    for i in range(16):
        if (ranges >> (15 - i)) & 1:
            row = r.get(16)
            used += [16 * i + j for j in range(16) if (row >> (15 - j)) & 1]
    if not used:
        raise ValueError("no byte value in use")
    alpha = len(used) + 2
    n_groups = r.get(3)
    n_selectors = r.get(15)
    if not 2 <= n_groups <= 6 or n_selectors < 1:
        raise ValueError("bad table or selector count")
    order = list(range(n_groups))
    selectors = []
    for _ in range(n_selectors):
        j = 0
        while r.get(1):
            j += 1
            if j >= n_groups:
                raise ValueError("selector beyond the table count")
        selectors.append(order.pop(j))
        order.insert(0, selectors[-1])
    lengths = []
    for _ in range(n_groups):
        cur = r.get(5)
        table = []
        for _ in range(alpha):
            while r.get(1):
                cur += -1 if r.get(1) else 1
            if not 1 <= cur <= MAX_FORMAT_LENGTH:
                raise ValueError("code length %d" % cur)
            table.append(cur)
        lengths.append(table)
    out.update(used=used, n_groups=n_groups, n_selectors=n_selectors, selectors=selectors, lengths=lengths,
               header_bits=r.pos - bit_offset)
    decoders = [_decode_table(t) for t in lengths]
    symbols = []
    pos = r.pos
    eob = alpha - 1
    total = len(bits)
    done = False
    base, chunk = pos, windows[pos:pos + _CHUNK].tolist()
    for sel in selectors:
        longest, symbol, length = decoders[sel]
        shift = _WINDOW - longest
        for _ in range(GROUP_SIZE):
            k = pos - base
            if k >= len(chunk):
                if pos >= total:
                    raise ValueError("the stream ends inside the symbols")
                base, chunk, k = pos, windows[pos:pos + _CHUNK].tolist(), 0
            w = chunk[k] >> shift
            s = symbol[w]
            if s < 0:
                raise ValueError("bits at %d match no code of table %d" % (pos, sel))
            pos += length[w]
            symbols.append(s)
            if s == eob:
                done = True
                break
        if done:
            break
    if not done:
        raise ValueError("the selectors run out before the end of block")
    if pos > total:
        raise ValueError("the stream ends inside the symbols")
    out.update(symbols=symbols, end_bit=pos)
    return out


def parse_stream(data):
    """A single-stream file: {level, blocks (parse_block dicts), eos_bit, stream_crc, end_bit}."""
    if data[:3] != b"BZh" or not 0x31 <= data[3] <= 0x39:
        raise ValueError("no stream header")
    bits, windows = _unpacked(data)
    pos = 32
    blocks = []
    while True:
        magic = _Reader(bits, pos).get(48)
        if magic == MAGIC_EOS:
            break
        blocks.append(_parse_block(bits, windows, pos))
        pos = blocks[-1]["end_bit"]
    crc = _Reader(bits, pos + 48).get(32)
    return {"level": data[3] - 0x30, "blocks": blocks, "eos_bit": pos, "stream_crc": crc, "end_bit": pos + 80}


# ----------------------------------------------------------------------------------------------- plain references

def rle1_libbz2(data):
    """bzip2's first run-length stage as libbz2 writes it: runs of one byte value are cut into pieces of at most 255
    bytes; a piece of 4 or more becomes the byte four times and a count of 0..251.  (bz2enc.rle1 writes counts up to
    255, which the format allows and libbz2 never does.)"""
    out = bytearray()
    i, n = 0, len(data)
    while i < n:
        c = data[i]
        j = i + 1
        stop = min(n, i + 255)
        while j < stop and data[j] == c:
            j += 1
        piece = j - i
        if piece >= 4:
            out += bytes([c, c, c, c, piece - 4])
        else:
            out += bytes([c]) * piece
        i = j
    return bytes(out)


def bwt_plain(s):
    """(L column, origPtr) from the sorted rotations of `s`; a few thousand bytes at most."""
    return bz2enc.bwt(s)


def _flush_run(run, symbols):
    while run > 0:            # bijective base 2: RUNA counts 1, RUNB 2, weights 1, 2, 4, ...
        if run & 1:
            symbols.append(0)
            run = (run - 1) >> 1
        else:
            symbols.append(1)
            run = (run - 2) >> 1


def mtf_symbols(last, used):
    """Move-to-front over the list `used` (sorted byte values), runs of position 0 as RUNA/RUNB, end of block last."""
    lst = list(used)
    symbols = []
    run = 0
    for b in last:
        if lst[0] == b:
            run += 1
            continue
        _flush_run(run, symbols)
        run = 0
        p = lst.index(b)
        symbols.append(p + 1)
        del lst[p]
        lst.insert(0, b)
    _flush_run(run, symbols)
    symbols.append(len(used) + 1)
    return symbols


def zero_runs(symbols):
    """The lengths of the runs of MTF position 0 that the RUNA/RUNB symbols of `symbols` stand for, in order."""
    runs = []
    run, weight = 0, 1
    for s in symbols:
        if s <= 1:
            run += weight << s
            weight <<= 1
        elif run:
            runs.append(run)
            run, weight = 0, 1
    return runs


def unmtf(symbols, used):
    """The L column that `symbols` (with their end of block) stand for: the inverse of mtf_symbols."""
    lst = list(used)
    eob = len(used) + 1
    out = bytearray()
    run, weight = 0, 1
    for k, s in enumerate(symbols):
        if s <= 1:
            run += weight << s
            weight <<= 1
            continue
        if run:
            out += bytes([lst[0]]) * run
            run, weight = 0, 1
        if s == eob:
            if k != len(symbols) - 1:
                raise ValueError("symbols behind the end of block")
            return bytes(out)
        b = lst.pop(s - 1)
        lst.insert(0, b)
        out.append(b)
    raise ValueError("no end of block")


def huffman_depth(freq):
    """The deepest leaf of an unlimited-depth Huffman code over `freq` (a frequency of 0 counts as 1)."""
    heap = [(f if f else 1, 0) for f in freq]
    if len(heap) < 2:
        return 1
    heapq.heapify(heap)
    while len(heap) > 1:
        wa, da = heapq.heappop(heap)
        wb, db = heapq.heappop(heap)
        heapq.heappush(heap, (wa + wb, max(da, db) + 1))
    return heap[0][1]


def n_groups_for(n_mtf):
    """libbz2's table count for a block of n_mtf symbols (end of block included)."""
    for bound, groups in ((200, 2), (600, 3), (1200, 4), (2400, 5)):
        if n_mtf < bound:
            return groups
    return 6


def kraft_17(lengths):
    """Kraft sum of the code in units of 2**-17: a complete prefix code gives exactly 2**17."""
    return sum(1 << (17 - l) for l in lengths)


def group_costs(lengths, symbols):
    """costs[t][g]: the bits of 50-symbol group g under table t."""
    sym = np.asarray(symbols, dtype=np.int64)
    starts = np.arange(0, len(sym), GROUP_SIZE)
    return np.stack([np.add.reduceat(np.asarray(t, dtype=np.int64)[sym], starts) for t in lengths])


def is_proper_power(s):
    """s == u * k for a shorter u: its rotations are not all different, so origPtr has more than one right value."""
    return len(s) > 1 and s in (s + s)[1:-1]


def combine_crc(stream_crc, block_crc):
    return (((stream_crc << 1) | (stream_crc >> 31)) ^ block_crc) & 0xFFFFFFFF


# ----------------------------------------------------------------------------------------------- inputs with a property

def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def find_n_mtf(target, seed=1):
    """A prefix of seeded noise whose libbz2 block (level 9) has exactly `target` symbols, or None.  Noise of n bytes
    gives about n symbols, so lengths around the target are tried one by one."""
    source = noise(target + 64, seed)
    for n in range(max(1, target - 24), target + 64):
        enc = bz2.compress(source[:n], 9)
        if len(parse_block(enc, 32)["symbols"]) == target:
            return source[:n]
    return None


def geometric_source(n=1_200_000, seed=17, ratio=0.55, values=40):
    """Bytes drawn with p_i proportional to ratio**i over `values` byte values: frequencies steep enough for an
    unlimited Huffman code of a 900 kB block to go deeper than 17."""
    p = ratio ** np.arange(values)
    rng = np.random.default_rng(seed)
    return rng.choice(values, size=n, p=p / p.sum()).astype(np.uint8).tobytes()


def capped_tables(block):
    """The tables of a parsed block whose longest code is 17 although a Huffman code over the symbols of their own
    groups would go deeper: where the encoder's length cap took effect."""
    alpha = len(block["used"]) + 2
    capped = []
    for t, lengths in enumerate(block["lengths"]):
        freq = [0] * alpha
        for g, sel in enumerate(block["selectors"]):
            if sel == t:
                for s in block["symbols"][g * GROUP_SIZE:(g + 1) * GROUP_SIZE]:
                    freq[s] += 1
        if max(lengths) == 17 and huffman_depth(freq) >= 18:
            capped.append(t)
    return capped


# ----------------------------------------------------------------------------------------------- what holds of every block

BWT_PLAIN_LIMIT = 4000      # bwt_plain sorts whole rotations


def check_block(block, payload, last, pre, where=""):
    """What must hold of any block that libbz2 could have written, given its parse, the bytes it stands for and the
    oracle's L column and pre-RLE1 bytes of it.  tests/test_bz2parse.py shows that libbz2's own blocks pass."""
    symbols, used = block["symbols"], block["used"]
    n_mtf = len(symbols)
    assert block["randomized"] == 0, where
    assert pre == rle1_libbz2(payload), "%s: RLE1 bytes differ from the plain reference" % where
    assert used == sorted(set(pre)), "%s: byte values in use %r, in the RLE1 bytes %r" % (where, used, sorted(set(pre)))
    assert unmtf(symbols, used) == last, "%s: the symbols do not give the L column" % where
    assert symbols == mtf_symbols(last, used), "%s: the symbols differ from the plain MTF of the L column" % where
    if len(pre) <= BWT_PLAIN_LIMIT:
        want_last, want_ptr = bwt_plain(pre)
        assert last == want_last, "%s: the L column differs from the sorted rotations'" % where
        if not is_proper_power(pre):
            assert block["orig_ptr"] == want_ptr, "%s: origPtr %d, plain BWT %d" % (where, block["orig_ptr"], want_ptr)
    assert block["n_groups"] == n_groups_for(n_mtf), "%s: %d tables for %d symbols" % (where, block["n_groups"], n_mtf)
    assert block["n_selectors"] == -(-n_mtf // GROUP_SIZE), \
        "%s: %d selectors for %d symbols" % (where, block["n_selectors"], n_mtf)
    assert all(s < block["n_groups"] for s in block["selectors"]), where
    for t, lengths in enumerate(block["lengths"]):
        assert len(lengths) == len(used) + 2, where
        assert min(lengths) >= 1 and max(lengths) <= 17, "%s: table %d has lengths %d..%d" % (
            where, t, min(lengths), max(lengths))
        assert kraft_17(lengths) == 1 << 17, "%s: table %d is not a complete code" % (where, t)
