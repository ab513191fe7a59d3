"""tests/bz2parse.py against libbz2 alone: every block that CPython's bz2 writes parses, its parsed stages agree with
the oracle's, and the properties that tests/test_gpu_compress_stages.py demands of the GPU encoder's blocks
(bz2parse.check_block) are true of the reference encoder's.  No GPU."""
import bz2
import functools

import pytest

import bz2enc
import bz2parse as P
import datagen


NMTF_TARGETS = (50, 51, 100, 101, 199, 200, 599, 600, 1199, 1200, 2399, 2400)

# name -> (how to make the input, level): made when its test runs, not when the file is collected
CORPUS = {
    "text-1": (lambda: datagen.text_like(260_000, seed=5), 1),                # three blocks
    "text-9": (lambda: datagen.text_like(260_000, seed=5), 9),
    "noise-1": (lambda: datagen.random_bytes(120_000, seed=6), 1),            # two blocks
    "noise-9": (lambda: datagen.random_bytes(40_000, seed=7), 9),
    "runs-1": (lambda: datagen.runs(150_000, seed=8), 1),
    "runs-9": (lambda: datagen.runs(60_000, seed=9), 9),
    "one-byte": (lambda: b"q", 9),
    "one-value": (lambda: b"\x00" * 4, 9),
    "all256": (lambda: bytes(range(256)), 9),
    "all256-twice": (lambda: bytes(range(256)) + bytes(range(255, -1, -1)), 1),
    "ab": (lambda: b"ab" * 300, 9),
    "long-run": (lambda: b"z" * 70_000 + b"y", 1),
    "stripes": (lambda: datagen.ab_stripes(30_000, 7), 9),
}
for _target in NMTF_TARGETS:      # bz2parse.find_n_mtf keeps what it found: the GPU tests use the same inputs
    CORPUS["nmtf-%d" % _target] = (functools.partial(P.find_n_mtf, _target), 9)


@pytest.mark.parametrize("name", list(CORPUS))
def test_libbz2_blocks(oracle, name):
    make, level = CORPUS[name]
    x = make()
    assert x is not None, "no input with that symbol count was found"
    enc = bz2.compress(x, level)
    stream = P.parse_stream(enc)
    assert stream["level"] == level
    assert [b["bit_offset"] for b in stream["blocks"]] == oracle.find_magic(enc)
    assert stream["eos_bit"] == oracle.find_magic(enc, oracle.MAGIC_EOS)[-1]
    assert len(enc) == (stream["end_bit"] + 7) // 8
    start, crc = 0, 0
    for i, block in enumerate(stream["blocks"]):
        d, payload, last, pre = oracle.decode_block(enc, block["bit_offset"], want_stages=True)
        assert d["status"] == 0
        assert payload == x[start:start + len(payload)]
        start += len(payload)
        P.check_block(block, payload, last, pre, where="%s block %d" % (name, i))
        assert block["orig_ptr"] == d["orig_ptr"]
        assert block["end_bit"] == d["encoded_offset_bits"] + d["encoded_size_bits"]
        assert block["crc"] == d["header_crc"] == bz2enc.crc32_bzip2(payload) ^ 0xFFFFFFFF
        crc = P.combine_crc(crc, block["crc"])
    assert start == len(x)
    assert stream["stream_crc"] == crc
    if name.startswith("nmtf-"):
        assert len(stream["blocks"][0]["symbols"]) == int(name[5:])
    if name in ("text-1", "noise-1"):
        assert len(stream["blocks"]) >= 2


def test_references_on_known_answers():
    assert P.rle1_libbz2(b"") == b""
    assert P.rle1_libbz2(b"aaa") == b"aaa"
    assert P.rle1_libbz2(b"aaaa") == b"aaaa\x00"
    assert P.rle1_libbz2(b"a" * 255 + b"b") == b"aaaa\xfbb"
    assert P.rle1_libbz2(b"a" * 256) == b"aaaa\xfba"
    assert P.rle1_libbz2(b"a" * 259) == b"aaaa\xfbaaaa\x00"
    assert bz2enc.rle1(b"a" * 259) == b"aaaa\xff"          # the format's widest count, which libbz2 never writes
    assert P.bwt_plain(b"banana") == (b"nnbaaa", 3)
    assert P.mtf_symbols(b"bbbaaa", [97, 98]) == [2, 1, 2, 1, 3]
    assert P.unmtf([2, 1, 2, 1, 3], [97, 98]) == b"bbbaaa"
    assert P.zero_runs([2, 1, 2, 0, 0, 3]) == [2, 3]
    assert P.huffman_depth([1, 1, 2, 4, 8]) == 4
    assert P.huffman_depth([0, 0]) == 1
    assert [P.n_groups_for(n) for n in (2, 199, 200, 599, 600, 1199, 1200, 2399, 2400)] == [2, 2, 3, 3, 4, 4, 5, 5, 6]
    assert P.is_proper_power(b"abab") and not P.is_proper_power(b"aba") and not P.is_proper_power(b"a")


def test_parser_rejects_what_it_cannot_decode():
    good = bz2enc.encode_block(b"hello hello hello")
    assert P.parse_block(good, 32)["symbols"][-1] == len(set(b"hello ")) + 1
    with pytest.raises(ValueError):
        P.parse_block(good, 33)
    with pytest.raises(ValueError):
        P.parse_block(bz2enc.encode_block(b"hello hello hello", faults={"drop_selectors": 1}) , 32)


def test_parser_reads_what_libbz2_never_writes(oracle):
    """20-bit codes, six tables for a short block, a declared value that never occurs: parsed, and check_block says no."""
    data = bytes(range(40)) * 3
    enc = bz2enc.encode_block(data, n_groups=6, declare_unused=(200,))
    block = P.parse_block(enc, 32)
    d, payload, last, pre = oracle.decode_block(enc, 32, want_stages=True)
    assert d["status"] == 0 and payload == data
    assert block["n_groups"] == 6 and 200 in block["used"] and max(map(max, block["lengths"])) > 17
    assert P.unmtf(block["symbols"], block["used"]) == last
    with pytest.raises(AssertionError):
        P.check_block(block, payload, last, pre)


def test_cap_precondition_on_libbz2():
    """The geometric source drives libbz2 itself into its 17-bit cap, and a 900 kB block parses quickly."""
    enc = bz2.compress(P.geometric_source(), 9)
    block = P.parse_block(enc, 32)
    assert len(P.capped_tables(block)) >= 2
    assert max(map(max, block["lengths"])) == 17
