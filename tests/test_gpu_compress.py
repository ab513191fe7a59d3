"""compress / compress_many on the MI355X: round trips through libbz2 (every block CRC and the stream CRC are checked),
decompress_many and the reader; outputs independent of how blocks fall into launches; the block index against the
reader's and libbz2's; the compression ratio against libbz2's; reuse of the kept context."""
import bz2
import io
import random

import pytest

import datagen

pytestmark = pytest.mark.gpu


def _runs_at_cut(level, run, byte=b"z"):
    """A run of `run` bytes placed so that it starts where the first block's RLE1 fill limit is reached."""
    limit = 100000 * level - 19
    head = bytes(i % 251 for i in range(limit - 2))     # no runs: one RLE1 byte per input byte
    return head + byte * run + b"tail" * 10


def _reader_read(native, data):
    with native.open(io.BytesIO(data), 1) as f:
        out = f.read()
        assert f.streams_verified() >= 1
        return out


def _check_round_trip(native, inputs, level, **kw):
    outs = native.compress_many(inputs, compresslevel=level, **kw)
    assert len(outs) == len(inputs)
    for x, out in zip(inputs, outs):
        assert out[:4] == b"BZh" + str(level).encode()
        assert bz2.decompress(out) == x
    back = native.decompress_many(outs)
    for x, y in zip(inputs, back):
        assert x == y
    return outs


@pytest.fixture(scope="module")
def edge_inputs():
    return {
        "empty": b"",
        "one": b"q",
        "all256": bytes(range(256)),
        "runs": datagen.runs(400_000),
        "run3": b"ab" + b"c" * 3 + b"d",
        "run4": b"c" * 4,
        "run5": b"c" * 5,
        "run255": b"x" * 255 + b"y",
        "run256": b"x" * 256,
        "run259": b"x" * 259 + b"x",
        "A5M": b"A" * 5_000_000,
        "stripes": datagen.ab_stripes(300_000, 7),
        "abc": b"abc" * 400_000,
    }


@pytest.mark.parametrize("level", [1, 9])
def test_round_trip_edge_cases(native, edge_inputs, level):
    names = list(edge_inputs)
    outs = _check_round_trip(native, [edge_inputs[k] for k in names], level)
    # the reader at parallelization 1 checks the stream CRC too
    for name in ("one", "runs", "abc", "A5M"):
        assert _reader_read(native, outs[names.index(name)]) == edge_inputs[name]


@pytest.mark.parametrize("run", [3, 4, 5, 255, 256, 259, 300_000])
def test_runs_at_block_cut(native, run):
    x = _runs_at_cut(1, run)
    out, index = native.compress_many([x], compresslevel=1, return_index=True)[0]
    assert bz2.decompress(out) == x
    ref = bz2.compress(x, 1)
    with native.open(io.BytesIO(ref), 0) as f:
        want = sorted(f.block_offsets().values())
    assert sorted(index.values()) == want


def test_text_every_level(native):
    x = datagen.text_like(2_000_000)
    for level in range(1, 10):
        out = native.compress(x, compresslevel=level)
        assert bz2.decompress(out) == x


def test_random_and_multi_block(native):
    r = datagen.random_bytes(350_000)
    t = datagen.text_like(450_000, seed=11)
    outs = _check_round_trip(native, [r, t], 1)
    with native.open(io.BytesIO(outs[1]), 1) as f:
        assert len(f.block_offsets()) >= 3 + 2      # at least three data blocks at level 1


def test_many_mixed_buffers(native):
    rng = random.Random(7)
    inputs = []
    for i in range(300):
        kind = i % 5
        n = rng.randrange(0, 40_000)
        if kind == 0:
            inputs.append(datagen.text_like(n, seed=i))
        elif kind == 1:
            inputs.append(datagen.random_bytes(n, seed=i))
        elif kind == 2:
            inputs.append(datagen.runs(n, seed=i))
        elif kind == 3:
            inputs.append(bytes([i % 256]) * n)
        else:
            inputs.append(b"")
    inputs.append(datagen.text_like(250_000, seed=999))   # three blocks at level 1
    _check_round_trip(native, inputs, 1)
    _check_round_trip(native, inputs[:120], 6)


def test_launch_independence_and_determinism(native):
    inputs = [datagen.text_like(260_000, seed=3), b"", datagen.runs(210_000, seed=5), b"z" * 123_457,
              datagen.random_bytes(150_000, seed=9), datagen.text_like(30_000, seed=4)]
    base = native.compress_many(inputs, compresslevel=1, max_launch_blocks=0)
    for cap in (1, 3, 0):
        assert native.compress_many(inputs, compresslevel=1, max_launch_blocks=cap) == base
    for x, out in zip(inputs, base):
        assert bz2.decompress(out) == x


def test_index(native):
    inputs = [datagen.text_like(520_000, seed=21), b"", b"k", datagen.runs(330_000, seed=22)]
    pairs = native.compress_many(inputs, compresslevel=1, return_index=True)
    for x, (out, index) in zip(inputs, pairs):
        with native.open(io.BytesIO(out), 0) as f:
            assert f.block_offsets() == index
        with native.open(io.BytesIO(bz2.compress(x, 1)), 0) as f:
            assert sorted(f.block_offsets().values()) == sorted(index.values())
    x, (out, index) = inputs[0], pairs[0]
    rng = random.Random(5)
    with native.open(io.BytesIO(out), 4) as f:
        f.set_block_offsets(index)
        ranges = []
        for _ in range(40):
            a = rng.randrange(0, len(x))
            ranges.append((a, rng.randrange(1, 30_000)))
        got = f.read_ranges(ranges)
        for (a, n), g in zip(ranges, got):
            assert bytes(g) == x[a:a + n]


@pytest.mark.parametrize("level", [1, 9])
def test_ratio_against_libbz2(native, level):
    text = datagen.enwik_like(8_000_000)
    ours = native.compress(text, compresslevel=level)
    assert bz2.decompress(ours) == text
    assert len(ours) <= 1.01 * len(bz2.compress(text, level))
    rnd = datagen.random_bytes(2_000_000, seed=77)
    ours = native.compress(rnd, compresslevel=level)
    assert len(ours) <= 1.005 * len(bz2.compress(rnd, level))


def test_levels_rejected(native):
    for bad in (0, 10, -1, 2.5, True):
        with pytest.raises(ValueError):
            native.compress_many([b"x"], compresslevel=bad)


def test_reuse_and_memory(native):
    from indexed_bzip2_amd import _native as N
    dec = N.Decoder(device=0)
    try:
        enc = bz2.compress(datagen.text_like(300_000), 9)
        dec.decompress_buffers([enc])
        assert dec.encoder_memory() == 0           # a context that only decodes has no encoder scratch
        scratch = dec.device_memory()["scratch_bytes"]
        x = datagen.text_like(700_000, seed=31)
        res, total = dec.compress_buffers([x, b"abc"], 1)
        out = dec.copy_output(res[0]["output_offset"], res[0]["compressed_size"])
        assert bz2.decompress(out) == x
        assert dec.encoder_memory() > 0
        assert dec.device_memory()["scratch_bytes"] == scratch
        res2, total2 = dec.decompress_buffers([out, enc])
        assert res2[0]["status"] == 0 and res2[1]["status"] == 0
        assert dec.copy_output(res2[0]["output_offset"], res2[0]["decoded_size"]) == x
        res3, _ = dec.compress_buffers([x], 1)
        assert dec.copy_output(res3[0]["output_offset"], res3[0]["compressed_size"]) == out
    finally:
        dec.close()
    # the module-level functions keep using the device's one context
    from indexed_bzip2_amd import buffers as B
    native.compress(b"warm")
    count = len(B._contexts)
    native.compress_many([b"a", b"b"])
    native.decompress_many([native.compress(b"c")])
    assert len(B._contexts) == count


def test_worst_case_periodic_level9(native):
    x = b"abcdefgh" * 112_000    # one block of 896 000 bytes, every rotation tied for ~18 doubling rounds
    out = native.compress(x, compresslevel=9)
    assert bz2.decompress(out) == x
