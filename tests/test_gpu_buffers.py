"""decompress_many / decompress_many_to_tensor / decompress (mi355x_bz2_decompress_buffers) on an MI355X.

Every buffer must decode to bz2.decompress(buffer) and to what the reader returns at parallelization 1; a damaged or
truncated buffer must fail with the reader's status wherever it sits in a batch, and its neighbours must not notice."""
import bz2
import io
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import FIXTURES, ROOT

pytestmark = pytest.mark.gpu

OK, ERR_EOF, ERR_CRC, ERR_STREAM_HEADER, ERR_STREAM_CRC = 0, 1, 15, 16, 17


def reader_result(native, data):
    """(status, bytes, bit offset named in the message or None) of the reader at parallelization 1."""
    try:
        with native.open(io.BytesIO(bytes(data)), 1) as f:
            return OK, f.read(), None
    except native.Bz2Error as e:
        m = re.search(r"bit offset (\d+)", str(e))
        return e.status, b"", int(m.group(1)) if m else None


def block_offsets(native, data):
    return native.find_magic(bytes(data), native._native.MAGIC_BLOCK)


def eos_offsets(native, data):
    return native.find_magic(bytes(data), native._native.MAGIC_EOS)


def silesia(n, seed):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import silesia_like
    return bytes(silesia_like.generate(n, seed=seed, threads=1))


@pytest.fixture(scope="module")
def corpus():
    """About 300 seeded buffers: every level, empty to several 900 kB blocks, multi-stream, golden fixtures, exotic
    encoder output, an RLE-maximal block."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import datagen
    rng = random.Random(0xB0FFE2)
    big = silesia(3_200_000, 7)
    raws = []
    for i in range(240):
        kind = i % 6
        size = [0, rng.randrange(1, 300), rng.randrange(300, 40_000), rng.randrange(40_000, 400_000),
                rng.randrange(400_000, 1_000_000), rng.randrange(1_000_000, 3_000_000)][kind]
        at = rng.randrange(0, len(big) - size + 1)
        raws.append((big[at:at + size], rng.randrange(1, 10)))
    bufs = [(bz2.compress(raw, level), raw) for raw, level in raws]
    for i in range(30):   # two and three streams
        parts = [raws[rng.randrange(len(raws))] for _ in range(2 + i % 2)]
        bufs.append((b"".join(bz2.compress(raw, level) for raw, level in parts), b"".join(raw for raw, _ in parts)))
    for name in sorted(os.listdir(FIXTURES)):
        if name.endswith(".bz2"):
            raw_path = os.path.join(FIXTURES, name[:-4])
            enc = open(os.path.join(FIXTURES, name), "rb").read()
            bufs.append((enc, open(raw_path, "rb").read() if os.path.exists(raw_path) else bz2.decompress(enc)))
    for name, (raw, enc) in sorted(datagen.exotic_streams().items()):
        bufs.append((enc, raw))
    # an RLE-maximal block: 900 000 bytes of 0xFF after the first run-length stage, i.e. runs of 4 + 255 bytes, decode to
    # 46.6 MB (the most a level-9 block can produce); the rest of the input goes into a second block
    rle = b"\xff" * 47_000_000
    bufs.append((bz2.compress(rle, 9), rle))
    return bufs


@pytest.mark.parametrize("max_launch_blocks", [1, 7, 0])
def test_parity(native, corpus, max_launch_blocks):
    encs = [e for e, _ in corpus]
    out = native.decompress_many(encs, max_launch_blocks=max_launch_blocks)
    assert len(out) == len(corpus)
    for i, ((enc, raw), got) in enumerate(zip(corpus, out)):
        assert got == raw == bz2.decompress(enc), i
    if max_launch_blocks == 0:
        for i, (enc, raw) in enumerate(corpus[::5]):   # the reader at parallelization 1 agrees
            assert reader_result(native, enc) == (OK, raw, None), i


def test_input_types(native, corpus):
    enc, raw = corpus[3]
    kinds = [enc, bytearray(enc), memoryview(enc), np.frombuffer(enc, dtype=np.uint8)]
    assert native.decompress_many(kinds) == [raw] * 4
    assert native.decompress(enc) == raw


def cut_points(native, enc):
    """{name: (the buffer cut there, bit offset of the block or header where reading it fails)} for a multi-block
    single-stream buffer."""
    blocks = block_offsets(native, enc)
    eos = eos_offsets(native, enc)[-1]
    assert len(blocks) >= 3
    cuts = {
        "stream header": (2, 0),
        # header, symbol map and about 2 000 selectors of a 100 kB block lie in front of its code lengths
        "code lengths": ((blocks[1] + 48 + 32 + 1 + 24 + 16 + 16 * 16 + 3 + 15 + 3_600) // 8, blocks[1]),
        "near end-of-block": ((blocks[2] - 12) // 8, blocks[1]),
        # the last data block ends at `eos`: a cut in front of that bit truncates it, one at it leaves the header
        "before end-of-stream": (eos // 8, eos if eos % 8 == 0 else blocks[-1]),
        "inside end-of-stream": (eos // 8 + 5, eos),
    }
    return {name: (enc[:at], offset) for name, (at, offset) in cuts.items()}


def test_per_block_end(native):
    raw = silesia(2_400_000, 11)
    enc = bz2.compress(raw, 1)          # 100 kB blocks: many blocks per buffer
    valid = bz2.compress(raw[:500_000], 9)
    ff = b"\xff" * 4096
    dec = native.buffers._decoder(-1)[0]
    for name, (cut, want_offset) in cut_points(native, enc).items():
        want_status, _, reader_offset = reader_result(native, cut)
        if name == "stream header":
            # the reader reads bytes without a block magic as an empty file; a buffer without a header fails here
            assert want_status == OK
            want_status = ERR_STREAM_HEADER
        assert want_status != OK, name
        assert reader_offset in (None, want_offset), (name, reader_offset, want_offset)
        for batch, index in (([valid, cut], 1), ([cut, valid], 0), ([cut, ff, valid], 0)):
            out, status = native.decompress_many(batch, return_status=True)
            assert status[index] == want_status, (name, index, status)
            results, _ = dec.decompress_buffers(batch)
            assert results[index]["status"] == want_status, (name, index)
            assert results[index]["error_offset_bits"] == want_offset, (name, index, results[index])
            assert results[index]["decoded_size"] == 0
            for j, buf in enumerate(batch):
                if buf is valid:
                    assert status[j] == OK and out[j] == bz2.decompress(valid), name
                elif buf is ff:
                    assert status[j] == ERR_STREAM_HEADER and results[j]["error_offset_bits"] == 0, name


def test_damage(native):
    raw = silesia(1_500_000, 13)
    enc = bytearray(bz2.compress(raw, 2))
    blocks = block_offsets(native, enc)
    eos = eos_offsets(native, enc)[-1]
    before, after = bz2.compress(b"before " * 1000, 9), bz2.compress(b"after " * 3000, 9)

    def check(buf, want_status, want_offset=None, want_bytes=None, garbage=0):
        results, total = native.buffers._decoder(-1)[0].decompress_buffers([before, bytes(buf), after])
        status, got, _ = reader_result(native, buf)
        if want_status is None:   # whatever the reader reports, as long as it fails
            assert status != OK
            want_status = status
        assert results[1]["status"] == want_status == status, (results[1], status)
        if want_offset is not None:
            assert results[1]["error_offset_bits"] == want_offset
        assert results[1]["trailing_garbage"] == garbage
        out = native.decompress_many([before, bytes(buf), after], return_status=True)[0]
        assert out[0] == bz2.decompress(before) and out[2] == bz2.decompress(after)
        if want_bytes is not None:
            assert out[1] == want_bytes == got

    flipped = bytearray(enc)
    flipped[(blocks[1] + 48 + 8) // 8] ^= 0x10      # the block's stored CRC
    check(flipped, ERR_CRC, want_offset=blocks[1])
    flipped = bytearray(enc)
    flipped[(blocks[1] + 200_000) // 8] ^= 0x10     # deep in its Huffman data
    check(flipped, None, want_offset=blocks[1])
    wrong = bytearray(enc)
    wrong[(eos + 48) // 8] ^= 0x01   # the stored stream CRC
    check(wrong, ERR_STREAM_CRC)
    check(b"BZx9" + enc[4:], ERR_STREAM_HEADER, want_offset=0)
    check(enc + b"garbage at the end" * 10, OK, want_bytes=raw, garbage=1)
    check(b"", OK, want_bytes=b"")   # as the reader and bz2.decompress


DEVICE_CHILD = r"""
import bz2, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
torch.zeros(1, device="cuda")
import indexed_bzip2_amd as m
raws = [bytes(range(256)) * (7 * i) + b"tail %d" % i for i in range(60)]
encs = [bz2.compress(r, 1 + i % 9) for i, r in enumerate(raws)]
encs[7] = b""                       # 0 bytes in, 0 bytes out
raws[7] = b""
data, offsets = m.decompress_many_to_tensor(encs)
assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
assert offsets.dtype == torch.int64 and not offsets.is_cuda and len(offsets) == len(encs) + 1
assert offsets.tolist() == [int(x) for x in np.cumsum([0] + [len(r) for r in raws])]
assert bytes(data.cpu().numpy()) == b"".join(raws)
encs[9] = encs[9][:-3]              # cut: fails, takes 0 bytes
data, offsets, status = m.decompress_many_to_tensor(encs, return_status=True)
assert status[9] != 0 and (status[:9] == 0).all() and (status[10:] == 0).all()
assert offsets[10] == offsets[9]
assert bytes(data.cpu().numpy()) == b"".join(r for i, r in enumerate(raws) if i != 9)
try:
    m.decompress_many_to_tensor(encs)
    raise AssertionError("no error")
except m.Bz2Error as e:
    assert "buffer 9" in str(e), str(e)
# device=-1 and the explicit ordinal name the same device: one kept context for every entry point
assert m.decompress_many(encs[:3]) == raws[:3]
assert m.decompress(encs[0], device=torch.cuda.current_device()) == raws[0]
assert len(m.buffers._contexts) == 1, m.buffers._contexts
print("device buffers ok")
"""


def test_device_output(native):
    run = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "device buffers ok" in run.stdout


def test_output_functions_after_call(native, corpus):
    """The call's result is what copy_output / gather_output / output_device_ptr address; the background copy of the
    double-buffered batch output refuses it instead of copying a launch's ragged bytes."""
    import ctypes
    encs = [e for e, _ in corpus[:30]]
    want = b"".join(raw for _, raw in corpus[:30])
    dec = native.buffers._decoder(-1)[0]
    results, total = dec.decompress_buffers(encs)
    assert total == len(want)
    assert dec.copy_output(0, total) == want
    assert dec.gather_output([(r["output_offset"], r["output_offset"], r["decoded_size"]) for r in results]) == want
    buf = (ctypes.c_ubyte * max(1, total))()
    rc = native.lib().mi355x_bz2_copy_output_begin(dec._h, 0, total, buf)
    assert rc == 103, rc   # MI355X_BZ2_ERR_INVALID_ARGUMENT
    assert b"decompress_buffers" in native.lib().mi355x_bz2_last_error(dec._h)
    assert dec.copy_output(0, total) == want   # still there
    # a batch afterwards owns the output again, and its background copy works
    enc = corpus[3][0]
    dec.set_input(enc)
    _, n = dec.decode_batch(native.find_magic(enc))
    dst = dec.copy_output_begin(0, n)
    dec.copy_output_end()
    assert bytes(dst)[:n] == corpus[3][1][:n]


def test_context_reuse(native, corpus):
    assert native.decompress_many([]) == []
    out, status = native.decompress_many([], return_status=True)
    assert out == [] and len(status) == 0
    encs = [e for e, _ in corpus[:40]]
    first = native.decompress_many(encs)
    dec = native.buffers._decoder(-1)[0]
    memory = dec.device_memory()
    second = native.decompress_many(encs)
    assert second == first
    assert dec.device_memory() == memory
