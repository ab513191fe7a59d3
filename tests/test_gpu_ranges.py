"""read_ranges / read_ranges_into (mi355x_bz2_reader_read_ranges) and the k_gather kernel under it
(mi355x_bz2_gather_output) on the GPU.

The file: the bench's Silesia-style generator (tools/silesia_like.py) at 20 MB, compressed in pieces with `bzip2 -9`
blocks and stitched into one stream (tools/bz2build.py), three such streams behind each other -- about 70 blocks, with two
stream boundaries.  Plus the golden fixtures `empty`, `1B`, `zeros` and `random-128KiB`.  Every result is compared with
slices of the raw bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, read_fixture

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

BASE_BYTES = 20_000_000
STREAMS = 3
RANGES = 500
MAX_RANGE = 3_000_000


@pytest.fixture(scope="module")
def corpus(native, tmp_path_factory):
    import bz2build
    import silesia_like
    threads = min(16, os.cpu_count() or 8)
    base = silesia_like.generate(BASE_BYTES, threads=threads)
    pieces = bz2build.compress_pieces(base, piece_size=900_000 * 4, level=9, threads=threads)
    enc, nblocks, _ = bz2build.stitch(pieces, 1, 9, native.find_magic)
    enc = enc * STREAMS
    raw = base.tobytes() * STREAMS
    path = tmp_path_factory.mktemp("ranges") / "silesia-like-3streams.bz2"
    path.write_bytes(enc)
    with native.open(str(path), parallelization=0) as f:
        index = f.block_offsets()
    assert 50 <= len(index) - 2 * STREAMS <= 110
    return str(path), enc, raw, index


def seeded_ranges(total, seed, count=RANGES):
    """Sizes 0 to 3 MB (a third of them short, some zero), offsets anywhere up to a little beyond the end."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        kind = k % 6
        size = 0 if kind == 0 else int(rng.integers(1, 70_000)) if kind < 3 else int(rng.integers(1, MAX_RANGE))
        offset = int(rng.integers(0, total + 1000))
        out.append((offset, size))
    return out


def data_blocks(index):
    """[(bits, next_bits, start, end)] of the data blocks of a complete index."""
    items = sorted(index.items())
    return [(b, nb, s, e) for (b, s), (nb, e) in zip(items, items[1:]) if e > s]


def needed_blocks(index, ranges, total):
    blocks = data_blocks(index)
    needed = set()
    for offset, size in ranges:
        end = min(offset + size, total)
        for bits, _, start, stop in blocks:
            if offset < end and start < end and offset < stop:
                needed.add(bits)
    return needed


@pytest.mark.parametrize("indexed", [True, False], ids=["imported-index", "on-the-fly"])
@pytest.mark.parametrize("parallelization", [1, 4, 0])
def test_random_ranges(native, corpus, parallelization, indexed):
    path, enc, raw, index = corpus
    total = len(raw)
    ranges = seeded_ranges(total, 0xAB5 + parallelization)
    with native.open(path, parallelization=parallelization) as f:
        if indexed:
            f.set_block_offsets(index)
        # a position inside the first stream, and the buffered reader's read-ahead behind it
        f.seek(1_234_567)
        assert f.read(1000) == raw[1_234_567:1_235_567]
        before = f.statistics()
        got = f.read_ranges(ranges)
        for (offset, size), data in zip(ranges, got):
            assert data == raw[offset:offset + size], (offset, size)
        # positionless: tell() and the next read() are as if the call had not happened
        assert f.tell() == 1_235_567
        assert f.read(300_000) == raw[1_235_567:1_535_567]
        after = f.statistics()
        if indexed:
            # each distinct block once, in as few launches as the batch size allows
            distinct = len(needed_blocks(index, ranges, total))
            cap = 512 if parallelization == 0 else parallelization
            decoded = after["blocks_decoded"] - before["blocks_decoded"]
            # (the read() behind may have launched blocks of its own: at most a window of look-ahead)
            assert decoded >= distinct
            assert after["batches"] - before["batches"] >= -(-distinct // cap)
        else:
            assert f.block_offsets_complete()
        assert f.block_offsets() == index


def test_each_block_once_per_call(native, corpus):
    """With an imported index and no read around the call, the statistics count exactly the call's launches."""
    path, enc, raw, index = corpus
    ranges = seeded_ranges(len(raw), 0x0CE, count=200)
    distinct = len(needed_blocks(index, ranges, len(raw)))
    for parallelization, cap in ((4, 4), (0, 512)):
        with native.open(path, parallelization=parallelization) as f:
            f.set_block_offsets(index)
            before = f.statistics()
            got = f.read_ranges(ranges)
            after = f.statistics()
            assert [len(g) for g in got] == [len(raw[o:o + s]) for o, s in ranges]
            assert after["blocks_decoded"] - before["blocks_decoded"] == distinct
            assert after["batches"] - before["batches"] == -(-distinct // cap)
            # a second call decodes them again (nothing is kept), and gives the same bytes
            assert f.read_ranges(ranges) == got


def test_gather_alignment(native, corpus):
    """Every source misalignment 0-15 against destination offsets that walk through all 16 residues, sizes 0-40 inside
    one block and across a block boundary, plus pieces long enough for several tiles; against copy_output slices."""
    path, enc, raw, index = corpus
    blocks = data_blocks(index)
    dec = native.Decoder(device=0)
    dec.set_input(enc)
    results, total = dec.decode_batch([blocks[0][0], blocks[1][0]])
    out = dec.copy_output(0, total)
    assert out == raw[:total]
    first = results[0]["decoded_size"]
    for crossing in (False, True):
        base = ((first - 24) & ~15) if crossing else 16 * 1000
        for sm in range(16):
            for dm in range(16):
                pieces = [(5, 0, dm)]          # a filler: the next pieces' destinations start at dm
                at = dm
                for size in list(range(41)) + [1000, 3 * 32768 + 13]:
                    src = base + sm if size < 1000 else base + sm - (size // 2 if crossing else 0)
                    pieces.append((src, at, size))
                    at += size
                got = dec.gather_output(pieces)
                want = b"".join(out[s:s + n] for s, _, n in pieces)
                assert got == want, (crossing, sm, dm)
    # pieces outside the output are refused
    with pytest.raises(native.Bz2Error):
        dec.gather_output([(total - 10, 0, 11)])
    dec.close()


def test_end_of_file_and_empty_ranges(native, corpus):
    path, enc, raw, index = corpus
    total = len(raw)
    offsets = [total - 10, total, total + 5, 0, 100, total - 1]
    sizes = [100, 7, 3, 0, 0, 1]
    with native.open(path, parallelization=4) as f:
        f.set_block_offsets(index)
        out = bytearray(b"\xab" * (sum(sizes) + 16))
        got = f.read_ranges_into(offsets, sizes, out)
        assert got.dtype == np.uint64
        assert list(got) == [10, 0, 0, 0, 0, 1]
        assert out[:10] == raw[-10:] and out[10:100] == b"\xab" * 90
        assert out[110] == raw[-1] and out[111:] == b"\xab" * 16
        assert out[100:110] == b"\xab" * 10
        # argument errors
        with pytest.raises(ValueError):
            f.read_ranges_into([0], [10], bytearray(9))
        with pytest.raises(ValueError):
            f.read_ranges_into([0, 1], [10], bytearray(20))
        with pytest.raises(ValueError):
            f.read_ranges([(-1, 10)])
        with pytest.raises(ValueError):
            f.read_ranges([(0, -10)])
        assert f.read_ranges([]) == []
    with pytest.raises(ValueError):
        f.read_ranges([(0, 1)])


@pytest.mark.parametrize("name", ["empty", "1B", "zeros", "random-128KiB"])
def test_golden_fixtures(native, name, tmp_path):
    enc, raw = read_fixture(name)
    path = tmp_path / (name + ".bz2")
    path.write_bytes(enc)
    ranges = [(0, len(raw)), (0, len(raw) + 10), (len(raw) // 3, 1000), (len(raw), 1), (0, 0), (len(raw) // 2, 17)]
    for parallelization in (1, 0):
        with native.open(str(path), parallelization=parallelization) as f:
            assert f.read_ranges(ranges) == [raw[o:o + s] for o, s in ranges]
            assert f.tell() == 0
            assert f.read() == raw


def test_damaged_block(native, corpus, tmp_path):
    path, enc, raw, index = corpus
    blocks = data_blocks(index)
    bits, next_bits, start, stop = blocks[7]
    damaged = bytearray(enc)
    damaged[(bits + next_bits) // 16] ^= 0xFF
    bad = tmp_path / "damaged.bz2"
    bad.write_bytes(bytes(damaged))
    avoid = [(blocks[k][2] + 10, 5000) for k in (0, 3, 6, 8, 20)] + [(blocks[6][3] - 100, 100)]
    with native.open(str(bad), parallelization=4) as f:
        f.set_block_offsets(index)
        assert f.read_ranges(avoid) == [raw[o:o + s] for o, s in avoid]
        with pytest.raises(native.Bz2Error) as failure:
            f.read_ranges(avoid + [(start + 1000, 10)])
        assert failure.value.status != 0
        assert f"bit offset {bits}" in str(failure.value)
        # the reader stays usable
        assert f.read_ranges(avoid[:2]) == [raw[o:o + s] for o, s in avoid[:2]]


def test_bounded_residency(native, corpus, monkeypatch):
    path, enc, raw, index = corpus
    total = len(raw)
    # 20 ranges in the first stream: at most about a third of the file's blocks
    ranges = [(o % (total // STREAMS), min(s, 200_000)) for o, s in seeded_ranges(total, 0xB0B, count=20)]
    with native.open(path, parallelization=0) as f:
        f.set_block_offsets(index)
        want = f.read_ranges(ranges)
    assert want == [raw[o:o + s] for o, s in ranges]
    monkeypatch.setenv("MI355X_BZ2_INPUT_BUDGET", "1048576")
    for parallelization in (4, 0):
        with native.open(path, parallelization=parallelization) as f:
            f.set_block_offsets(index)
            before = f.statistics()
            assert before["input_resident"] == 0
            assert f.read_ranges(ranges) == want
            uploaded = f.statistics()["input_bytes_uploaded"] - before["input_bytes_uploaded"]
        needed = needed_blocks(index, ranges, total)
        compressed = sum((nb - b) // 8 + 1 for b, nb, _, _ in data_blocks(index) if b in needed)
        # each block's own bytes, the slack behind it and the alignment of its window: nothing else
        assert 0 < uploaded <= compressed + 24 * len(needed), (uploaded, compressed)
        assert uploaded < len(enc) / 2


CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process, as bench.py does
sys.path.insert(0, sys.argv[1])
import numpy as np
import indexed_bzip2_amd as m

path = sys.argv[2]
rng = np.random.default_rng(7)
with m.open(path, parallelization=0) as f:
    total = f.seek(0, 2)
    f.seek(0)
    offsets = [int(x) for x in rng.integers(0, total + 100, 300)] + [total - 5]
    sizes = [int(x) for x in rng.integers(0, 300_000, 300)] + [50]
    host = bytearray(b"\xcd" * (sum(sizes) + 3))
    counts_host = f.read_ranges_into(offsets, sizes, memoryview(host)[3:])
    for dm in (0, 3):
        dev = torch.full((sum(sizes) + 3,), 0xCD, dtype=torch.uint8, device="cuda")
        counts = f.read_ranges_into(offsets, sizes, dev[dm:])
        assert (counts == counts_host).all()
        got = bytes(dev.cpu().numpy())
        assert got[dm:] == bytes(host[3:]) + b"\xcd" * (3 - dm), dm
        assert got[:dm] == b"\xcd" * dm
    assert f.tell() == 0

    # k_gather into device memory at every destination misalignment, against the host path
    dec = m.Decoder(device=0)
    dec.set_input(open(path, "rb").read())
    offs = sorted(f.block_offsets())[:2]
    results, out_total = dec.decode_batch(offs)
    for sm in range(16):
        pieces, at = [], 0
        for dm in range(16):
            for size in (0, 1, 15, 16, 17, 40, 70_000):
                at += dm
                pieces.append((1600 + sm + 37 * dm, at, size))
                at += size
        dev = torch.zeros(at + 16, dtype=torch.uint8, device="cuda")
        dec.gather_output_to_device(pieces, dev.data_ptr())
        got = bytes(dev.cpu().numpy())
        want = bytearray(at + 16)
        for s, d, n in pieces:
            want[d:d + n] = dec.copy_output(s, n)
        assert got == bytes(want), sm
    dec.close()
print("device ranges ok")
"""


def test_device_destination(native, corpus):
    path, enc, raw, index = corpus
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, path], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "device ranges ok" in run.stdout
