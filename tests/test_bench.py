"""bench.py --dump-outputs without a GPU: what it writes for a step's block records and decoded extents."""
import os

import numpy as np
import pytest

import bench


def _records(n):
    from indexed_bzip2_amd._native import BlockResult
    arr = (BlockResult * n)()
    for i in range(n):
        arr[i].decoded_size = 900_000 + i
        arr[i].computed_crc = 0xFFFFFFFF - i
        arr[i].encoded_offset_bits = (1 << 40) + 8 * i
        arr[i].status = 0
    return arr


@pytest.mark.parametrize("sizes", [[5 * 2**20 + 1000, 6 * 2**20 - 7], [3 * 2**20, 2**20 + 5]])
def test_dump_outputs(tmp_path, sizes):
    torch = pytest.importorskip("torch")
    total = sum(sizes)
    # every 4 KiB window of the decoded bytes starts with its own index, so a sampled window tells where it came from
    data = np.random.default_rng(3).integers(0, 256, total, dtype=np.uint8)
    n_windows = total // bench.DUMP_WINDOW
    heads = np.arange(n_windows, dtype="<u4").view(np.uint8).reshape(n_windows, 4)
    data[:n_windows * bench.DUMP_WINDOW].reshape(n_windows, bench.DUMP_WINDOW)[:, :4] = heads
    extents = [torch.from_numpy(part.copy()) for part in np.split(data, np.cumsum(sizes)[:-1])]

    bench.dump_outputs(str(tmp_path / "a"), _records(5), 3, extents)
    bench.dump_outputs(str(tmp_path / "b"), _records(5), 3, extents)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert "decoded_sample.npy" in names and "block_computed_crc.npy" in names and "block_status.npy" in names
    size = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        size += os.path.getsize(tmp_path / "a" / name)
    assert size <= 64 * 2**20

    assert np.load(tmp_path / "a" / "block_decoded_size.npy").tolist() == [900_000, 900_001, 900_002]
    assert np.load(tmp_path / "a" / "block_computed_crc.npy").tolist() == [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD]
    assert np.load(tmp_path / "a" / "block_encoded_offset_bits.npy").tolist() == [(1 << 40) + 8 * i for i in range(3)]

    sample = np.load(tmp_path / "a" / "decoded_sample.npy")
    if total <= bench.DUMP_WINDOW * bench.DUMP_WINDOWS:
        assert np.array_equal(sample, data.astype(np.float32))
        return
    windows = sample.astype(np.uint8).reshape(bench.DUMP_WINDOWS, bench.DUMP_WINDOW)
    where = windows[:, :4].copy().view("<u4").ravel()
    assert len(set(where.tolist())) == bench.DUMP_WINDOWS and np.all(np.diff(where.astype(np.int64)) > 0)
    for w, k in zip(windows, where):
        assert np.array_equal(w, data[k * bench.DUMP_WINDOW:(k + 1) * bench.DUMP_WINDOW])
    # the positions are those bench.dump_positions names (in the first case the sampled window 1280 straddles the extents)
    assert np.array_equal(sample, data[bench.dump_positions(total)].astype(np.float32))
