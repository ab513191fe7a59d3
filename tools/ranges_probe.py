"""Developer probe: config 5 (1 000 random 64 KiB reads of the bench's 2 GiB Silesia-style file, block index imported)
three ways, each after a warm-up and repeated to show the spread:

  (a) 1 000 x seek + read(65536)                       -- one request at a time, as before read_ranges
  (b) one read_ranges_into of the same 1 000 ranges into host memory
  (c) the same into a torch.uint8 tensor on the GPU   -- the bytes never pass through the host

For each: wall milliseconds, distinct blocks decoded (the reader's blocks_decoded) and bytes moved D2H (for (a) the
decoded runs the reader copies out whole, estimated from the mean decoded block size; for (b) the requested bytes; for
(c) none).  One JSON line per measurement.  Run it under a time limit: `timeout -k 10 900 python tools/ranges_probe.py`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: F401  (first: one HIP runtime in the process, as bench.py does)
import numpy as np

import bench
import indexed_bzip2_amd as m

READ = 65536


def emit(**record):
    print(json.dumps(record), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parallelization", type=int, default=0)
    ap.add_argument("--loop-repeats", type=int, default=2, help="repeats of (a), which takes seconds each")
    args = ap.parse_args()

    path, enc, meta = bench.build_workload(2 * 1024**3, 214_748_364, bench.default_cache_dir(), 0, 1, lambda: None)
    t0 = time.perf_counter()
    with m.open(path, parallelization=0) as f:
        index = f.block_offsets()
        total = f.size()
    blocks = len(index) - 2
    emit(step="index", seconds=round(time.perf_counter() - t0, 2), blocks=blocks, decoded_bytes=total,
         compressed_bytes=len(enc))
    mean_block = total / blocks

    def ranges(seed):
        return [int(x) for x in np.random.default_rng(seed).integers(0, total - READ, args.reads)]

    def opened():
        f = m.open(path, parallelization=args.parallelization)
        f.set_block_offsets(index)
        return f

    # (a) the loop
    with opened() as f:
        for p in ranges(1)[:20]:
            f.seek(p)
            f.read(READ)
        for rep in range(args.loop_repeats):
            offsets = ranges(100 + rep)
            before = f.statistics()
            lat = []
            t = time.perf_counter()
            for p in offsets:
                t1 = time.perf_counter()
                f.seek(p)
                assert len(f.read(READ)) == READ
                lat.append(time.perf_counter() - t1)
            wall = time.perf_counter() - t
            decoded = f.statistics()["blocks_decoded"] - before["blocks_decoded"]
            emit(step="a: seek+read loop", repeat=rep, wall_ms=round(1e3 * wall, 1),
                 p50_ms=round(1e3 * float(np.median(lat)), 2), blocks_decoded=decoded,
                 d2h_bytes_estimate=int(decoded * mean_block))

    # (b) host destination, (c) device destination
    out_host = bytearray(args.reads * READ)
    out_dev = torch.empty(args.reads * READ, dtype=torch.uint8, device="cuda")
    for name, out in (("b: read_ranges_into host", out_host), ("c: read_ranges_into device", out_dev)):
        with opened() as f:
            f.read_ranges_into(ranges(1), [READ] * args.reads, out)     # warm-up: contexts, scratch, staging
            for rep in range(args.repeats):
                offsets = ranges(100 + rep)
                before = f.statistics()
                t = time.perf_counter()
                got = f.read_ranges_into(offsets, [READ] * args.reads, out)
                wall = time.perf_counter() - t
                after = f.statistics()
                assert int(got.sum()) == args.reads * READ
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1),
                     blocks_decoded=after["blocks_decoded"] - before["blocks_decoded"],
                     launches=after["batches"] - before["batches"],
                     d2h_bytes=0 if out is out_dev else args.reads * READ)
    # the bytes of (b) and (c) agree
    with opened() as f:
        f.read_ranges_into(ranges(7), [READ] * args.reads, out_host)
        f.read_ranges_into(ranges(7), [READ] * args.reads, out_dev)
        f.seek(ranges(7)[0])
        first = f.read(READ)
    assert bytes(out_dev[:READ].cpu().numpy()) == bytes(out_host[:READ]) == first
    assert bytes(out_dev.cpu().numpy()) == bytes(out_host)
    emit(step="check", host_equals_device=True)


if __name__ == "__main__":
    main()
