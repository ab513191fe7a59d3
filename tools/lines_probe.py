"""Developer probe for line access on the bench's 2 GiB Silesia-style file (parallelization 0), each figure after a
warm-up and repeated to show the spread.  One JSON line per measurement.

  index    line_offsets() on a fresh reader (block map built on the way: two passes over the file) against
           block_offsets() on a fresh reader, alternated; and line_offsets() with the block map imported (the counting
           pass alone: every block decoded once, k_count_byte over it, nothing copied out)
  ranges   1 000 random 10-line ranges with both indexes imported, into host memory (read_line_ranges) and into a
           torch.uint8 tensor (read_line_ranges_to_tensor): wall, blocks decoded, launches, bytes D2H
  --count-only   just one counting pass with the block map imported, for a run under
           `rocprofv3 --kernel-trace --stats -- python tools/lines_probe.py --count-only`: k_count_byte and k_crc then
           appear in one trace, over the same decoded bytes

Run it under a time limit: `timeout -k 10 900 python tools/lines_probe.py`."""
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


def emit(**record):
    print(json.dumps(record), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranges", type=int, default=1000)
    ap.add_argument("--lines", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--count-only", action="store_true")
    args = ap.parse_args()

    path, enc, meta = bench.build_workload(2 * 1024**3, 214_748_364, bench.default_cache_dir(), 0, 1, lambda: None)
    with m.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
        total = f.size()
    n_blocks = sum(1 for a, b in zip(sorted(blocks.values()), sorted(blocks.values())[1:]) if b > a)

    def opened(block_index=True, line_index=None):
        f = m.open(path, parallelization=0)
        if block_index:
            f.set_block_offsets(blocks)
        if line_index is not None:
            f.set_line_offsets(line_index)
        return f

    if args.count_only:
        with opened() as f:
            t = time.perf_counter()
            n = f.count_lines()
            emit(step="count-only", lines=n, wall_ms=round(1e3 * (time.perf_counter() - t), 1), blocks=n_blocks,
                 decoded_bytes=total)
        return

    with opened() as f:                       # warm-up: runtime, kernels
        lines = f.line_offsets()
    n = max(lines.values())
    emit(step="file", blocks=n_blocks, decoded_bytes=total, compressed_bytes=len(enc), lines=n)

    for rep in range(args.repeats):
        for name in ("block_offsets, fresh reader", "line_offsets, fresh reader"):
            with opened(block_index=False) as f:
                t = time.perf_counter()
                got = f.block_offsets() if name.startswith("block") else f.line_offsets()
                wall = time.perf_counter() - t
                st = f.statistics()
                assert got == (blocks if name.startswith("block") else lines)
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1), blocks_decoded=st["blocks_decoded"],
                     launches=st["batches"])
        with opened() as f:
            t = time.perf_counter()
            got = f.line_offsets()
            wall = time.perf_counter() - t
            st = f.statistics()
            assert got == lines
            emit(step="line_offsets, block map imported", repeat=rep, wall_ms=round(1e3 * wall, 1),
                 blocks_decoded=st["blocks_decoded"], launches=st["batches"],
                 decoded_gb_per_s=round(total / wall / 1e9, 2))

    def ranges(seed):
        return [(int(x), args.lines) for x in np.random.default_rng(seed).integers(0, n, args.ranges)]

    for name in ("read_line_ranges, host", "read_line_ranges_to_tensor, device"):
        with opened(line_index=lines) as f:
            host = name.endswith("host")
            call = f.read_line_ranges if host else f.read_line_ranges_to_tensor
            call(ranges(1))                   # warm-up: contexts, scratch, staging
            for rep in range(args.repeats):
                wanted = ranges(100 + rep)
                before = f.statistics()
                t = time.perf_counter()
                got = call(wanted)
                wall = time.perf_counter() - t
                after = f.statistics()
                size = sum(len(g) for g in got) if host else int(got[0].numel())
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1), bytes=size,
                     blocks_decoded=after["blocks_decoded"] - before["blocks_decoded"],
                     launches=after["batches"] - before["batches"], d2h_bytes=size if host else 0)
    with opened(line_index=lines) as f:
        wanted = ranges(7)
        host = f.read_line_ranges(wanted)
        data, offsets = f.read_line_ranges_to_tensor(wanted)
        assert bytes(data.cpu().numpy()) == b"".join(host) and offsets.tolist()[-1] == sum(len(h) for h in host)
        starts = f.line_starts([k for k, _ in wanted[:50]])
        f.seek(int(starts[0]))
        assert f.read(len(host[0])) == host[0]
    emit(step="check", host_equals_device=True)


if __name__ == "__main__":
    main()
