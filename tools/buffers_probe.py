"""Developer probe: many independent .bz2 buffers, four ways (profiles/buffers_probe.txt).

For each compressed size per buffer (16 KiB, 256 KiB, 900 KiB; Silesia-style data at level 9), `--count` buffers (2 048)
are decoded by
  (a) one warm ibz2.decompress_many call              -- host bytes out
  (b) one warm ibz2.decompress_many_to_tensor call    -- one torch.uint8 tensor on the GPU, nothing back to the host
  (c) ibz2.open(io.BytesIO(b)).read() per buffer      -- timed over the first `--loop` buffers (a reader per buffer)
  (d) CPython bz2.decompress on a pool of 16 threads  -- it releases the GIL; 16 CPUs is what a GPU-box command gets
Reported: buffers per second and decoded GB/s, one JSON line per measurement.  The buffers are `--distinct` different
pieces repeated (the decoder does not care).  Run it under a time limit: `timeout -k 10 900 python tools/buffers_probe.py`.
"""
import argparse
import bz2
import io
import json
import multiprocessing
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: F401  (first: one HIP runtime in the process, as bench.py does)

import indexed_bzip2_amd as m
import silesia_like


def emit(**record):
    print(json.dumps(record), flush=True)


def _compress(args):
    raw, level = args
    return bz2.compress(raw, level)


def make_buffers(target, count, distinct, seed):
    """`count` buffers of about `target` compressed bytes each (level 9)."""
    sample = bytes(silesia_like.generate(4 << 20, seed=seed, threads=1))
    ratio = len(bz2.compress(sample, 9)) / len(sample)
    raw_size = int(target / ratio)
    pool_bytes = bytes(silesia_like.generate(max(raw_size * distinct, raw_size + 1), seed=seed + 1, threads=8))
    pieces = [pool_bytes[i * raw_size:(i + 1) * raw_size] for i in range(distinct)]
    # (all rows are built before the first GPU call, and the workers are spawned, not forked: no child of a process that
    # holds the GPU)
    with ProcessPoolExecutor(16, mp_context=multiprocessing.get_context("spawn")) as pool:
        encs = list(pool.map(_compress, [(p, 9) for p in pieces]))
    return [encs[i % distinct] for i in range(count)], [len(pieces[i % distinct]) for i in range(count)]


def timed(fn, repeats):
    best = None
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--sizes", default="16384,262144,921600")
    ap.add_argument("--loop", type=int, default=128, help="buffers timed for the open().read() loop")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    rows = [(target, *make_buffers(target, args.count, args.distinct, seed=target))
            for target in [int(s) for s in args.sizes.split(",")]]
    for target, encs, raw_sizes in rows:
        decoded = sum(raw_sizes)
        row = dict(target_bytes=target, buffers=len(encs), compressed_bytes=sum(map(len, encs)), decoded_bytes=decoded)

        def rate(method, seconds, n=len(encs), nbytes=decoded):
            emit(**row, method=method, seconds=round(seconds, 4), buffers_per_s=round(n / seconds, 1),
                 decoded_GBps=round(nbytes / seconds / 1e9, 3))

        out = m.decompress_many(encs)                       # warm-up: context, scratch, result buffer
        assert [len(o) for o in out] == raw_sizes
        del out
        rate("decompress_many", timed(lambda: m.decompress_many(encs), args.repeats))
        data, offsets = m.decompress_many_to_tensor(encs)   # warm-up
        assert int(offsets[-1]) == decoded
        del data

        def to_tensor():
            d, _ = m.decompress_many_to_tensor(encs)
            torch.cuda.synchronize()
            return d
        rate("decompress_many_to_tensor", timed(to_tensor, args.repeats))
        k = min(args.loop, len(encs))

        def loop():
            for b in encs[:k]:
                with m.open(io.BytesIO(b)) as f:
                    f.read()
        rate("open_read_per_buffer", timed(loop, 1), n=k, nbytes=sum(raw_sizes[:k]))
        with ThreadPoolExecutor(16) as pool:
            list(pool.map(bz2.decompress, encs[:64]))
            rate("cpython_bz2_16_threads", timed(lambda: list(pool.map(bz2.decompress, encs)), 1))


if __name__ == "__main__":
    main()
