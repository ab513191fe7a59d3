"""Developer probe for line_hashes on the bench's 2 GiB Silesia-style file (block map and line index imported,
parallelization 0), in one warm process, a fresh reader per figure, every figure repeated to show the spread.  One JSON
line per measurement.

  count_lines()            the yardstick: the decode plus a counting pass.  The one figure whose reader gets the block map
                           only -- with the line index imported the call would return what it was given
  line_hashes_to_tensor()  the decode plus the hashing passes; 8 bytes per line stay on the GPU
  line_hashes()            the same plus the copy of the hashes to the host
  count_distinct_lines()   the same plus the sort of (hash, line number), the flags and their count
  first_occurrences()      the same plus the selection and the second sort
  --trace   one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/linehash_probe.py --trace`:
            k_linehash_chunks, k_linehash_link, k_linehash_emit and rocPRIM's kernels then appear in one trace

Run it under a time limit: `timeout -k 10 900 python tools/linehash_probe.py`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (first: one HIP runtime in the process, as bench.py does)

import bench
import indexed_bzip2_amd as m


def emit(**record):
    print(json.dumps(record), flush=True)


def timed(call):
    began = time.perf_counter()
    result = call()
    torch.cuda.synchronize()
    return result, time.perf_counter() - began


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()

    path, enc, meta = bench.build_workload(2 * 1024**3, 214_748_364, bench.default_cache_dir(), 0, 1, lambda: None)
    with m.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
        lines_index = f.line_offsets()
        total = f.size()

    def opened(with_lines=True):
        f = m.open(path, parallelization=0)
        f.set_block_offsets(blocks)
        if with_lines:
            f.set_line_offsets(lines_index)
        return f

    calls = (("count_lines()", False, lambda f: f.count_lines()),
             ("line_hashes_to_tensor()", True, lambda f: int(f.line_hashes_to_tensor().numel())),
             ("line_hashes()", True, lambda f: len(f.line_hashes())),
             ("count_distinct_lines()", True, lambda f: f.count_distinct_lines()),
             ("first_occurrences()", True, lambda f: len(f.first_occurrences())))
    if args.trace:
        for name, with_lines, call in calls:
            with opened(with_lines) as f:
                got, wall = timed(lambda: call(f))
                emit(step="trace, " + name, result=got, wall_ms=round(1e3 * wall, 1), decoded_bytes=total)
        return

    results = {}
    for name, with_lines, call in calls:            # warm-up: runtime, kernels, contexts, rocPRIM
        with opened(with_lines) as f:
            results[name] = call(f)
    emit(step="file", decoded_bytes=total, compressed_bytes=len(enc), delimiters=max(lines_index.values()),
         chunk_bytes=m._native.line_hash_chunk_bytes(), results=results)
    assert results["line_hashes()"] == results["line_hashes_to_tensor()"] >= results["count_lines()"]
    assert results["count_distinct_lines()"] == results["first_occurrences()"] <= results["line_hashes()"]

    walls = {name: [] for name, _, _ in calls}
    for rep in range(args.repeats):
        for name, with_lines, call in calls:
            with opened(with_lines) as f:
                got, wall = timed(lambda: call(f))
                walls[name].append(wall)
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1), result=got, decoded_gb_per_s=round(total / wall / 1e9, 2))
    for name, values in walls.items():
        emit(step="summary, " + name, min_ms=round(1e3 * min(values), 1), max_ms=round(1e3 * max(values), 1))


if __name__ == "__main__":
    main()
