"""Developer probe for grep and line numbers on the bench's 2 GiB Silesia-style file (block map and line index imported,
parallelization 0), each figure after a warm-up and repeated to show the spread.  One JSON line per measurement.

  (a) grep     grep and count_matching_lines of a rare 8-byte string and of one frequent byte pair (the pair's lines are
               limited to --pair-lines: all of them are most of the file), beside count_matches of the same patterns:
               grep = the search pass + the rank pass over the blocks with matches + the line ranges, so the difference to
               count_matches is what the feature adds
      halves   find_all of the same pattern and line_numbers of its positions, timed one after the other: what the search
               with all positions emitted costs, and what planning and the rank pass cost
  (b) host     the same answers from f.read() of the whole file, a bytes.find loop and a split into lines in the same
               process: what a user does without the feature
  --trace      one count_matching_lines of the pair, for a run under
               `rocprofv3 --kernel-trace --stats -- python tools/grep_probe.py --trace`: k_rank_byte, k_count_byte and
               k_count_bytes then appear in one trace

Run it under a time limit: `timeout -k 10 900 python tools/grep_probe.py`."""
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


def host_grep(raw, newlines, pattern, limit):
    """Distinct lines with a match's first byte, by bytes.find and a binary search over the newline positions."""
    numbers, p = [], raw.find(pattern)
    while p != -1:
        numbers.append(p)
        p = raw.find(pattern, p + 1)
    numbers = np.unique(np.searchsorted(newlines, np.array(numbers, dtype=np.int64), "left"))
    count = len(numbers)
    starts = np.concatenate([[0], newlines + 1, [len(raw)]])
    lines = [raw[starts[k]:starts[k + 1]] for k in numbers[:limit]]
    return count, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pair", default="e ")
    ap.add_argument("--pair-lines", type=int, default=100_000)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()

    path, enc, meta = bench.build_workload(2 * 1024**3, 214_748_364, bench.default_cache_dir(), 0, 1, lambda: None)
    with m.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
        lines_index = f.line_offsets()
        total = f.size()
        f.seek(total // 3)
        rare = f.read(8)                     # an 8-byte string the file is known to hold
    n_blocks = sum(1 for a, b in zip(sorted(blocks.values()), sorted(blocks.values())[1:]) if b > a)
    pair = args.pair.encode()
    patterns = {"rare 8 bytes": (rare, None), "byte pair": (pair, args.pair_lines)}

    def opened():
        f = m.open(path, parallelization=0)
        f.set_block_offsets(blocks)
        f.set_line_offsets(lines_index)
        return f

    if args.trace:
        with opened() as f:
            t = time.perf_counter()
            n = f.count_matching_lines(pair)
            emit(step="trace, count_matching_lines, byte pair", lines=n, wall_ms=round(1e3 * (time.perf_counter() - t), 1),
                 blocks=n_blocks, decoded_bytes=total)
        return

    with opened() as f:                       # warm-up: runtime, kernels, contexts
        matches = {name: f.count_matches(p) for name, (p, _) in patterns.items()}
        matching = {name: f.count_matching_lines(p) for name, (p, _) in patterns.items()}
    emit(step="file", blocks=n_blocks, decoded_bytes=total, compressed_bytes=len(enc), lines=max(lines_index.values()),
         rare=rare.hex(), pair=args.pair, matches=matches, matching_lines=matching)

    for rep in range(args.repeats):
        for name, (pattern, limit) in patterns.items():
            with opened() as f:
                t = time.perf_counter()
                got = f.count_matches(pattern)
                wall = time.perf_counter() - t
                assert got == matches[name]
                emit(step="count_matches, " + name, repeat=rep, wall_ms=round(1e3 * wall, 1),
                     decoded_gb_per_s=round(total / wall / 1e9, 2))
            with opened() as f:
                t = time.perf_counter()
                got = f.count_matching_lines(pattern)
                wall = time.perf_counter() - t
                st = f.statistics()
                assert got == matching[name]
                emit(step="count_matching_lines, " + name, repeat=rep, wall_ms=round(1e3 * wall, 1), lines=got,
                     launches=st["batches"], blocks_decoded=st["blocks_decoded"])
            with opened() as f:                # the two halves of count_matching_lines, each through its public call
                t = time.perf_counter()
                positions = f.find_all(pattern)
                t_find = time.perf_counter() - t
                t = time.perf_counter()
                numbers = f.line_numbers(positions)
                t_rank = time.perf_counter() - t
                assert len(positions) == matches[name] and len(np.unique(numbers)) == matching[name]
                emit(step="find_all, then line_numbers of the positions, " + name, repeat=rep,
                     find_all_ms=round(1e3 * t_find, 1), line_numbers_ms=round(1e3 * t_rank, 1), positions=len(positions))
            with opened() as f:
                t = time.perf_counter()
                numbers, lines = f.grep(pattern, limit=limit)
                wall = time.perf_counter() - t
                st = f.statistics()
                assert len(numbers) == min(matching[name], limit or matching[name])
                emit(step="grep, " + name, repeat=rep, wall_ms=round(1e3 * wall, 1), lines=len(lines),
                     line_bytes=sum(map(len, lines)), launches=st["batches"], blocks_decoded=st["blocks_decoded"])

    if args.skip_host:
        return
    for rep in range(args.repeats):
        with opened() as f:
            t = time.perf_counter()
            raw = f.read()
            t_read = time.perf_counter() - t
            t = time.perf_counter()
            newlines = np.flatnonzero(np.frombuffer(raw, dtype=np.uint8) == 10).astype(np.int64)
            t_index = time.perf_counter() - t
            for name, (pattern, limit) in patterns.items():
                t = time.perf_counter()
                count, lines = host_grep(raw, newlines, pattern, limit)
                t_grep = time.perf_counter() - t
                assert count == matching[name]
                emit(step="f.read() + bytes.find loop + line split, " + name, repeat=rep, read_ms=round(1e3 * t_read, 1),
                     newline_ms=round(1e3 * t_index, 1), grep_ms=round(1e3 * t_grep, 1),
                     wall_ms=round(1e3 * (t_read + t_index + t_grep), 1))
            del raw


if __name__ == "__main__":
    main()
