"""Developer probe for search on the bench's 2 GiB Silesia-style file (block map imported, parallelization 0), each figure
after a warm-up and repeated to show the spread.  One JSON line per measurement.

  (a) count    count_matches of a rare 8-byte string and of a 1-byte pattern against count_lines() on a fresh line index:
               the same decode with another kernel behind it, so the difference is the search's own cost
  (b) host     the same answers from f.read() of the whole file and a bytes.find loop in the same process: what a user
               does without the feature
  --count-only one count_matches and one count_lines pass, for a run under
               `rocprofv3 --kernel-trace --stats -- python tools/search_probe.py --count-only`: k_count_bytes, k_count_byte
               and k_crc then appear in one trace, over the same decoded bytes (c)
  --ignore-case   (d) count_matches of the rare string exact and with ignore_case=True, alternated on fresh readers in one
               process: the yardstick of the folded call is the exact call of the same run
  --ignore-case --count-only [--frequent]   one exact and one folded pass of count_matches and of count_matches_each with
               k = 200, for a run under rocprofv3 as above: the two instantiations of k_count_bytes and of k_count_set
               then appear side by side in one trace.  --frequent searches for `e` followed by seven bytes that follow
               no `e` of the file's first 64 MiB instead of the rare string: a candidate at every `e` and `E`, and no match

Run it under a time limit: `timeout -k 10 900 python tools/search_probe.py`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: F401  (first: one HIP runtime in the process, as bench.py does)

import bench
import indexed_bzip2_amd as m


def emit(**record):
    print(json.dumps(record), flush=True)


def host_count(raw, pattern):
    count, p = 0, raw.find(pattern)
    while p != -1:
        count += 1
        p = raw.find(pattern, p + 1)
    return count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--count-only", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--ignore-case", action="store_true")
    ap.add_argument("--frequent", action="store_true")
    args = ap.parse_args()

    path, enc, meta = bench.build_workload(2 * 1024**3, 214_748_364, bench.default_cache_dir(), 0, 1, lambda: None)
    with m.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
        total = f.size()
        f.seek(total // 3)
        rare = f.read(8)                     # an 8-byte string the file is known to hold
        if args.ignore_case:
            f.seek(total // 30)
            sample = f.read(64 * 1024 * 1024 if args.frequent else 8 * 1024 * 1024)
    n_blocks = sum(1 for a, b in zip(sorted(blocks.values()), sorted(blocks.values())[1:]) if b > a)
    patterns = {"rare 8 bytes": rare, "1 byte": b"\n"}

    def opened():
        f = m.open(path, parallelization=0)
        f.set_block_offsets(blocks)
        return f

    if args.ignore_case and args.count_only:
        pattern = rare
        if args.frequent:                    # the worst case of the candidate step: a frequent first letter, a tail that never follows it
            tail = b"qZ#7xK@"
            assert sample.lower().find(b"e" + tail.lower()) == -1
            pattern = b"e" + tail
        step = len(sample) // 220
        words = [sample[i * step:i * step + 8] for i in range(200)]
        with opened() as f:
            for fold in (False, True):
                t = time.perf_counter()
                n = f.count_matches(pattern, ignore_case=fold)
                emit(step="count-only, count_matches", ignore_case=fold, pattern=pattern.hex(), matches=n,
                     wall_ms=round(1e3 * (time.perf_counter() - t), 1), blocks=n_blocks, decoded_bytes=total)
            if not args.frequent:
                for fold in (False, True):
                    t = time.perf_counter()
                    each = f.count_matches_each(words, ignore_case=fold)
                    emit(step="count-only, count_matches_each", ignore_case=fold, k=len(words), pairs=int(each.sum()),
                         wall_ms=round(1e3 * (time.perf_counter() - t), 1))
        return

    if args.ignore_case:
        with opened() as f:                   # warm-up: runtime, both instantiations, contexts
            counts = {fold: f.count_matches(rare, ignore_case=fold) for fold in (False, True)}
        emit(step="file", blocks=n_blocks, decoded_bytes=total, compressed_bytes=len(enc), pattern=rare.hex(),
             exact_matches=counts[False], folded_matches=counts[True])
        for rep in range(args.repeats):
            for fold in (False, True):
                with opened() as f:
                    t = time.perf_counter()
                    got = f.count_matches(rare, ignore_case=fold)
                    wall = time.perf_counter() - t
                    assert got == counts[fold]
                    emit(step="count_matches, rare 8 bytes", ignore_case=fold, repeat=rep, wall_ms=round(1e3 * wall, 1),
                         launches=f.statistics()["batches"], decoded_gb_per_s=round(total / wall / 1e9, 2))
        return

    if args.count_only:
        with opened() as f:
            t = time.perf_counter()
            n = f.count_matches(rare)
            emit(step="count-only, count_matches", matches=n, wall_ms=round(1e3 * (time.perf_counter() - t), 1),
                 blocks=n_blocks, decoded_bytes=total)
            t = time.perf_counter()
            n = f.count_lines()
            emit(step="count-only, count_lines", lines=n, wall_ms=round(1e3 * (time.perf_counter() - t), 1))
        return

    with opened() as f:                       # warm-up: runtime, kernels, contexts
        counts = {name: f.count_matches(p) for name, p in patterns.items()}
        lines = f.count_lines()
    assert counts["1 byte"] == lines
    emit(step="file", blocks=n_blocks, decoded_bytes=total, compressed_bytes=len(enc), pattern=rare.hex(), counts=counts)

    for rep in range(args.repeats):
        for name, pattern in patterns.items():
            with opened() as f:
                t = time.perf_counter()
                got = f.count_matches(pattern)
                wall = time.perf_counter() - t
                st = f.statistics()
                assert got == counts[name]
                emit(step="count_matches, " + name, repeat=rep, wall_ms=round(1e3 * wall, 1), launches=st["batches"],
                     blocks_decoded=st["blocks_decoded"], decoded_gb_per_s=round(total / wall / 1e9, 2))
        with opened() as f:
            t = time.perf_counter()
            got = f.count_lines()
            wall = time.perf_counter() - t
            assert got == lines
            emit(step="count_lines, fresh line index", repeat=rep, wall_ms=round(1e3 * wall, 1),
                 decoded_gb_per_s=round(total / wall / 1e9, 2))
        with opened() as f:
            t = time.perf_counter()
            got = f.find_all(rare)
            wall = time.perf_counter() - t
            assert len(got) == counts["rare 8 bytes"]
            emit(step="find_all, rare 8 bytes", repeat=rep, wall_ms=round(1e3 * wall, 1), matches=len(got))

    if args.skip_host:
        return
    for rep in range(args.repeats):
        with opened() as f:
            t = time.perf_counter()
            raw = f.read()
            t_read = time.perf_counter() - t
            for name, pattern in patterns.items():
                t = time.perf_counter()
                got = host_count(raw, pattern)
                t_find = time.perf_counter() - t
                assert got == counts[name]
                emit(step="f.read() + bytes.find loop, " + name, repeat=rep, read_ms=round(1e3 * t_read, 1),
                     find_ms=round(1e3 * t_find, 1), wall_ms=round(1e3 * (t_read + t_find), 1))
            del raw


if __name__ == "__main__":
    main()
