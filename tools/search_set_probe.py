"""Developer probe for the search for a set of patterns on the bench's 2 GiB Silesia-style file (block map imported,
parallelization 0), each figure after a warm-up and repeated to show the spread.  One JSON line per measurement.

  (1) k = 64    count_matches_each of 64 rare 8-byte strings against a loop of 64 count_matches calls in the same process
                (the loop is what a user does without the feature: one decode of the file per string)
  (2) k = 1, k = 1024 (16-byte strings)  the same; of the 1 024 single calls only the first --singles-cap are timed, and
                the figure for all of them is that time scaled, marked as an extrapolation
  (3) dense     a set of 8-byte strings cut from the text where its most frequent bytes stand: long buckets, a candidate
                at most positions
  --count-only K   one count_matches pass and one count_matches_each pass with k = K, for a run under
                `rocprofv3 --kernel-trace --stats -- python tools/search_set_probe.py --count-only K`: k_count_bytes and
                k_count_set then appear in one trace, over the same decoded bytes (4)

Run it under a time limit: `timeout -k 10 900 python tools/search_set_probe.py`."""
import argparse
import collections
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--singles-cap", type=int, default=64)
    ap.add_argument("--count-only", type=int, default=0, metavar="K")
    args = ap.parse_args()

    path, enc, meta = bench.build_workload(2 * 1024**3, 214_748_364, bench.default_cache_dir(), 0, 1, lambda: None)
    with m.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
        total = f.size()
        # strings the file is known to hold, cut at places spread over its first tenth (the file repeats ten times)
        f.seek(total // 30)
        sample = f.read(8 * 1024 * 1024)
    step = len(sample) // 1100
    sets = {
        1: [sample[3 * step:3 * step + 8]],
        64: [sample[i * step * 16:i * step * 16 + 8] for i in range(64)],
        1024: [sample[i * step:i * step + 16] for i in range(1024)],
    }
    common = [byte for byte, _ in collections.Counter(sample).most_common(16)]
    dense = []
    for byte in common:
        at = -1
        for _ in range(16):                          # 16 strings per frequent first byte: buckets of 16
            at = sample.index(bytes([byte]), at + 1 + step)
            dense.append(sample[at:at + 8])
    sets["dense"] = dense

    def opened():
        f = m.open(path, parallelization=0)
        f.set_block_offsets(blocks)
        return f

    if args.count_only:
        patterns = sets[args.count_only]
        with opened() as f:
            t = time.perf_counter()
            n = f.count_matches(patterns[0])
            emit(step="count-only, count_matches", matches=n, wall_ms=round(1e3 * (time.perf_counter() - t), 1),
                 decoded_bytes=total)
            t = time.perf_counter()
            each = f.count_matches_each(patterns)
            emit(step="count-only, count_matches_each", k=len(patterns), pairs=int(each.sum()),
                 wall_ms=round(1e3 * (time.perf_counter() - t), 1))
        return

    with opened() as f:                       # warm-up: runtime, kernels, contexts
        f.count_matches(sets[1][0])
        counts = {name: f.count_matches_each(patterns) for name, patterns in sets.items()}
    emit(step="file", decoded_bytes=total, compressed_bytes=len(enc),
         sets={str(name): {"k": len(p), "bytes": sum(map(len, p)), "pairs": int(counts[name].sum())} for name, p in sets.items()})

    for name, patterns in sets.items():
        k = len(patterns)
        timed = min(k, args.singles_cap)
        for rep in range(args.repeats):
            with opened() as f:
                t = time.perf_counter()
                each = f.count_matches_each(patterns)
                wall_set = time.perf_counter() - t
                st = f.statistics()
                assert each.tolist() == counts[name].tolist()
            with opened() as f:
                t = time.perf_counter()
                singles = [f.count_matches(p) for p in patterns[:timed]]
                wall_singles = time.perf_counter() - t
                assert singles == counts[name][:timed].tolist()
            scaled = wall_singles * k / timed
            emit(step=f"set {name}", k=k, repeat=rep, set_wall_ms=round(1e3 * wall_set, 1), launches=st["batches"],
                 blocks_decoded=st["blocks_decoded"], singles_timed=timed, singles_wall_ms=round(1e3 * wall_singles, 1),
                 singles_wall_ms_for_k=round(1e3 * scaled, 1), extrapolated=timed < k, ratio=round(scaled / wall_set, 1))


if __name__ == "__main__":
    main()
