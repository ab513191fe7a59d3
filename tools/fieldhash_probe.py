"""Developer probe for field hashes on the bench's 2 GiB Silesia-style file (block map and line index imported,
parallelization 0), in one warm process, a fresh reader per figure, every figure repeated to show the spread, the calls
alternated within a repeat.  One JSON line per measurement.

  line_hashes_to_tensor()     the decode plus the hashing passes; 8 bytes per line stay on the GPU
  field_spans_to_tensor(j)    the decode plus the field passes; 16 bytes per line stay on the GPU
  field_hashes_to_tensor(j)   the decode plus both first passes, one emitting pass and the finish; 24 bytes per line stay on
                              the GPU.  The yardstick is the SUM of the two figures above: the call does both jobs
  count_by_field(j)           field_hashes, the sort and the run kernels; 32 bytes per distinct value come back
  value_counts(j, limit=20)   end to end: count_by_field and one read_ranges over twenty spans
  --trace   one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/fieldhash_probe.py --trace`

The file is text split at blanks: --delimiter is a blank by default and field 0, the first word, is the short key column.
Run it under a time limit: `timeout -k 10 900 python tools/fieldhash_probe.py`."""
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
    ap.add_argument("--field", type=int, default=0)
    ap.add_argument("--delimiter", default=" ")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    dl, j = args.delimiter.encode("latin-1"), args.field

    path, enc, meta = bench.build_workload(2 * 1024**3, 214_748_364, bench.default_cache_dir(), 0, 1, lambda: None)
    with m.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
        lines_index = f.line_offsets()
        total = f.size()

    def opened():
        f = m.open(path, parallelization=0)
        f.set_block_offsets(blocks)
        f.set_line_offsets(lines_index)
        return f

    def grouped(f):
        lines, counts, missing = f.count_by_field(j, delimiter=dl)
        return [len(lines), int(counts.sum()) + missing]

    calls = (("line_hashes_to_tensor()", lambda f: int(f.line_hashes_to_tensor().numel())),
             ("field_spans_to_tensor(%d)" % j, lambda f: int(f.field_spans_to_tensor(j, delimiter=dl)[0].numel())),
             ("field_hashes_to_tensor(%d)" % j, lambda f: int(f.field_hashes_to_tensor(j, delimiter=dl).numel())),
             ("count_by_field(%d)" % j, grouped),
             ("value_counts(%d, limit=20)" % j, lambda f: [[v.decode("latin-1"), c] for v, c in f.value_counts(j, 20, delimiter=dl)][:3]))
    if args.trace:
        for name, call in calls:
            with opened() as f:
                got, wall = timed(lambda: call(f))
                emit(step="trace, " + name, result=got, wall_ms=round(1e3 * wall, 1), decoded_bytes=total)
        return

    results = {}
    for name, call in calls:                        # warm-up: runtime, kernels, contexts
        with opened() as f:
            results[name] = call(f)
    emit(step="file", decoded_bytes=total, compressed_bytes=len(enc), delimiters=max(lines_index.values()),
         chunk_bytes=m._native.field_chunk_bytes(), field=j, delimiter=args.delimiter, results=results)
    lines = results[calls[0][0]]
    assert results[calls[1][0]] == results[calls[2][0]] == results[calls[3][0]][1] == lines

    walls = {name: [] for name, _ in calls}
    for rep in range(args.repeats):
        for name, call in calls:
            with opened() as f:
                got, wall = timed(lambda: call(f))
                walls[name].append(wall)
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1), result=got, decoded_gb_per_s=round(total / wall / 1e9, 2))
    for name, values in walls.items():
        emit(step="summary, " + name, min_ms=round(1e3 * min(values), 1), max_ms=round(1e3 * max(values), 1))
    yardstick = [a + b for a, b in zip(walls[calls[0][0]], walls[calls[1][0]])]
    emit(step="summary, line_hashes_to_tensor + field_spans_to_tensor", min_ms=round(1e3 * min(yardstick), 1),
         max_ms=round(1e3 * max(yardstick), 1))


if __name__ == "__main__":
    main()
