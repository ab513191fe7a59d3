"""Developer probe for field numbers and sums on the bench's 2 GiB Silesia-style file (block map and line index imported,
parallelization 0), in one warm process, a fresh reader per figure, every figure repeated to show the spread, the calls
alternated within a repeat.  One JSON line per measurement.

  field_spans_to_tensor(k)    the decode plus the field passes; 16 bytes per line stay on the GPU
  field_hashes_to_tensor(k)   the decode plus the field and hash passes; 24 bytes per line stay on the GPU
  count_by_field(k)           field_hashes, the sort and the run kernels; 32 bytes per distinct value come back
  field_ints_to_tensor(v)     the decode plus the field passes, k_field_numbers and k_field_texts; 24 bytes per line stay
                              on the GPU.  The yardsticks are field_spans (the same passes without the parse) and
                              field_hashes (one pass more over the bytes)
  sum_by_field(k, v)          one decode, the passes of field_hashes for k and of field_ints for v, the sort and one
                              reduce-by-key; 72 bytes per distinct key come back.  The yardstick is count_by_field plus
                              what field_ints adds to the decode
  --trace   one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/fieldnum_probe.py --trace`

The file is text split at blanks: --delimiter is a blank by default, field 0, the first word, is the key column and field
1 the value column: few of its words are numbers, which costs k_field_numbers no less, since every present field of 1
to 19 bytes is read.  Run it under a time limit: `timeout -k 10 900 python tools/fieldnum_probe.py`."""
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
    ap.add_argument("--key-field", type=int, default=0)
    ap.add_argument("--value-field", type=int, default=1)
    ap.add_argument("--delimiter", default=" ")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    dl, k, v = args.delimiter.encode("latin-1"), args.key_field, args.value_field

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
        lines, counts, missing = f.count_by_field(k, delimiter=dl)
        return [len(lines), int(counts.sum()) + missing]

    def numbers(f):
        column = f.field_ints_to_tensor(v, delimiter=dl)
        return [int(column.numel()), int((column > m.FIELD_NUMBER_MISSING).sum())]

    def summed(f):
        lines, counts, numbers_, sums, _, _, missing = f.sum_by_field(k, v, delimiter=dl)
        return [len(lines), int(counts.sum()) + missing, int(numbers_.sum()), sum(sums)]

    calls = (("field_spans_to_tensor(%d)" % k, lambda f: int(f.field_spans_to_tensor(k, delimiter=dl)[0].numel())),
             ("field_hashes_to_tensor(%d)" % k, lambda f: int(f.field_hashes_to_tensor(k, delimiter=dl).numel())),
             ("count_by_field(%d)" % k, grouped),
             ("field_ints_to_tensor(%d)" % v, numbers),
             ("sum_by_field(%d, %d)" % (k, v), summed))
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
         chunk_bytes=m._native.field_chunk_bytes(), key_field=k, value_field=v, delimiter=args.delimiter, results=results)
    lines = results[calls[0][0]]
    assert results[calls[1][0]] == results[calls[2][0]][1] == results[calls[3][0]][0] == results[calls[4][0]][1] == lines
    assert results[calls[2][0]][0] == results[calls[4][0]][0]                    # the same groups

    walls = {name: [] for name, _ in calls}
    for rep in range(args.repeats):
        for name, call in calls:
            with opened() as f:
                got, wall = timed(lambda: call(f))
                walls[name].append(wall)
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1), result=got, decoded_gb_per_s=round(total / wall / 1e9, 2))
    for name, values in walls.items():
        emit(step="summary, " + name, min_ms=round(1e3 * min(values), 1), median_ms=round(1e3 * sorted(values)[len(values) // 2], 1),
             max_ms=round(1e3 * max(values), 1))


if __name__ == "__main__":
    main()
