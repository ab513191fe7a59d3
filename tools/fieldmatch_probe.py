"""Developer probe for the selection of lines by a field on the bench's 2 GiB Silesia-style file (block map and line index
imported, parallelization 0), in one warm process, a fresh reader per figure, every figure repeated to show the spread, the
calls alternated within a repeat.  One JSON line per measurement; wall time until the device is idle.

  field_hashes_to_tensor(k)       the baseline a predicate of values is built on: the decode, the field and hash passes
  field_ints_to_tensor(v)         the baseline of a range: the decode, the field passes and k_field_numbers
  count_where_field(k, values)    field_hashes' passes, k_field_match per stretch and one rocPRIM select; 8 bytes come back.
                                  For sets of 1, 64 and 1 024 values taken from the file's own column
  where_field_to_tensor(k, ...)   the same with the selected numbers kept on the GPU
  count_where_field(v, between)   field_ints' passes and the select over the numbers
  select_lines_to_tensor(k, ...)  the selection at a selectivity near 1 %, then the selected lines in a second pass
  --trace   one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/fieldmatch_probe.py --trace`

The file is text split at blanks: --delimiter is a blank by default, field 0, the first word, is the key column and field
1 the number column.  Run it under a time limit: `timeout -k 10 900 python tools/fieldmatch_probe.py`."""
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


def fitting(values, n):
    """The first n of the values that fit a predicate: at most 256 bytes each and 16 384 in total."""
    out, total = [], 0
    for value in values:
        if len(out) == n:
            break
        if len(value) <= 256 and total + len(value) <= 16384:
            out.append(value)
            total += len(value)
    return out


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
        lines = f.count_lines()
        counted = f.value_counts(k, limit=4000, delimiter=dl)       # by descending count

    def opened():
        f = m.open(path, parallelization=0)
        f.set_block_offsets(blocks)
        f.set_line_offsets(lines_index)
        return f

    sets = {n: fitting([value for value, _ in counted], n) for n in (1, 64, 1024)}
    # near 1 % of the lines: the least frequent of the counted values first, until their lines add up
    one_percent, covered = [], 0
    for value, count in reversed(counted):
        if covered >= lines // 100 or len(one_percent) == 1024:
            break
        if len(value) <= 256 and sum(map(len, one_percent)) + len(value) <= 16384:
            one_percent.append(value)
            covered += count
    between = (0, 1000)

    calls = [("field_hashes_to_tensor(%d)" % k, lambda f: int(f.field_hashes_to_tensor(k, delimiter=dl).numel())),
             ("field_ints_to_tensor(%d)" % v, lambda f: int(f.field_ints_to_tensor(v, delimiter=dl).numel()))]
    for n, values in sets.items():
        calls.append(("count_where_field(%d, %d values)" % (k, n), lambda f, values=values: f.count_where_field(k, values=values, delimiter=dl)))
        calls.append(("where_field_to_tensor(%d, %d values)" % (k, n),
                      lambda f, values=values: int(f.where_field_to_tensor(k, values=values, delimiter=dl).numel())))
    calls.append(("count_where_field(%d, between=%r)" % (v, between), lambda f: f.count_where_field(v, between=between, delimiter=dl)))
    calls.append(("select_lines_to_tensor(%d, %d values)" % (k, len(one_percent)),
                  lambda f: [len(f.select_lines_to_tensor(k, values=one_percent, delimiter=dl)[0])]))
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
    emit(step="file", decoded_bytes=total, compressed_bytes=len(enc), lines=lines, key_field=k, value_field=v, delimiter=args.delimiter,
         set_sizes={n: len(values) for n, values in sets.items()}, one_percent_values=len(one_percent), one_percent_lines=covered,
         results=results)
    for n in sets:                                  # a count is the length of the selection
        assert results["count_where_field(%d, %d values)" % (k, n)] == results["where_field_to_tensor(%d, %d values)" % (k, n)]

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
