"""Developer probe for the selection of lines by a regular expression on a field, on the bench's 2 GiB Silesia-style file
(block map and line index imported, parallelization 0), in one warm process, a fresh reader per figure, every figure
repeated to show the spread, the calls alternated within a repeat.  One JSON line per measurement; wall time until the
device is idle.

  field_spans_to_tensor(j)            the baseline a regex predicate is built on: the decode and the field-span passes
  count_where_field(j, values)        the value-set predicate on the same field: field_hashes' passes and k_field_match
  count_where_field(j, regex)         field_spans' passes, k_field_regex per stretch and one rocPRIM select; 8 bytes come
                                      back.  Five cases: an unanchored literal; ^prefix, where the early stop at the dead
                                      state shows; a literal of 62 bytes, 64 states, that never matches (every byte of every
                                      field is walked); ignore_case; and, split at the byte 0x01, which the file rarely
                                      holds, field 0 = the line or nearly all of it, the longest fields the file has, under
                                      the never-matching literal and under ^prefix (the mean and the largest field sizes
                                      are printed: ONE lane walks a field, so the largest decides)
  ... (window)                        the baseline, the value set, the literal and the 64-state pattern over the million lines
                                      whose largest field is the smallest: what the kernel costs on fields of ordinary size
  --trace   one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/fieldregex_probe.py --trace`:
            k_field_regex alone, per call

The file is text split at blanks: --delimiter is a blank by default and field 0, the first word, the column.  Run it under
a time limit: `timeout -k 10 900 python tools/fieldregex_probe.py`."""
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

LITERAL_62 = b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
WINDOW = 1_000_000
WHOLE_LINE = b"\x01"                       # a delimiter the file rarely holds: field 0 is the line, or nearly all of it


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
    ap.add_argument("--literal", default="he")
    ap.add_argument("--prefix", default="^th")
    ap.add_argument("--folded", default="^the$")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    dl, j = args.delimiter.encode("latin-1"), args.field
    literal, prefix, folded = (text.encode("latin-1") for text in (args.literal, args.prefix, args.folded))

    path, enc, meta = bench.build_workload(2 * 1024**3, 214_748_364, bench.default_cache_dir(), 0, 1, lambda: None)
    with m.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
        lines_index = f.line_offsets()
        total = f.size()
        lines = f.count_lines()
        value = f.value_counts(j, limit=1, delimiter=dl)[0][0]      # the most frequent value of the column
        mean_sizes, max_sizes = {}, {}
        for name, k, d in (("field", j, dl), ("whole line", 0, WHOLE_LINE)):
            sizes = f.field_spans_to_tensor(k, delimiter=d)[1]
            mean_sizes[name] = round(float(sizes.clamp(min=0).double().mean()), 1)
            max_sizes[name] = torch.topk(sizes, 3).values.tolist()
        # the window of WINDOW lines of the column whose largest field is the smallest
        sizes = f.field_spans_to_tensor(j, delimiter=dl)[1]
        windows = sizes.numel() // WINDOW
        largest = sizes[:windows * WINDOW].view(windows, WINDOW).max(dim=1).values
        at = int(torch.argmin(largest))
        first = at * WINDOW
        window = {"first": first, "count": WINDOW, "largest_field": int(largest[at]),
                  "field_bytes": int(sizes[first:first + WINDOW].clamp(min=0).sum())}
        del sizes, largest

    def opened():
        f = m.open(path, parallelization=0)
        f.set_block_offsets(blocks)
        f.set_line_offsets(lines_index)
        return f

    regexes = {name: m.compile_regex(pattern, fold) for name, pattern, fold in (
        ("literal", literal, False), ("prefix", prefix, False), ("64 states", LITERAL_62, False), ("ignore_case", folded, True))}
    calls = [("field_spans_to_tensor(%d)" % j, lambda f: int(f.field_spans_to_tensor(j, delimiter=dl)[0].numel())),
             ("count_where_field(%d, 1 value)" % j, lambda f: f.count_where_field(j, values=[value], delimiter=dl))]
    for name, regex in regexes.items():
        calls.append(("count_where_field(%d, regex: %s)" % (j, name), lambda f, regex=regex: f.count_where_field(j, regex=regex, delimiter=dl)))
    calls.append(("field_spans_to_tensor(whole line)", lambda f: int(f.field_spans_to_tensor(0, delimiter=WHOLE_LINE)[0].numel())))
    calls.append(("count_where_field(whole line, 1 value)", lambda f: f.count_where_field(0, values=[value], delimiter=WHOLE_LINE)))
    for name in ("64 states", "prefix"):
        calls.append(("count_where_field(whole line, regex: %s)" % name,
                      lambda f, regex=regexes[name]: f.count_where_field(0, regex=regex, delimiter=WHOLE_LINE)))
    calls.append(("where_field_to_tensor(%d, regex: literal)" % j,
                  lambda f: int(f.where_field_to_tensor(j, regex=regexes["literal"], delimiter=dl).numel())))
    where = dict(first=window["first"], count=WINDOW, delimiter=dl)
    calls.append(("field_spans_to_tensor(%d, window)" % j, lambda f: int(f.field_spans_to_tensor(j, **where)[0].numel())))
    calls.append(("count_where_field(%d, 1 value, window)" % j, lambda f: f.count_where_field(j, values=[value], **where)))
    for name in ("literal", "64 states"):
        calls.append(("count_where_field(%d, regex: %s, window)" % (j, name),
                      lambda f, regex=regexes[name]: f.count_where_field(j, regex=regex, **where)))
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
    emit(step="file", decoded_bytes=total, compressed_bytes=len(enc), lines=lines, field=j, delimiter=args.delimiter,
         value=value.decode("latin-1"), patterns={name: regex.pattern.decode("latin-1") for name, regex in regexes.items()},
         states={name: regex.states for name, regex in regexes.items()}, mean_line_bytes=round(total / lines, 1), mean_field_bytes=mean_sizes,
         largest_fields=max_sizes, window=window, results=results)
    assert results["count_where_field(%d, regex: literal)" % j] == results["where_field_to_tensor(%d, regex: literal)" % j]

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
