"""Developer probe for quote= of field access on the bench's 2 GiB Silesia-style file (block map and line index imported,
parallelization 0), in one warm process, a fresh reader per figure, every figure repeated to show the spread.  One JSON
line per measurement.

  field_spans_to_tensor(j)              the unquoted path: the decode plus the field passes; 16 bytes per line stay on the GPU
  field_spans_to_tensor(j, quote='"')   the same under a quote: the quoted twins of the passes and k_field_unquote

  --root DIR   import the package from another checkout (one that was built there), to run the unquoted call of the
               parent commit in the same job: a tree without quote= measures the first call only
  --unquoted-only   the unquoted call alone: no quoted warm-up, no quoted call, no difference step.  This is the mode for the
               comparison with the parent commit: the process then does exactly what a process of a tree without quote=
               does, so that the allocator and the runtime are in the same state when the call is timed (the call lands on
               levels about 25 ms apart, and what ran before it in the process can decide which)
  --trace      one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/fields_quoted_probe.py
               --trace`: k_field_chunks, k_field_emit and their quoted twins, k_field_sizes and k_field_unquote then appear
               in one trace

The file is text split at blanks: --delimiter is a blank by default and field 0, the first word, is the short key column.
The file holds quote bytes as any English text does, unbalanced ones too; what is timed is the passes, whatever they find.
Run it under a time limit: `timeout -k 10 600 python tools/fields_quoted_probe.py`."""
import argparse
import inspect
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--field", type=int, default=0)
    ap.add_argument("--delimiter", default=" ")
    ap.add_argument("--quote", default='"')
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--unquoted-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch  # noqa: F401  (first: one HIP runtime in the process, as bench.py does)
    import bench
    import indexed_bzip2_amd as m
    assert os.path.abspath(m.__file__).startswith(os.path.abspath(args.root)), m.__file__

    def emit(**record):
        print(json.dumps(dict(record, label=args.label)), flush=True)

    def timed(call):
        began = time.perf_counter()
        result = call()
        torch.cuda.synchronize()
        return result, time.perf_counter() - began

    dl, q, j = args.delimiter.encode("latin-1"), args.quote.encode("latin-1"), args.field
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

    calls = [("field_spans_to_tensor(%d)" % j, lambda f: int(f.field_spans_to_tensor(j, delimiter=dl)[0].numel()))]
    if not args.unquoted_only and "quote" in inspect.signature(m.reader._IndexedBzip2FileParallel.field_spans_to_tensor).parameters:
        def quoted(f):
            starts, sizes = f.field_spans_to_tensor(j, delimiter=dl, quote=q)
            return int(starts.numel())
        calls.append(("field_spans_to_tensor(%d, quote=%r)" % (j, args.quote), quoted))
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
    emit(step="file", decoded_bytes=total, compressed_bytes=len(enc), lines=max(lines_index.values()), field=j,
         delimiter=args.delimiter, quote=args.quote, results=results)
    assert len(set(results.values())) == 1
    if len(calls) == 2:
        # what the quote changes in this file: the lines whose field differs, counted on the GPU
        with opened() as f:
            plain = f.field_spans_to_tensor(j, delimiter=dl)
            under = f.field_spans_to_tensor(j, delimiter=dl, quote=q)
            emit(step="difference", lines_with_another_start=int((plain[0] != under[0]).sum()),
                 lines_with_another_size=int((plain[1] != under[1]).sum()), lines=int(plain[0].numel()))

    walls = {name: [] for name, _ in calls}
    for rep in range(args.repeats):
        for name, call in calls:
            with opened() as f:
                got, wall = timed(lambda: call(f))
                walls[name].append(wall)
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1), result=got, decoded_gb_per_s=round(total / wall / 1e9, 2))
    for name, values in walls.items():
        emit(step="summary, " + name, min_ms=round(1e3 * min(values), 1), max_ms=round(1e3 * max(values), 1))


if __name__ == "__main__":
    main()
