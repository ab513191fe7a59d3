"""Developer probe for field columns on the bench's 2 GiB Silesia-style file (block map and line index imported,
parallelization 0), in one warm process, a fresh reader per figure, one warm-up and then --repeats rounds with the calls
alternated, wall time until the device is idle.  One JSON line per measurement.

  field_spans_to_tensor(0)               the floor: the decode plus the field passes; 16 bytes per line stay on the GPU
  read_fields_to_tensor(0)               the path there was: field_spans, the ranges planned on the host, a second decode
  read_columns_to_tensor([0])            one column from one decode: the field passes, the gather, the fix-ups
  read_columns_to_tensor([0, 1])         each further field: one more set of field passes and one more gather
  read_columns_to_tensor([0, 1, 2, 3])
  --trace   one call of read_columns_to_tensor([0]) and one plain device-to-device copy of the column's size, for a run
            under `rocprofv3 --kernel-trace --stats -- python tools/fieldcols_probe.py --trace`: k_field_gather,
            k_fieldcol_sums / _top / _offsets and the field kernels then appear per launch in one trace

The file is text split at blanks: --delimiter is a blank by default and field 0, the first word, is the short key column.
Run it under a time limit: `timeout -k 10 900 python tools/fieldcols_probe.py`."""
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
    torch.cuda.synchronize()
    began = time.perf_counter()
    result = call()
    torch.cuda.synchronize()
    return result, time.perf_counter() - began


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--delimiter", default=" ")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    dl = args.delimiter.encode("latin-1")

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

    def columns(fields):
        def call(f):
            before = f.statistics()
            got = f.read_columns_to_tensor(fields, delimiter=dl)
            after = f.statistics()
            return {"lines": int(got[0][2].numel()), "bytes": [int(data.numel()) for data, _, _ in got],
                    "blocks_decoded": after["blocks_decoded"] - before["blocks_decoded"], "launches": after["batches"] - before["batches"]}
        return call

    def spans(f):
        return {"lines": int(f.field_spans_to_tensor(0, delimiter=dl)[0].numel())}

    def fields(f):
        before = f.statistics()
        data, offsets = f.read_fields_to_tensor(0, delimiter=dl)
        after = f.statistics()
        return {"lines": len(offsets) - 1, "bytes": [int(data.numel())], "blocks_decoded": after["blocks_decoded"] - before["blocks_decoded"]}

    calls = (("field_spans_to_tensor(0)", spans), ("read_fields_to_tensor(0)", fields), ("read_columns_to_tensor([0])", columns([0])),
             ("read_columns_to_tensor([0, 1])", columns([0, 1])), ("read_columns_to_tensor([0, 1, 2, 3])", columns([0, 1, 2, 3])))
    if args.trace:
        with opened() as f:
            got, wall = timed(lambda: columns([0])(f))
            emit(step="trace, read_columns_to_tensor([0])", result=got, wall_ms=round(1e3 * wall, 1), decoded_bytes=total)
        source = torch.empty(got["bytes"][0], dtype=torch.uint8, device="cuda")
        for _ in range(3):
            _, wall = timed(lambda: source.clone())
            emit(step="trace, device-to-device copy", bytes=got["bytes"][0], wall_ms=round(1e3 * wall, 3))
        return

    results = {}
    for name, call in calls:                        # warm-up: runtime, kernels, contexts
        with opened() as f:
            results[name] = call(f)
    emit(step="file", decoded_bytes=total, compressed_bytes=len(enc), delimiters=max(lines_index.values()),
         tile_bytes=m._native.gather_fields_tile_bytes(), delimiter=args.delimiter, results=results)
    assert len({result["lines"] for result in results.values()}) == 1
    assert results["read_fields_to_tensor(0)"]["bytes"] == results["read_columns_to_tensor([0])"]["bytes"]

    walls = {name: [] for name, _ in calls}
    for rep in range(args.repeats):
        for name, call in calls:
            with opened() as f:
                got, wall = timed(lambda: call(f))
                walls[name].append(wall)
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1), decoded_gb_per_s=round(total / wall / 1e9, 2))
    for name, values in walls.items():
        emit(step="summary, " + name, min_ms=round(1e3 * min(values), 1), median_ms=round(1e3 * sorted(values)[len(values) // 2], 1),
             max_ms=round(1e3 * max(values), 1))
    column_bytes = results["read_columns_to_tensor([0])"]["bytes"][0]
    source = torch.empty(column_bytes, dtype=torch.uint8, device="cuda")
    copies = [timed(lambda: source.clone())[1] for _ in range(args.repeats + 1)][1:]
    emit(step="summary, device-to-device copy of one column", bytes=column_bytes, min_ms=round(1e3 * min(copies), 3),
         max_ms=round(1e3 * max(copies), 3))


if __name__ == "__main__":
    main()
