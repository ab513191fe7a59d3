"""Developer probe for field access on the bench's 2 GiB Silesia-style file (block map and line index imported,
parallelization 0), in one warm process, a fresh reader per figure, every figure repeated to show the spread.  One JSON
line per measurement.

  line_hashes_to_tensor()    the yardstick: the decode plus the hashing passes; 8 bytes per line stay on the GPU
  line_hashes()              the same plus the copy of the hashes to the host
  field_spans_to_tensor(j)   the decode plus the field passes; 16 bytes per line stay on the GPU
  field_spans(j)             the same plus the copy of starts and sizes to the host
  read_fields_to_tensor(j)   for --key-lines lines, split into its three parts: field_spans, the arrays prepared in numpy,
                             and the one read_ranges call that decodes the blocks a second time and gathers the fields.
                             Beside it the same read_ranges call over one byte per --coarse-bytes of the same stretch of
                             the file: the same blocks decoded, a few thousand ranges instead of millions.  The
                             difference is what the ranges cost: planning them on the host, their piece lists, the gather
  --trace   one call of each, for a run under `rocprofv3 --kernel-trace --stats -- python tools/fields_probe.py --trace`:
            k_field_chunks, k_field_link, k_field_emit, k_field_sizes and the line-hash kernels then appear in one trace

The file is text split at blanks: --delimiter is a blank by default and field 0, the first word, is the short key column.
Run it under a time limit: `timeout -k 10 900 python tools/fields_probe.py`."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (first: one HIP runtime in the process, as bench.py does)

import numpy as np

import bench
import indexed_bzip2_amd as m


def emit(**record):
    print(json.dumps(record), flush=True)


def timed(call):
    began = time.perf_counter()
    result = call()
    torch.cuda.synchronize()
    return result, time.perf_counter() - began


def read_ranges_to_tensor(f, starts, lengths):
    """The read_ranges call of read_fields_to_tensor, alone: the bytes gathered on the device."""
    reader = f._open_reader()
    data = torch.empty(int(lengths.sum()), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = np.empty(len(starts), dtype=np.uint64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    began = time.perf_counter()
    reader._check(m.lib().mi355x_bz2_reader_read_ranges(reader._h, starts.ctypes.data_as(u64p), lengths.ctypes.data_as(u64p),
                                                        len(starts), ctypes.c_void_p(data.data_ptr()), 1, got.ctypes.data_as(u64p)))
    torch.cuda.synchronize()
    return time.perf_counter() - began, int(got.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--field", type=int, default=0)
    ap.add_argument("--delimiter", default=" ")
    ap.add_argument("--key-lines", type=int, nargs="*", default=[1_000_000, 8_000_000, 0], help="0: all lines")
    ap.add_argument("--coarse-bytes", type=int, default=65_536)
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

    calls = (("line_hashes_to_tensor()", lambda f: int(f.line_hashes_to_tensor().numel())),
             ("line_hashes()", lambda f: len(f.line_hashes())),
             ("field_spans_to_tensor(%d)" % j, lambda f: int(f.field_spans_to_tensor(j, delimiter=dl)[0].numel())),
             ("field_spans(%d)" % j, lambda f: len(f.field_spans(j, delimiter=dl)[0])))
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
    with opened() as f:
        starts, sizes = f.field_spans(j, delimiter=dl)
    present = sizes >= 0
    emit(step="file", decoded_bytes=total, compressed_bytes=len(enc), delimiters=max(lines_index.values()),
         chunk_bytes=m._native.field_chunk_bytes(), field=j, delimiter=args.delimiter, results=results,
         lines_with_the_field=int(present.sum()), field_bytes=int(sizes[present].sum()))
    assert len(set(results.values())) == 1

    walls = {name: [] for name, _ in calls}
    for rep in range(args.repeats):
        for name, call in calls:
            with opened() as f:
                got, wall = timed(lambda: call(f))
                walls[name].append(wall)
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1), result=got, decoded_gb_per_s=round(total / wall / 1e9, 2))
    for name, values in walls.items():
        emit(step="summary, " + name, min_ms=round(1e3 * min(values), 1), max_ms=round(1e3 * max(values), 1))

    # the key column: field_spans, numpy, read_ranges -- and read_ranges over few ranges of the same blocks
    for wanted in args.key_lines:
        n = len(starts) if wanted == 0 else min(wanted, len(starts))
        for rep in range(2):
            with opened() as f:
                (s, z), spans_wall = timed(lambda: f.field_spans(j, 0, n, delimiter=dl))
                began = time.perf_counter()
                lengths = np.maximum(z, 0).astype(np.uint64)
                bounds = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(lengths, out=bounds[1:])
                numpy_wall = time.perf_counter() - began
                ranges_wall, got = read_ranges_to_tensor(f, s, lengths)
                assert got == int(bounds[-1])
            end = int(s[-1]) + 1
            coarse = np.arange(0, end, args.coarse_bytes, dtype=np.uint64)
            with opened() as f:
                coarse_wall, _ = read_ranges_to_tensor(f, coarse, np.ones(len(coarse), dtype=np.uint64))
            with opened() as f:
                _, whole_wall = timed(lambda: f.read_fields_to_tensor(j, 0, n, delimiter=dl))
            emit(step="read_fields_to_tensor(%d), %d lines" % (j, n), repeat=rep, field_bytes=got, stretch_bytes=end,
                 field_spans_ms=round(1e3 * spans_wall, 1), numpy_ms=round(1e3 * numpy_wall, 1),
                 read_ranges_ms=round(1e3 * ranges_wall, 1), coarse_ranges=len(coarse),
                 read_ranges_coarse_ms=round(1e3 * coarse_wall, 1), per_range_ns=round(1e9 * (ranges_wall - coarse_wall) / n, 1),
                 ranges_share=round((ranges_wall - coarse_wall) / (spans_wall + numpy_wall + ranges_wall), 3),
                 whole_call_ms=round(1e3 * whole_wall, 1))


if __name__ == "__main__":
    main()
