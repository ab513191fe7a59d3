"""Developer probe for grep_regex on the bench's 2 GiB Silesia-style file (block map and line index imported,
parallelization 0), in one warm process, every figure repeated to show the spread.  One JSON line per measurement.

  (a) count_matching_lines_regex(b"error") beside count_matching_lines(b"error"): the same lines, the second through the
      fixed-string search, which is the path the regex pass stands next to.  Both decode the file once; the difference is
      the pass over the decoded bytes (and, for the fixed string, the rank pass over the blocks with matches).
  (b) the same for a 19-state pattern, ^(GET|POST) /[a-z/]* HTTP/1\\.[01]$, and for b"the", which many lines hold:
      count_matching_lines then pays for its positions and its rank pass, the regex count for neither
  (c) 256 MiB without a single delimiter (16 MiB of seeded bytes, none of them "\\n", as 16 streams): every chunk is all
      head, the pass pays up to n table steps per byte
  --trace   one count_matching_lines_regex of b"error", and of b"the" one count and one grep_regex with a limit, for a run under
            `rocprofv3 --kernel-trace --stats -- python tools/regex_probe.py --trace`: k_regex_chunks, k_regex_link and
            k_regex_emit then appear in one trace

Run it under a time limit: `timeout -k 10 900 python tools/regex_probe.py`."""
import argparse
import bz2
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (first: one HIP runtime in the process, as bench.py does)

import numpy as np

import bench
import indexed_bzip2_amd as m

WIDE = rb"^(GET|POST) /[a-z/]* HTTP/1\.[01]$"


def emit(**record):
    print(json.dumps(record), flush=True)


def timed(call):
    began = time.perf_counter()
    result = call()
    return result, time.perf_counter() - began


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--skip-headless", action="store_true", help="leave out (c)")
    args = ap.parse_args()

    path, enc, meta = bench.build_workload(2 * 1024**3, 214_748_364, bench.default_cache_dir(), 0, 1, lambda: None)
    with m.open(path, parallelization=0) as f:
        blocks = f.block_offsets()
        lines_index = f.line_offsets()
        total = f.size()

    def opened(file=path, block_map=blocks, lines=lines_index):
        f = m.open(file, parallelization=0)
        f.set_block_offsets(block_map)
        if lines is not None:
            f.set_line_offsets(lines)
        return f

    compiled = {p: m.compile_regex(p) for p in (b"error", b"the", WIDE)}
    if args.trace:
        with opened() as f:
            n, wall = timed(lambda: f.count_matching_lines_regex(compiled[b"error"]))
            emit(step="trace, count_matching_lines_regex, error", lines=n, wall_ms=round(1e3 * wall, 1), decoded_bytes=total)
            n, wall = timed(lambda: f.count_matching_lines_regex(compiled[b"the"]))
            emit(step="trace, count_matching_lines_regex, the", lines=n, wall_ms=round(1e3 * wall, 1))
            (numbers, lines), wall = timed(lambda: f.grep_regex(compiled[b"the"], limit=100_000))
            emit(step="trace, grep_regex, the, limit 100000", lines=len(lines), wall_ms=round(1e3 * wall, 1))
        return

    with opened() as f:                       # warm-up: runtime, kernels, contexts
        fixed = f.count_matching_lines(b"error")
        regex = f.count_matching_lines_regex(compiled[b"error"])
        wide = f.count_matching_lines_regex(compiled[WIDE])
        the = f.count_matching_lines(b"the")
        assert the == f.count_matching_lines_regex(compiled[b"the"])
    emit(step="file", decoded_bytes=total, compressed_bytes=len(enc), lines=max(lines_index.values()),
         chunk_bytes=m._native.regex_chunk_bytes(), matching_lines={"error, fixed": fixed, "error, regex": regex, "wide": wide, "the": the},
         states={"error": compiled[b"error"].states, "wide": compiled[WIDE].states})
    assert fixed == regex

    walls = {"count_matching_lines(b'error')": [], "count_matching_lines_regex(b'error')": [],
             "count_matching_lines_regex(19 states)": [], "count_matches(b'error')": [], "count_matching_lines(b'the')": [],
             "count_matching_lines_regex(b'the')": [], "grep_regex(b'the', limit=100000)": []}
    for rep in range(args.repeats):
        for name, call in (("count_matches(b'error')", lambda f: f.count_matches(b"error")),
                           ("count_matching_lines(b'error')", lambda f: f.count_matching_lines(b"error")),
                           ("count_matching_lines_regex(b'error')", lambda f: f.count_matching_lines_regex(compiled[b"error"])),
                           ("count_matching_lines_regex(19 states)", lambda f: f.count_matching_lines_regex(compiled[WIDE])),
                           ("count_matching_lines(b'the')", lambda f: f.count_matching_lines(b"the")),
                           ("count_matching_lines_regex(b'the')", lambda f: f.count_matching_lines_regex(compiled[b"the"])),
                           ("grep_regex(b'the', limit=100000)", lambda f: len(f.grep_regex(compiled[b"the"], limit=100_000)[1]))):
            with opened() as f:
                got, wall = timed(lambda: call(f))
                walls[name].append(wall)
                emit(step=name, repeat=rep, wall_ms=round(1e3 * wall, 1), result=got, decoded_gb_per_s=round(total / wall / 1e9, 2))
    for name, values in walls.items():
        emit(step="summary, " + name, min_ms=round(1e3 * min(values), 1), max_ms=round(1e3 * max(values), 1))

    if args.skip_headless:
        return
    # (c) no delimiter anywhere: 16 streams of the same 16 MiB
    piece = np.random.default_rng(0x4EAD).integers(0, 255, 16 << 20, dtype=np.uint8)
    piece[piece >= 10] += 1                   # 0 .. 255 without 10
    stream = bz2.compress(piece.tobytes(), 9)
    with tempfile.TemporaryDirectory() as folder:
        headless = os.path.join(folder, "headless.bz2")
        with open(headless, "wb") as out:
            for _ in range(16):
                out.write(stream)
        with m.open(headless, parallelization=0) as f:
            block_map = f.block_offsets()
            size = f.size()
        values = {"count_matches(b'error')": [], "count_matching_lines_regex(b'error')": [],
                  "count_matching_lines_regex(19 states)": []}
        for rep in range(args.repeats + 1):
            for name, call in (("count_matches(b'error')", lambda f: f.count_matches(b"error")),
                               ("count_matching_lines_regex(b'error')", lambda f: f.count_matching_lines_regex(compiled[b"error"])),
                               ("count_matching_lines_regex(19 states)", lambda f: f.count_matching_lines_regex(compiled[WIDE]))):
                with opened(headless, block_map, None) as f:
                    got, wall = timed(lambda: call(f))
                    if rep > 0:               # the first round warms the contexts up for the new sizes
                        values[name].append(wall)
                        emit(step="no delimiter, " + name, repeat=rep - 1, wall_ms=round(1e3 * wall, 1), result=got,
                             decoded_gb_per_s=round(size / wall / 1e9, 2))
        for name, walls in values.items():
            emit(step="summary, no delimiter, " + name, decoded_bytes=size, min_ms=round(1e3 * min(walls), 1),
                 max_ms=round(1e3 * max(walls), 1))


if __name__ == "__main__":
    main()
