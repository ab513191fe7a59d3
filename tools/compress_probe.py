"""Throughput of compress_many on the MI355X against CPython's bz2 on the host's cores.

    python tools/compress_probe.py [--mib 2048] [--level 9] [--piece-mib 9] [--threads 16] [--kind silesia|random]

The corpus (tools/silesia_like.py, or seeded random bytes) is cut into pieces of --piece-mib and compressed
  host    compress_many: host bytes in, host bytes out
  hbm     Decoder.compress_buffers on the kept context: the outputs stay in HBM (the GPU's own share)
  plan    the host's block planner alone (mi355x_bz2_plan_compress_blocks over every piece, 16 threads)
  cpython bz2.compress on --threads threads
and every output is checked with bz2.decompress (sampled) and its size compared with libbz2's.  Prints one JSON line.
"""
import argparse
import bz2
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def corpus(kind, total):
    import numpy as np
    if kind == "random":
        return np.random.Generator(np.random.PCG64(0xBADC0DE)).integers(0, 256, total, dtype=np.uint8).tobytes()
    import silesia_like
    base = silesia_like.generate(min(total, 256 << 20), threads=16)
    base = bytes(base)
    return (base * (total // len(base) + 1))[:total]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=2048)
    ap.add_argument("--level", type=int, default=9)
    ap.add_argument("--piece-mib", type=float, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--kind", default="silesia", choices=["silesia", "random"])
    ap.add_argument("--skip-cpython", action="store_true")
    args = ap.parse_args()
    import indexed_bzip2_amd as m
    from indexed_bzip2_amd import _native as N
    from indexed_bzip2_amd import buffers as B
    total = args.mib << 20
    data = corpus(args.kind, total)
    piece = int(args.piece_mib * (1 << 20))
    view = memoryview(data)
    pieces = [view[i:i + piece] for i in range(0, total, piece)]
    m.compress(b"warm up", args.level)
    t0 = time.perf_counter()
    outs = m.compress_many(pieces, compresslevel=args.level)
    t_host = time.perf_counter() - t0
    dec, lock = B._decoder(-1)
    with lock:
        t0 = time.perf_counter()
        dec.compress_buffers(pieces, args.level)
        t_hbm = time.perf_counter() - t0
    with ThreadPoolExecutor(16) as pool:      # as compress_buffers plans: buffers over 16 threads
        t0 = time.perf_counter()
        list(pool.map(lambda p: N.plan_compress_blocks(p, args.level), pieces))
        t_plan = time.perf_counter() - t0
    for k in range(0, len(pieces), max(1, len(pieces) // 8)):
        assert bz2.decompress(outs[k]) == bytes(pieces[k]), k
    ours = sum(len(o) for o in outs)
    result = {"kind": args.kind, "level": args.level, "input_bytes": total, "pieces": len(pieces),
              "host_to_host_GBps": total / t_host / 1e9, "hbm_resident_GBps": total / t_hbm / 1e9,
              "host_to_host_s": t_host, "hbm_resident_s": t_hbm, "plan_s": t_plan,
              "plan_share_of_host_to_host": t_plan / t_host, "compressed_bytes": ours}
    if not args.skip_cpython:
        with ThreadPoolExecutor(args.threads) as pool:
            t0 = time.perf_counter()
            ref = list(pool.map(lambda p: bz2.compress(p, args.level), pieces))
            t_cpu = time.perf_counter() - t0
        lib = sum(len(r) for r in ref)
        result.update({"cpython_threads": args.threads, "cpython_GBps": total / t_cpu / 1e9, "cpython_s": t_cpu,
                       "libbz2_bytes": lib, "size_vs_libbz2": ours / lib})
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
