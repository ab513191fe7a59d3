"""Block cuts of the encoder (mi355x_bz2_plan_compress_blocks, host only) against libbz2's: the decoded size of every
block of bz2.compress(x, level), found by cutting its output at the block magics and decoding each block as a one-block
stream.  And the launch planner (indexed_bzip2_amd/csrc/bz2_compress.hpp) under AddressSanitizer + UBSan:
tests/native/compress_cases.cpp."""
import bz2
import os
import shutil
import subprocess

import pytest

import datagen
from conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "native", "compress_cases.cpp")


def _libbz2_block_sizes(x, level):
    """Decoded sizes of the blocks of bz2.compress(x, level) (the stitch of tools/bz2build.py, in reverse)."""
    import indexed_bzip2_amd._native as N
    enc = bz2.compress(x, level)
    starts = N.find_magic(enc, N.MAGIC_BLOCK)
    eos = N.find_magic(enc, N.MAGIC_EOS)
    bounds = starts + [eos[-1]]
    bits = "".join(f"{b:08b}" for b in enc)
    sizes = []
    for a, b in zip(bounds, bounds[1:]):
        body = bits[a:b]
        crc = body[48:80]
        stream = "".join(f"{c:08b}" for c in b"BZh" + str(level).encode()) + body + f"{0x177245385090:048b}" + crc
        stream += "0" * (-len(stream) % 8)
        sizes.append(len(bz2.decompress(int(stream, 2).to_bytes(len(stream) // 8, "big"))))
    return sizes


def _at_cut(level, tail):
    limit = 100000 * level - 19
    return bytes(i % 251 for i in range(limit - 2)) + tail


def _inputs(level):
    cases = {
        "empty": b"",
        "one": b"x",
        "text": datagen.text_like(1_300_000 if level == 9 else 450_000),
        "random": datagen.random_bytes(250_000),
        "runs": datagen.runs(600_000 if level == 9 else 300_000),
        "long_run_across_cut": _at_cut(level, b"r" * 300_000 + datagen.random_bytes(5000)),
        "ends_at_cut": bytes(i % 251 for i in range(100000 * level - 19)),
    }
    for run in (3, 4, 5, 255, 256, 259):
        cases[f"run{run}_at_cut"] = _at_cut(level, b"q" * run + b"after")
    return cases


@pytest.mark.parametrize("level", [1, 2, 9])
def test_block_cuts_match_libbz2(native, level):
    for name, x in _inputs(level).items():
        assert native.plan_compress_blocks(x, level) == _libbz2_block_sizes(x, level), name


def test_plan_rejects_levels(native):
    for bad in (0, 10):
        with pytest.raises(native.Bz2Error):
            native.plan_compress_blocks(b"abc", bad)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "compress_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "compress plan ok" in run.stdout
