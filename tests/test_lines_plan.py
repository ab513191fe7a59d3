"""Line access on the CPU: the planner of read_line_ranges / line_starts (indexed_bzip2_amd/csrc/bz2_lines.hpp) under
AddressSanitizer + UBSan -- tests/native/lines_cases.cpp checks launches, boundary queries and resolved pieces against a
byte-by-byte restatement --, the text form of the line index, the argument checks of the Python layer that need no GPU,
and the tool's help."""
import io
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "native", "lines_cases.cpp")
CLI = os.path.join(ROOT, "indexed_bzip2_amd", "ibzip2-mi355x")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_line_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "lines_cases"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-o", str(exe), HARNESS], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "lines ok" in run.stdout


def test_line_offsets_text_round_trip(native, tmp_path):
    offsets = {0: 0, 99_981: 412, 199_962: 412, 299_943: 1_733, 2**40: 2**33 + 5}
    text = io.StringIO()
    native.write_line_offsets(offsets, text)
    assert text.getvalue().splitlines() == ["0,0", "99981,412", "199962,412", "299943,1733", f"{2**40},{2**33 + 5}"]
    assert native.read_line_offsets(io.StringIO(text.getvalue())) == offsets
    path = tmp_path / "lines.txt"
    native.write_line_offsets(offsets, str(path))
    assert native.read_line_offsets(str(path)) == offsets
    assert native.read_line_offsets(io.BytesIO(path.read_bytes())) == offsets
    assert native.read_line_offsets(io.StringIO("")) == {}
    assert native.read_line_offsets(io.StringIO("\n0,0\n\n")) == {0: 0}
    with pytest.raises(ValueError):
        native.read_line_offsets(io.StringIO("0,0\n17\n"))
    # an empty file's index
    text = io.StringIO()
    native.write_line_offsets({0: 0}, text)
    assert text.getvalue() == "0,0\n"


def test_help_lists_count_lines(native):
    assert os.path.exists(CLI)
    run = subprocess.run([CLI, "--help"], capture_output=True, timeout=300)
    assert run.returncode == 0
    assert b"--count-lines" in run.stdout
    assert b"-l, --count-lines" not in run.stdout     # long only: -l lists the compressed offsets


def test_every_line_symbol_is_bound(native):
    names = {name for name, _, _ in native._native.SYMBOLS}
    for name in ("count_byte", "find_byte", "reader_line_offsets", "reader_set_line_offsets", "reader_line_starts",
                 "reader_read_line_ranges", "reader_take_line_ranges"):
        assert "mi355x_bz2_" + name in names
    for method in ("line_offsets", "set_line_offsets", "count_lines", "line_starts", "read_line_ranges", "read_lines",
                   "read_line_ranges_to_tensor"):
        assert callable(getattr(native.reader._IndexedBzip2FileParallel, method))
        assert callable(getattr(native.IndexedBzip2File, method))
    assert native.lib().mi355x_bz2_abi_version() == 2
