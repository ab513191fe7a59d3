"""Host-side C++ (magic finder, block index, run cache, access-pattern tracker, block finder thread, batch plan) under
AddressSanitizer + UBSan and under ThreadSanitizer: CPU builds only (GPU sanitizers are not available on the pool).  The
harnesses in tests/native/ drive the classes with seeded random operations and exact-size buffers; host_known_answers
replays the answers recorded from the reference's own classes (tests/golden/host_vectors.txt)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
FINDER = os.path.join(ROOT, "indexed_bzip2_amd", "csrc", "bz2_finder.cpp")
VECTORS = os.path.join(ROOT, "tests", "golden", "host_vectors.txt")

CASES = [
    ("finder_sanitize.cpp", "address,undefined", [], "matches"),
    ("host_sanitize.cpp", "address,undefined", [], "host ok"),
    ("host_sanitize.cpp", "thread", [], "host ok"),                      # the finder thread against its consumers
    ("finder_sanitize.cpp", "thread", [], "matches"),
    ("host_known_answers.cpp", "address,undefined", [VECTORS], "known answers ok"),
    # asking threads against a hand-over / an import / a cut of the list at a random moment (the round-2 finder restarted its
    # scan behind a complete list: this harness shows that within ten rounds on that code)
    ("finder_race.cpp", "thread", ["60"], "finder race ok"),
    ("finder_race.cpp", "address,undefined", ["120"], "finder race ok"),
    ("plan_cases.cpp", "address,undefined", [], "plan ok"),           # how a batch is cut into groups and kernel forms
]


ADDR_NO_RANDOMIZE = 0x0040000


def _without_aslr():
    """ThreadSanitizer expects the program within fixed address ranges; kernels that randomise mappings with more bits
    place it outside them ("FATAL: ThreadSanitizer: unexpected memory mapping").  Its harnesses therefore run with address
    randomisation off for that one process (personality(2), what `setarch -R` does)."""
    libc = ctypes.CDLL(None, use_errno=True)
    libc.personality(libc.personality(0xFFFFFFFF) | ADDR_NO_RANDOMIZE)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("harness, sanitizer, args, expect", CASES)
def test_host_code_under_sanitizers(tmp_path, harness, sanitizer, args, expect):
    exe = tmp_path / "harness"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all",
                            "-pthread", "-o", str(exe), os.path.join(NATIVE, harness), FINDER],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600,
                         preexec_fn=_without_aslr if sanitizer == "thread" else None)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert expect in run.stdout
