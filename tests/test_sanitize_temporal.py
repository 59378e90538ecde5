"""The host half of the temporal reprojection under AddressSanitizer + UBSan (CPU; the GPU pool runs no sanitizers): the
validation fuzzed against an independent statement of its rules, the projection rule and the previous-surface rule driven
with NaN, infinities, z <= 0, huge coordinates and an empty instance list, and the tap index they lead to held inside the
image (tests/sanitize_temporal.cpp, over the HIP-free csrc/prt_temporal_contract.h).  Any report aborts the binary.  Nothing
here is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_temporal_rules_and_validation_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_temporal")
    csrc = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "sanitize_temporal.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "no sanitizer report" in r.stdout and "UNEXPECTED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
