"""The host half of the SH probes under AddressSanitizer + UBSan (CPU; the GPU pool runs no sanitizers): the basis and the
irradiance rule over exactly sized arrays of every order, with NaN, infinities, huge and non-unit directions, held to the
addition theorem, to orthonormality and to the constant sky's closed form, and their refusals (tests/sanitize_probe_sh.cpp,
over the HIP-free csrc/prt_sh_contract.h alone).  Any report aborts the binary.  Nothing here is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_sh_basis_and_irradiance_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_probe_sh")
    csrc = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", csrc, os.path.join(ROOT, "tests", "sanitize_probe_sh.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "no sanitizer report" in r.stdout and "UNEXPECTED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
