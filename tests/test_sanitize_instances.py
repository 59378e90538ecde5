"""The host half of prt_set_instance_transforms under AddressSanitizer + UBSan (CPU; the GPU pool runs no sanitizers):
200 random valid transform sets in sequence on the scene of test_instance_motion_host.py (with and without its world mesh),
every 20th result compared with a fresh compile of the moved description, and the invalid sets, which must be refused with
the scene untouched (tests/sanitize_instances.cpp).  Any report aborts the binary."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_instance_updates_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_instances")
    csrc = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "sanitize_instances.cpp"),
           os.path.join(csrc, "prt_host.cpp"), os.path.join(csrc, "bvh.cpp"), os.path.join(csrc, "prt_scene.cpp"), "-pthread",
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "assets", "models"), "200"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "no sanitizer report" in r.stdout and "UNEXPECTED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
