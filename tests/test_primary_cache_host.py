"""The HIP-free half of the persistent primary stage (no GPU; tests/primary_cache.cpp, a stand-alone program compiled with
g++ -fsanitize=address,undefined against csrc/prt_primary_cache.h alone): prt_primary_reusable holds for equal keys of an
eligible batch, fails when any single field of the key or of the route plan differs, fails from and for a cleared key, and
fails for a jittered, lens, listed or instrumented batch whatever the held key says.  The program names every field through
structured bindings, so a field added to the key without a case stops it compiling."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_key_comparison_field_by_field(tmp_path):
    exe = str(tmp_path / "primary_cache")
    csrc = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", csrc, os.path.join(ROOT, "tests", "primary_cache.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "primary-cache host checks passed" in r.stdout and "UNEXPECTED" not in r.stdout
