"""The HIP-free half of the path numbering (no GPU; tests/path_id.cpp, a stand-alone program compiled with
g++ -fsanitize=address,undefined against csrc/prt_path_id.h and csrc/prt_primary_cache.h alone): encode and decode invert each
other in both orders, the pixel-major decode's magic multiply-high equals id / S and id % S up to id = 2^32 - 1 for every
listed batch size, and the kept primary stage's key tells two stages apart that differ only in the id order or only in the S
their ids were built for."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_path_id_encode_decode_and_stage_key(tmp_path):
    exe = str(tmp_path / "path_id")
    csrc = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", csrc, os.path.join(ROOT, "tests", "path_id.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "path-id host checks passed" in r.stdout and "UNEXPECTED" not in r.stdout
