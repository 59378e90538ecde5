"""The host half of image textures under AddressSanitizer + UBSan (CPU; the GPU pool runs no sanitizers): 300 random texture
sets, half of them invalid in one of fourteen ways, on a scene with world meshes, placed copies and analytic primitives
(valid sets: every table entry checked against the description; invalid ones: refused with the previous tables untouched), and
400 mutated UV-carrying PLY files through the reader, refine and append (tests/sanitize_textures.cpp).  Any report aborts the
binary.  Nothing here is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_texture_sets_and_uv_plys_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_textures")
    csrc = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "sanitize_textures.cpp"),
           os.path.join(csrc, "prt_host.cpp"), os.path.join(csrc, "bvh.cpp"), os.path.join(csrc, "prt_scene.cpp"), "-pthread",
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "assets", "models"), "300", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "no sanitizer report" in r.stdout and "UNEXPECTED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
