"""The cluster builder of clustered light selection under AddressSanitizer + UBSan (CPU; a stand-alone program, nothing loaded
into Python): scenes with emissive meshes and placed copies, among them zero-area and coincident triangles, one light and no
light, every max_clusters from 1 to 64 with the contract's invariants checked, then 100 random instance transform sets through
the rebuild, compared with fresh compiles of the moved description (tests/sanitize_light_clusters.cpp).  Any report aborts
the binary."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cluster_builder_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_light_clusters")
    csrc = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "sanitize_light_clusters.cpp"),
           os.path.join(csrc, "prt_host.cpp"), os.path.join(csrc, "bvh.cpp"), os.path.join(csrc, "prt_scene.cpp"), "-pthread",
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "assets", "models"), "100"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "no sanitizer report" in r.stdout and "UNEXPECTED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
