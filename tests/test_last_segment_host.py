"""The HIP-free half of the last-segment route (no GPU; tests/last_segment_host.cpp, compiled alone against prt_route.h and
prt_scene.cpp): the plan's last_segment is the tunable exactly when the batch is not the path instance, does not fuse, is not
lit, has no emissive triangle, has a tree, walks it with the persistent kernels, does not sort its rays and has max_depth >= 2,
over every combination of the facts, and 0 otherwise, and on rows written by hand from the headline batch's facts that do not
lean on the plan's own path / fuse / walk8; mesh_emissive is true for an emissive mesh and for an emissive placed
copy, false for the benchmark scene's materials and for scenes whose only emitters are analytic."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_route_decision_and_scene_fact(tmp_path):
    exe = str(tmp_path / "last_segment_host")
    csrc = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "last_segment_host.cpp"), os.path.join(csrc, "prt_host.cpp"), os.path.join(csrc, "bvh.cpp"),
           os.path.join(csrc, "prt_scene.cpp"), "-pthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "assets", "models")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "last-segment host checks passed" in r.stdout and "UNEXPECTED" not in r.stdout
