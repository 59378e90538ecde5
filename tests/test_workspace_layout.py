"""The workspace layout helper (parallelraytracing_amd/csrc/prt_workspace.h) under AddressSanitizer + UBSan (CPU; a stand-alone
program that includes only that header, nothing loaded into Python): regions of 1, 4, 8, 12, 16, 40 and 44 bytes per element at
0, 1, 2, 3, 5, 7, 63, 64, 65 and 2^28 elements in mixed orders of up to 12 regions.  Every start is a multiple of 16, the regions
are disjoint and in declaration order, the total is the end of the last region rounded up by less than 16 and at most the sizes
plus 15 per region; layouts under 1 MiB are allocated at exactly their total and written in full; a capacity one byte short is
refused with no pointer handed out; the same declarations bind to the same offsets; prt_scatter's eight arrays at n = 3 and 7
lie inside their own total (tests/workspace_layout.cpp).  Any report aborts the binary."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_layouts_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "workspace_layout")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "parallelraytracing_amd", "csrc"),
           os.path.join(ROOT, "tests", "workspace_layout.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "no sanitizer report" in r.stdout and "UNEXPECTED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    cases = int(r.stdout.split(" cases")[0].split()[-1])
    assert cases > 30000
