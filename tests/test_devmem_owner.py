"""The owners of a context's device memory (parallelraytracing_amd/csrc/prt_devmem.h), without a GPU.

1. tests/devmem_owner.cpp under AddressSanitizer + UBSan: a stand-alone program that includes only that header and defines its
   seam over malloc, with a fake allocator that counts live blocks and bytes and can fail the k-th allocation.  A
   default-constructed owner frees nothing; one alloc and one destruction balance; ensure with need <= bytes keeps the pointer
   and makes no call; a growing ensure frees before it allocates (never two live blocks); a failed ensure leaves p == nullptr,
   bytes == 0 and nothing to free; alloc_copy of 0 bytes allocates the minimum and copies nothing; move construction and
   assignment transfer ownership, assignment frees the target's old block once, self-move is harmless; adopt then destruction
   frees once, take then destruction frees nothing; a struct of five owners whose k-th allocation fails (k = 0..4, the third
   among them) leaves no live block and no live byte; the pinned and event owners balance the same way.
2. prt_api.cpp names hipMalloc, hipFree, hipHostMalloc, hipHostFree, hipEventCreate and hipEventDestroy only inside the seam's
   definitions."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallelraytracing_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_owners_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "devmem_owner")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "devmem_owner.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "no sanitizer report" in r.stdout and "UNEXPECTED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert " 0 unexpected" in r.stdout
    assert int(r.stdout.split(" checks")[0].split()[-1]) >= 80


SEAM = ("prt_dev_alloc", "prt_dev_free", "prt_pinned_alloc", "prt_pinned_free", "prt_event_create", "prt_event_destroy")
CALLS = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|hipEventCreate|hipEventCreateWithFlags|hipEventDestroy)\s*\(")


def test_raw_allocation_calls_only_in_the_seam():
    src = open(os.path.join(CSRC, "prt_api.cpp")).read()
    # the body of each seam function: from its definition at column 0 to the closing brace at column 0 or the end of a one-liner
    inside = []
    for name in SEAM:
        m = re.search(r"^(?:int|void) %s\([^)]*\) \{" % name, src, re.M)
        assert m, f"{name} is not defined in prt_api.cpp"
        end = src.index("\n", m.end()) if src[m.end():src.index("\n", m.end())].rstrip().endswith("}") else src.index("\n}", m.end())
        inside.append((m.start(), end))
    seen = set()
    for m in CALLS.finditer(src):
        assert any(a <= m.start() < b for a, b in inside), f"{m.group(1)} at line {src.count(chr(10), 0, m.start()) + 1} is outside the seam"
        seen.add(m.group(1))
    assert seen >= {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipEventCreate", "hipEventDestroy"}
