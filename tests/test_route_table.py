"""The route of a batch as a table (no GPU): tests/route_table.cpp runs every combination of the batch facts through
prt_plan_route (parallelraytracing_amd/csrc/prt_route.h, plain g++, no HIP) and prints one line per distinct plan with the number
of combinations behind it and a hash of their indices.  tests/golden/route_table.txt is what the hand-written launchers and the
four route expressions of run_batch gave for the same combinations in the commit before the plan existed (recorded by compiling
that commit's launch section with hipLaunchKernelGGL redefined to note the kernel's name).  Every instance the table names
must be a kernel of the current compile (tools/resreport.py)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELDS = ("raygen", "shade0", "shade", "accumulate")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "route_table")
    b = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "parallelraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tests", "route_table.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def instance_names(lines):
    names = set()
    for ln in lines:
        for f in FIELDS:
            v = ln.split(f" {f}=")[1]
            for g in FIELDS + ("count",):
                v = v.split(f" {g}=")[0]
            names.add(v)
    return names - {"-"}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_every_combination_of_facts_plans_what_the_old_launchers_launched(table):
    want = open(os.path.join(ROOT, "tests", "golden", "route_table.txt")).read().splitlines()
    assert len(want) > 1000 and len(instance_names(want)) == 35 + 52 + 6
    missing = sorted(set(want) - set(table))
    extra = sorted(set(table) - set(want))
    assert not missing and not extra, (missing[:5], extra[:5])
    assert table == want


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs g++ and hipcc")
def test_every_planned_instance_is_a_kernel_of_this_compile(table):
    import resreport
    kernels = {r["name"] for r in resreport.report()}
    names = instance_names(table)
    assert names and not sorted(names - kernels), sorted(names - kernels)
