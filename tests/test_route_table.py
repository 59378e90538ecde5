"""The route of a batch as a table (no GPU): tests/route_table.cpp runs every combination of the batch facts through
prt_plan_route (parallelraytracing_amd/csrc/prt_route.h, plain g++, no HIP) and prints one line per distinct plan with the number
of combinations behind it and a hash of their indices.  tests/golden/route_table.txt is what the hand-written launchers and the
four route expressions of run_batch gave for the same combinations in the commit before the plan existed (recorded by compiling
that commit's launch section with hipLaunchKernelGGL redefined to note the kernel's name).  Every instance the table names
must be a kernel of the current compile (tools/resreport.py).

The golden table was recorded before clustered light selection and keeps light_clusters = false.  A second pass
(route_table clusters) plans every combination with light_clusters false and true and the test below states, in words of its
own and not through the plan's index arithmetic, how the two plans may differ; the names of both passes together are exactly the
lists the library enumerates (prt_instance_name)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELDS = ("raygen", "shade0", "shade", "accumulate")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("route") / "route_table")
    b = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "parallelraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tests", "route_table.cpp"), "-o", out], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def table(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def clusters(exe):
    r = subprocess.run([exe, "clusters"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def plan_fields(text):
    """'path=0 ... raygen=k_raygen<..> shade0=.. shade=.. accumulate=..' -> dict of its ten fields"""
    keys = ("path", "compact", "walk", "fuse", "primary_hit", "walk8") + FIELDS
    m = re.fullmatch(" ".join(f"{k}=(?P<{k}>.+?)" for k in keys), text.strip())
    assert m, text
    return m.groupdict()


def clustered_name(name):
    """The shade instance that stands in `name`'s place when the light set has triangle lights and clustered selection is on."""
    m = re.fullmatch(r"k_shade_nee_mesh<(\w+), (\w+)>", name)
    if m:
        return f"k_shade_nee_clus<{m[1]}, {m[2]}>"
    m = re.fullmatch(r"k_shade_nee_mesh_env<(\w+), (\w+)>", name)
    if m:
        return f"k_shade_nee_clus_env<{m[1]}, {m[2]}>"
    m = re.fullmatch(r"k_shade_nee_tex<(\w+), (\w+), true, (\w+)>", name)
    if m:
        return f"k_shade_nee_clus_tex<{m[1]}, {m[2]}, {m[3]}>"
    return None


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


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_clustered_selection_only_renames_the_mesh_light_shade_instances(table, clusters):
    """Every combination of the other facts, planned with light_clusters false and true (201,326,592 possible combinations of
    the golden table's facts).  With lit && mesh_lights and the path route not taken, the shade instance is the clustered one
    of the same family and arguments (clustered_name), shade0 follows shade unless the route is compact, and every other field
    is equal; in every other combination the two plans are identical.  The names of both passes are the library's lists."""
    from util import prt
    total = 0
    seen = set()
    for ln in clusters:
        m = re.fullmatch(r"mesh_lit=([01]) \| (.+) \| (.+) count=(\d+)", ln)
        assert m, ln
        off, on = plan_fields(m[2]), plan_fields(m[3])
        total += int(m[4])
        seen |= {p[f] for p in (off, on) for f in FIELDS} - {"-"}
        if m[1] == "1" and off["path"] == "0":
            want = dict(off, shade=clustered_name(off["shade"]))
            assert want["shade"] is not None, ln
            want["shade0"] = off["shade0"] if off["compact"] == "1" else want["shade"]
            assert on == want, ln
            assert off["compact"] == "0"          # (a lit batch never takes the compact route: shade0 followed shade above)
        else:
            assert on == off, ln
            assert clustered_name(off["shade"]) is None or m[1] == "0" or off["path"] == "1", ln
    assert total == sum(int(ln.rsplit(" count=", 1)[1].split()[0]) for ln in table)
    assert sum(m == "1" for m in (ln[9] for ln in clusters)) > 100
    lists = {st: set(prt.instance_names(st)) for st in ("raygen", "shade", "accumulate")}
    assert [len(lists[st]) for st in ("raygen", "shade", "accumulate")] == [35, 68, 6]
    assert prt.instance_names("shade0") == prt.instance_names("shade")
    assert seen == lists["raygen"] | lists["shade"] | lists["accumulate"], sorted(seen ^ (lists["raygen"] | lists["shade"] | lists["accumulate"]))
    assert seen - instance_names(table) == {n for n in lists["shade"] if n.startswith("k_shade_nee_clus")}


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs g++ and hipcc")
def test_every_planned_instance_is_a_kernel_of_this_compile(table, clusters):
    import resreport
    kernels = {r["name"] for r in resreport.report()}
    names = instance_names(table)
    for ln in clusters:      # and what clustered selection plans in their place
        names |= {plan_fields(ln.split(" | ")[2].rsplit(" count=", 1)[0])[f] for f in FIELDS} - {"-"}
    assert len(names) == 35 + 68 + 6
    assert names and not sorted(names - kernels), sorted(names - kernels)
