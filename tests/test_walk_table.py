"""The tree walk as a table (no GPU): tests/walk_table.cpp runs every combination of the walk facts through prt_plan_walk
(parallelraytracing_amd/csrc/prt_walk.h, plain g++, no HIP) and prints, in one section per component of the outcome (what is
launched; the grids; each resolved tunable), one line per distinct value with the number of combinations behind it and a hash
of their indices: equal sections mean equal components for every index, that is equal outcomes.  tests/golden/walk_table.txt is
what the hand-written launchers gave for the same combinations in the commit before the plan existed.  It was recorded by
compiling that commit's own text into walk_table.cpp in outcome_of's place (-DWALK_TABLE_OUTCOME_FROM): prt_kernels.hip from prt_traverse_takes_primary to the end of
prt_launch_intersect, blocks_for, the two prototypes with default arguments and struct PrtTravTuning of prt_kernels.h,
prt_route_walk8 of prt_route.h, and the choices of walk_rays, run_batch's prt_launch_path call and prt_kernel_occupancy
transcribed from prt_api.cpp; around them stub types, the kernels as variable templates with the kernels' own template heads
(so that default arguments are spelled out), and hipLaunchKernelGGL as a macro that notes kernel, grid, the tunables passed,
the count and list pointers and a preceding k_reset_cursors.

tests/golden/walk_instances.txt lists the 47 walk kernels of that commit's gfx950 assembly (.amdhsa_kernel symbols, demangled)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("walk") / "walk_table")
    b = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC, os.path.join(ROOT, "tests", "walk_table.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def kernels_of(lines):
    return {k for ln in lines if ln.startswith("walk ") for k in re.findall(r"k_\w+<[^>]*>", ln.split(" | ")[1])}


def test_every_combination_of_facts_plans_what_the_old_launchers_launched(table):
    want = open(os.path.join(ROOT, "tests", "golden", "walk_table.txt")).read().splitlines()
    sections = ("walk", "grid", "exit_max", "tri_min", "stack_cap", "steal")
    totals = {sec: sum(int(re.search(r" count=(\d+) ", ln)[1]) for ln in want if ln.startswith(sec + " ")) for sec in sections}
    assert len(want) > 400 and set(totals.values()) == {40451328}, totals    # every section covers every possible combination
    missing = sorted(set(want) - set(table))
    extra = sorted(set(table) - set(want))
    assert not missing and not extra, (missing[:3], extra[:3])
    assert table == want


def test_the_table_launches_exactly_the_walk_instances_there_were(table):
    want = open(os.path.join(ROOT, "tests", "golden", "walk_instances.txt")).read().split("\n")[:-1]
    assert len(want) == len(set(want)) == 47
    assert [sum(k.startswith(p + "<") for k in want) for p in ("k_traverse8_persistent", "k_occluded8_persistent", "k_occluded8_seeded",
                                                               "k_traverse4_persistent", "k_traverse_persistent", "k_intersect")] == [11, 4, 4, 14, 6, 8]
    got = kernels_of(table)
    assert got == set(want), (sorted(set(want) - got), sorted(got - set(want)))
    # the occupancy query's instances are among them
    assert {re.search(r"occupancy=(k_\w+<[^>]*>)", ln)[1] for ln in table if ln.startswith("walk ")} <= set(want)


def test_isa_count_names_the_rows_of_the_list(table):
    """tools/isa_count.py finds its five instances of k_traverse8_persistent by mangled name, typed in; each must be the row of
    that name in PRT_WALK8_ROWS, plain closest hit (STATS, PATH false; PRIM only for `_primary`), and a kernel of the table."""
    import isa_count
    head = open(os.path.join(CSRC, "prt_walk.h")).read()
    body = re.search(r"#define PRT_WALK8_ROWS\(T\) \\\n(.*)\n", head)[1]
    rows = {m[1]: (int(m[2]), int(m[3]), m[4] == "true", m[5] == "true") for m in re.finditer(r"T\((\w+), (\d+), (\d+), (true|false), (true|false)\)", body)}
    assert sorted(rows) == ["deep15_4waves", "inst12_4waves", "lean8_5waves", "wide11_5waves"]
    kernels = kernels_of(table)
    assert len(isa_count.INSTANCES) == 5
    for name, mangled in isa_count.INSTANCES.items():
        m = re.fullmatch(r"k_traverse8_persistentI((?:L[ib]\d+E)+)E", mangled)
        assert m, mangled
        args = [int(v) if t == "i" else v == "1" for t, v in re.findall(r"L([ib])(\d+)E", m[1])]
        prim = name.endswith("_primary")
        L, W, inst, lean = rows[name[:-len("_primary")] if prim else name]
        assert args == [L, W, False, inst, lean, prim, False], (name, args)
        spelled = "k_traverse8_persistent<" + ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in args) + ">"
        assert spelled in kernels, spelled
