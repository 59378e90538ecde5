"""Resource rows of the kernels in csrc/prt_bake_adaptive.hip (no GPU: hipcc cross-compiles gfx950), compiled with the
Makefile's own HIPFLAGS (no contraction: the moments are the film's single fp32 operations).  The unit holds exactly the
kernels DESIGN.md lists ("Bake statistics and adaptive sampling"): k_bka_sum, k_bka_select, k_bka_blocks and k_bka_mean; none
may use scratch, and only the ordered block compaction uses LDS (its sixteen wave totals).  prt_bake.hip and
prt_bake_light.hip keep their own kernel lists (their tests pin them)."""
import os
import re

import pytest

from test_denoise_kernel_resources import CSRC, HIPCC, ROOT
from test_radiance_kernel_resources import resource_rows

KERNELS = ("k_bka_sum", "k_bka_select", "k_bka_blocks", "k_bka_mean")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_unit_holds_its_four_kernels_without_scratch():
    rows = resource_rows("prt_bake_adaptive.hip")
    by_name = {k: [r for n, r in rows.items() if k in n] for k in KERNELS}
    assert all(len(v) == 1 for v in by_name.values()), {k: len(v) for k, v in by_name.items()}
    assert len(rows) == len(KERNELS), sorted(rows)      # a new kernel in the unit is listed here and in DESIGN.md too
    for k, (r,) in by_name.items():
        assert r["scratch"] == 0, (k, r)
        assert r["lds"] == (64 if k == "k_bka_blocks" else 0), (k, r)
    print("\n" + "\n".join(f"{n}: {r}" for n, r in sorted(rows.items())))


def test_design_lists_the_units_kernels():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("#### Bake statistics and adaptive sampling"):]
    section = section[:section.index("\n### ", 1)] if "\n### " in section[1:] else section
    assert set(re.findall(r"`(k_bka_\w+)", section)) == set(KERNELS)


def test_makefile_builds_the_unit_with_hipflags_into_the_library():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^prt_bake_adaptive\.o:[^\n]*prt_bake_adaptive\.hip[^\n]*\n\t([^\n]+)", mk, re.M)
    assert m, "no rule for prt_bake_adaptive.o"
    assert "$(HIPFLAGS)" in m.group(1) and "-ffp-contract=off" in mk
    objs = re.search(r"^OBJS = ([^\n]+)", mk, re.M).group(1).split()
    assert "prt_bake_adaptive.o" in objs and "prt_bake.o" in objs and "prt_bake_light.o" in objs
