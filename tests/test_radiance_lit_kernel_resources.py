"""Resource rows of the kernels in csrc/prt_radiance_lit.hip (no GPU: hipcc cross-compiles gfx950), compiled with the
Makefile's own HIPFLAGS (no contraction: the lit query's arithmetic is the shade kernels').  The unit holds exactly the
kernels DESIGN.md lists ("Light-sampled radiance query"): the start, the six instances of the step (plain, mesh, env,
mesh + env, clus, clus + env: the sample-light test kernels' set), the light kernel and the sum; the Makefile builds it into
the library.  None may use scratch.  The rows are printed beside the row of k_shade_nee_mesh<false, false> of the same
compiler and flags; no VGPR threshold is set: a lower occupancy is recorded in DESIGN.md, it is not a failure."""
import os
import re

import pytest

from test_denoise_kernel_resources import CSRC, HIPCC
from test_radiance_kernel_resources import resource_rows

# <MESHL, ENV, CLUS> as the mangled name spells them
STEPS = {"plain": "k_rdl_stepILb0ELb0ELb0EE", "mesh": "k_rdl_stepILb1ELb0ELb0EE", "env": "k_rdl_stepILb0ELb1ELb0EE",
         "mesh_env": "k_rdl_stepILb1ELb1ELb0EE", "clus": "k_rdl_stepILb1ELb0ELb1EE", "clus_env": "k_rdl_stepILb1ELb1ELb1EE"}
OTHERS = ("k_rdl_start", "k_rdl_light", "k_rdl_sum")
SHADE = "k_shade_nee_meshILb0ELb0EE"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_lit_radiance_unit_holds_its_nine_kernels_without_scratch():
    rows = resource_rows("prt_radiance_lit.hip")
    by_name = {k: next((r for n, r in rows.items() if pat in n), None) for k, pat in list(STEPS.items()) + [(o, o) for o in OTHERS]}
    assert all(by_name.values()), by_name
    assert len(rows) == len(STEPS) + len(OTHERS), sorted(rows)   # a new kernel in the unit is listed here and in DESIGN.md
    for k, r in by_name.items():
        assert r["scratch"] == 0, (k, r)
        assert r["lds"] == (8 if k == "k_rdl_light" else 0), (k, r)     # the light kernel's two block counters
    shade = [r for n, r in resource_rows("prt_kernels.hip").items() if SHADE in n]
    assert len(shade) == 1, "k_shade_nee_mesh<false, false> is not in prt_kernels.hip"
    print("".join(f"\n{k}: {r}" for k, r in by_name.items()) + f"\nk_shade_nee_mesh<false, false>: {shade[0]}")


def test_makefile_builds_the_unit_with_the_kernel_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS = (.*)$", mk, re.M).group(1).split()
    assert "prt_radiance_lit.o" in objs and "prt_radiance_lit.h" in hdrs and "prt_light_device.h" in hdrs
    rule = re.search(r"^prt_radiance_lit\.o: (.*)\n\t(.*)$", mk, re.M)
    assert rule and "prt_light_device.h" in rule.group(1).split() and "$(HIPFLAGS)" in rule.group(2)
    # the light-sampling device functions live in the header alone: the shade kernels' unit includes it where they stood
    kern = open(os.path.join(CSRC, "prt_kernels.hip")).read()
    head = open(os.path.join(CSRC, "prt_light_device.h")).read()
    assert kern.count('#include "prt_light_device.h"') == 1
    for fn in ("sphere_cone_omc", "select_light", "triangle_light", "sample_light", "light_weight", "bsdf_hit_weight", "light_sample_term",
               "env_selected", "sample_environment", "env_sample_term", "env_miss"):
        assert re.search(rf"^PRT_DEV \w+ {fn}\(", head, re.M), fn
        assert not re.search(rf"^PRT_DEV \w+ {fn}\(", kern, re.M), fn
