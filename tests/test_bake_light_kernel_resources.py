"""Resource rows of the kernels in csrc/prt_bake_light.hip (no GPU: hipcc cross-compiles gfx950), compiled with the Makefile's
own HIPFLAGS (no contraction: the light sample is the shade kernels' arithmetic).  The unit holds exactly the kernels
DESIGN.md lists ("The texel's light sample"): the six instances of k_bkl_sample<MESHL, ENV, CLUS> and k_bkl_add; none may
use scratch or LDS.  The Makefile builds the unit with $(HIPFLAGS) and links it into libprt.so."""
import os
import re

import pytest

from test_denoise_kernel_resources import CSRC, HIPCC, ROOT
from test_radiance_kernel_resources import resource_rows

# k_bkl_sample<MESHL, ENV, CLUS> as the mangled names spell the template arguments
SAMPLE_INSTANCES = ("Lb0ELb0ELb0E", "Lb0ELb1ELb0E", "Lb1ELb0ELb0E", "Lb1ELb1ELb0E", "Lb1ELb0ELb1E", "Lb1ELb1ELb1E")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_bake_light_unit_holds_its_seven_kernels_without_scratch():
    rows = resource_rows("prt_bake_light.hip")
    sample = {t: next((r for n, r in rows.items() if "k_bkl_sample" in n and t in n), None) for t in SAMPLE_INSTANCES}
    add = [r for n, r in rows.items() if "k_bkl_add" in n]
    assert all(sample.values()), sample
    assert len(add) == 1
    assert len(rows) == len(SAMPLE_INSTANCES) + 1, sorted(rows)   # a new kernel in the unit is listed here and in DESIGN.md too
    for n, r in rows.items():
        assert r["scratch"] == 0 and r["lds"] == 0, (n, r)
    print("\n" + "\n".join(f"{n}: {r}" for n, r in sorted(rows.items())))


def test_design_lists_the_units_kernels():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("#### The texel's light sample"):]
    section = section[:section.index("\n### ", 1)] if "\n### " in section[1:] else section
    listed = set(re.findall(r"`(k_bkl_\w+)", section))
    assert listed == {"k_bkl_sample", "k_bkl_add"}, listed
    assert "<MESHL, ENV, CLUS>" in section and "six instances" in section


def test_makefile_builds_the_unit_with_hipflags_into_the_library():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^prt_bake_light\.o:[^\n]*prt_bake_light\.hip[^\n]*\n\t([^\n]+)", mk, re.M)
    assert m, "no rule for prt_bake_light.o"
    assert "$(HIPFLAGS)" in m.group(1) and "-ffp-contract=off" in mk
    objs = re.search(r"^OBJS = ([^\n]+)", mk, re.M).group(1).split()
    assert "prt_bake_light.o" in objs and "prt_bake.o" in objs
