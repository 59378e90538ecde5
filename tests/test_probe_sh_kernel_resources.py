"""Resource rows of the kernels in csrc/prt_probe_sh.hip (no GPU: hipcc cross-compiles gfx950), compiled with the Makefile's
own HIPFLAGS (no contraction: the basis and the products are the operations they spell).  The unit holds exactly its two
kernels and neither may use scratch or LDS (the wave total of the segments is exchanged through lane shuffles)."""
import os

import pytest

from test_denoise_kernel_resources import HIPCC
from test_radiance_kernel_resources import resource_rows

KERNELS = ("k_sh_rays", "k_sh_project")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_probe_sh_unit_holds_its_two_kernels_without_scratch():
    rows = resource_rows("prt_probe_sh.hip")
    by_name = {k: next((r for n, r in rows.items() if k in n), None) for k in KERNELS}
    assert all(by_name.values()), by_name
    assert len(rows) == len(KERNELS), sorted(rows)   # a new kernel in the unit is listed here too
    for k, r in by_name.items():
        assert r["scratch"] == 0 and r["lds"] == 0, (k, r)
    print("\n" + "\n".join(f"{k}: {r}" for k, r in by_name.items()))
