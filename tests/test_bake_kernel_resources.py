"""Resource rows of the kernels in csrc/prt_bake.hip (no GPU: hipcc cross-compiles gfx950), compiled with the Makefile's own
HIPFLAGS (no contraction: the coverage rule and the interpolation are the operations they spell).  The unit holds exactly
its six kernels and none may use scratch; only the compaction kernel uses LDS (its sixteen wave totals)."""
import os

import pytest

from test_denoise_kernel_resources import HIPCC
from test_radiance_kernel_resources import resource_rows

KERNELS = ("k_bk_cover", "k_bk_surface", "k_bk_compact", "k_bk_rays", "k_bk_sum", "k_bk_dilate")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_bake_unit_holds_its_six_kernels_without_scratch():
    rows = resource_rows("prt_bake.hip")
    by_name = {k: next((r for n, r in rows.items() if k in n), None) for k in KERNELS}
    assert all(by_name.values()), by_name
    assert len(rows) == len(KERNELS), sorted(rows)   # a new kernel in the unit is listed here too
    for k, r in by_name.items():
        assert r["scratch"] == 0, (k, r)
        assert r["lds"] == (64 if k == "k_bk_compact" else 0), (k, r)
    print("\n" + "\n".join(f"{k}: {r}" for k, r in by_name.items()))
