"""Resource rows of the kernels in csrc/prt_radiance.hip (no GPU: hipcc cross-compiles gfx950), compiled with the Makefile's
own HIPFLAGS (no contraction: the query's arithmetic is the shade kernels').  The unit holds exactly its three kernels and
none may use scratch: the step kernel carries a path's whole state in registers between its loads and its stores.  The row
of k_rd_step is printed beside the row of k_shade<0, false, false, false, false> of the same compiler and flags; a lower
occupancy is recorded in DESIGN.md ("Radiance query"), it is not a failure."""
import os
import re
import subprocess

import pytest

from test_denoise_kernel_resources import CSRC, HIPCC, makefile_hipflags

KERNELS = ("k_rd_start", "k_rd_step", "k_rd_sum")
SHADE = "k_shadeILi0ELb0ELb0ELb0ELb0EE"   # k_shade<0, false, false, false, false> as the mangled name spells it


def resource_rows(unit):
    cmd = [HIPCC] + makefile_hipflags() + ["-c", os.path.join(CSRC, unit), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    rows, cur = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, ln)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_radiance_unit_holds_three_kernels_without_scratch():
    rows = resource_rows("prt_radiance.hip")
    by_name = {k: next((r for n, r in rows.items() if k in n), None) for k in KERNELS}
    assert all(by_name.values()), by_name
    assert len(rows) == len(KERNELS), sorted(rows)   # a new kernel in the unit is listed here too
    for k, r in by_name.items():
        assert r["scratch"] == 0 and r["lds"] == 0, (k, r)
    shade = [r for n, r in resource_rows("prt_kernels.hip").items() if SHADE in n]
    assert len(shade) == 1, "k_shade<0, false, false, false, false> is not in prt_kernels.hip"
    print(f"\nk_rd_step: {by_name['k_rd_step']}\nk_shade<0, false, false, false, false>: {shade[0]}")
