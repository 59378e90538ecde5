"""Resource rows of the kernels in csrc/prt_temporal.hip (no GPU: hipcc cross-compiles gfx950), compiled with the Makefile's
own HIPFLAGS.  None may use scratch: the reprojection is a streaming gather whose tap loop must unroll into registers (the two
3 x 4 matrices of the previous-surface rule included), and scratch would be traffic the contract's byte count does not have."""
import os
import re
import subprocess

import pytest

from test_denoise_kernel_resources import CSRC, HIPCC, makefile_hipflags

KERNELS = ("k_tp_pack_frame", "k_tp_unpack", "k_tp_reprojectILb0", "k_tp_reprojectILb1")   # (<false>: arrays, <true>: the film)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_temporal_kernels_use_no_scratch():
    cmd = [HIPCC] + makefile_hipflags() + ["-c", os.path.join(CSRC, "prt_temporal.hip"), "-o", os.devnull,
                                            "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
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
    by_name = {k: next((r for n, r in rows.items() if k in n), None) for k in KERNELS}
    print(by_name)
    assert all(by_name.values()), by_name
    assert len(rows) == len(KERNELS), sorted(rows)   # a new kernel in the unit is listed here too
    for k, r in by_name.items():
        assert r["scratch"] == 0, (k, r)
    for k in ("k_tp_reprojectILb0", "k_tp_reprojectILb1"):
        assert by_name[k]["occ"] >= 4 and by_name[k]["lds"] <= 16, (k, by_name[k])   # (the block's one 8-byte counter)
