"""Resource rows of the kernels in csrc/prt_feature_samples.hip (no GPU: hipcc cross-compiles gfx950), compiled with the
Makefile's own HIPFLAGS.  The three kernels of the sampled guide features are listed, and none may use scratch or LDS: the
sample-ray kernel holds one ray, the reduce a pixel's twelve sums, the finish one pixel's records."""
import os
import re
import subprocess

import pytest

from test_guide_features_kernel_resources import CSRC, HIPCC, makefile_hipflags

KERNELS = ("k_fs_rays", "k_fs_reduce", "k_fs_finish")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_feature_sample_kernels_use_no_scratch_and_no_lds():
    cmd = [HIPCC] + makefile_hipflags() + ["-c", os.path.join(CSRC, "prt_feature_samples.hip"), "-o", os.devnull,
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
    print(rows)
    by_name = {k: next((r for n, r in rows.items() if k in n), None) for k in KERNELS}
    assert all(by_name.values()), by_name
    assert len(rows) == len(KERNELS), sorted(rows)   # a new kernel in the unit is listed here too
    for k, r in by_name.items():
        assert r["scratch"] == 0, (k, r)
        assert r["lds"] == 0 and r["occ"] >= 8, (k, r)   # 256-thread streaming kernels: nothing holds their occupancy down
