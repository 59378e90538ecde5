"""Resource rows of the kernels in csrc/prt_features.hip (no GPU: hipcc cross-compiles gfx950), compiled with the Makefile's
own HIPFLAGS.  Both kernels of the guide features through specular chains are listed, and neither may use scratch: a chain's
state is a handful of registers moved with its ray, and scratch in a streaming kernel is traffic the pass does not have."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_ft_start", "k_ft_step")


def makefile_hipflags():
    """HIPFLAGS as csrc/Makefile spells them, with CXXFLAGS and ARCH expanded and EXTRA empty."""
    var = {}
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"(CXXFLAGS|HIPFLAGS|ARCH)\s*\??=\s*(.*)", line)
        if m:
            var[m.group(1)] = m.group(2).strip()
    flags = var["HIPFLAGS"].replace("$(CXXFLAGS)", var["CXXFLAGS"]).replace("$(ARCH)", var["ARCH"]).replace("$(EXTRA)", "")
    assert "$(" not in flags and "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags
    return flags.split()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_guide_feature_kernels_use_no_scratch():
    cmd = [HIPCC] + makefile_hipflags() + ["-c", os.path.join(CSRC, "prt_features.hip"), "-o", os.devnull,
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
    assert all(by_name.values()), by_name
    assert len(rows) == len(KERNELS), sorted(rows)   # a new kernel in the unit is listed here too
    for k, r in by_name.items():
        assert r["scratch"] == 0, (k, r)
        assert r["lds"] == 0 and r["occ"] >= 8, (k, r)   # a 256-thread streaming kernel: nothing holds its occupancy down
