"""The four kernels of the refit from device arrays (csrc/bvh_gpu.hip) in this compile (no GPU: hipcc cross-compiles gfx950,
tools/resreport.py): they exist and run without scratch (their per-mesh pointers are kernel arguments compared against
unrolled, never indexed), with no LDS beyond the validation pass's block reduction."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("k_refit_validate", "k_mesh_normals", "k_refit_indexed", "k_light_gather")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_refit_device_kernels_use_no_scratch():
    import resreport
    rows = resreport.report(source="bvh_gpu.hip")
    print()
    for k in KERNELS:   # (they live in an unnamed namespace: looked up by the mangled name, <length><name>E<arguments>)
        hit = [r for r in rows if f"{len(k)}{k}E" in r["mangled"]]
        assert len(hit) == 1, (k, [r["mangled"] for r in rows if "refit" in r["mangled"]])
        r = hit[0]
        print(f"{k:20s} vgpr {r['vgpr']:3d} occ {r['occ']} scratch {r['scratch']} lds {r['lds']}")
        assert r["scratch"] == 0, (k, r)
        assert r["lds"] == (2048 if k == "k_refit_validate" else 0), (k, r)
