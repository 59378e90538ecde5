"""Register budget of the thin-lens ray generation kernels, held to the parent's jittered kernels on the same compile (no
GPU: hipcc cross-compiles gfx950, tools/resreport.py).

k_raygen_lens / k_raygen_lens_env take the branch of raygen_step that jitter takes and keep one more vector (the origin) per
ray in flight; the jittered k_raygen instances already sit at 93-96 VGPRs (5 waves per SIMD) and, with the primitive-BVH walk,
at 128 (4 waves).  A lens instance that spills or drops a wave below the jittered instance with the same ABVH would make the
lens route slower than jitter for no visible reason: this makes it loud.  The yardstick is the jittered kernel of this very
compile, not a number fixed here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_lens_raygen_instances_keep_the_jittered_instances_occupancy():
    import resreport
    rows = {r["name"]: r for r in resreport.report()}
    lens = {n: r for n, r in rows.items() if n.startswith("k_raygen_lens")}
    assert len(lens) == 8, sorted(lens)          # <JITTER, ABVH> x {constant sky, environment image}
    for abvh in ("false", "true"):
        # the jittered instances of k_raygen<JITTER, SAMPLING, ABVH, COMPACT> with this ABVH
        yard = [r for n, r in rows.items() if n.startswith("k_raygen<true, ") and n.endswith(f", {abvh}, false>")]
        assert yard, sorted(rows)
        occ = min(r["occ"] for r in yard)
        for n, r in lens.items():
            if n.endswith(f", {abvh}>"):
                assert r["scratch"] == 0 and r["occ"] >= occ, (n, r, occ)
    # and no lens changed the jittered instances themselves
    for r in (r for n, r in rows.items() if n.startswith("k_raygen<")):
        assert r["scratch"] == 0, r
