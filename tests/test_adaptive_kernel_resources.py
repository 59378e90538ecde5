"""Resource rows of the kernels that film statistics and tile-adaptive sampling add (no GPU: hipcc cross-compiles gfx950).

k_accumulate_stat streams like k_accumulate and must stay at its occupancy; none of the new kernels may spill: scratch in a
streaming kernel is traffic to memory that the statistics-off build does not have.  The list raygen instances are the
full-record instances of k_raygen behind one more index load and are held to the registers of the widest k_raygen."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_new_kernel_instances_use_no_scratch_and_keep_their_occupancy():
    import resreport
    rows = {r["name"]: r for r in resreport.report()}
    acc = {n: r for n, r in rows.items() if n.startswith("k_accumulate_stat<")}
    gen = {n: r for n, r in rows.items() if n.startswith("k_raygen_list<")}
    assert len(acc) == 4 and len(gen) == 16
    assert "k_tile_select" in rows and "k_tile_compact" in rows
    for n, r in list(acc.items()) + list(gen.items()) + [(k, rows[k]) for k in ("k_tile_select", "k_tile_compact")]:
        assert r["scratch"] == 0, (n, r)
    for n, r in acc.items():
        assert r["vgpr"] <= 64 and r["occ"] >= rows["k_accumulate"]["occ"], (n, r)
    widest = max(r["vgpr"] for n, r in rows.items() if n.startswith(("k_raygen<", "k_raygen_env<", "k_raygen_lens")))
    for n, r in gen.items():
        assert r["vgpr"] <= widest, (n, r, widest)
