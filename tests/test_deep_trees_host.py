"""Deep trees, host side (no GPU): the gate that keeps tests/test_gpu_deep_trees.py from being vacuous.  Per case of
tests/deep_trees.py the host builder's tree has exactly the named depth and is valid, every level of the comb wins a ray
of the oracle's linear scan, every ray family keeps its share of hits, and by the numpy emulation of the 8-wide walk
(deep_trees.stack_need8) enough rays need the stack rows that no other test reaches.  Values asserted here (and quoted in
the GPU tests' docstrings):

    case   depth8  max_stack4  deepest need (upper estimate = lower estimate of the probe ray)   probe ray on the 4-wide tree
    d9        9       31          7                                                                  3
    d10      10       42          9                                                                  4
    d12      12       49         11                                                                 42
    d15      15       49         13                                                                 43
    d16      16       50         15   (the top row of deep15_4waves and of the PATH instance)       48
    d17      17       57         16                                                                 47
    d19      19       59         18                                                                 54
    p11    1 + 10      -         10   (six placed copies of d10)
    p12    1 + 11      -         11   (six placed copies of d11: the top row of inst12_4waves' 12 entries is 12)

The last column (deep_trees.stack_need4, a lower estimate) is what the 4-wide tree's instances must report under wide = 1:
from 12 levels on it lies beyond the 32 LDS entries of MODE 3, the 27 of MODE 1 / MODE 2 and the 24 of MODE 3's A/B form,
so the overflow list into MODE 1 and MODE 1's spill rows are used.  At 9 and 10 levels the probe ray (chosen for the
8-wide tree) stays shallow on the 4-wide one: the GPU test only prints the figure there.

Relaxed against the plan: in the two-level cases "every level of the comb wins a ray" holds for the levels larger than
2e-6 and for at least 90 % of all levels.  The copies sit 6 units from the origin, where fp32 world coordinates are 5e-7
apart, and the comb's last levels are 3e-8 wide: no world-space ray can be aimed at those.  (The one-level cases, whose
combs sit at the origin, hold the full condition.)

The binary tree of these combs has 13 .. 23 levels (at most 24 for any comb of this family within the 2^-36 size range),
so wide = 0 always runs the 31-entry LDS-only binary instance: the binary spill instance (depth > 32) stays unexercised.
"""
import numpy as np
import pytest

import deep_trees as dt
import scale_cases as sc
import util
from parallelraytracing_amd import capi
from util import prt

DEPTH = {"d9": 9, "d10": 10, "d12": 12, "d15": 15, "d16": 16, "d17": 17, "d19": 19}
STACK4 = {"d9": 31, "d10": 42, "d12": 49, "d15": 49, "d16": 50, "d17": 57, "d19": 59}
UPPER = {"d9": 8, "d10": 9, "d12": 11, "d15": 13, "d16": 15, "d17": 16, "d19": 18}
NEED4 = {"d9": 3, "d10": 4, "d12": 42, "d15": 43, "d16": 48, "d17": 47, "d19": 54}   # the probe ray, lower estimate
SPILLS4 = ("d12", "d15", "d16", "d17", "d19")   # NEED4 > 32: MODE 3 -> MODE 1 and the spill rows (> 27) are used
DEEPEST = {"d9": 7, "d10": 9, "d12": 11, "d15": 13, "d16": 15, "d17": 16, "d19": 18, "p11": 10, "p12": 11}


def _need_floor(name, depth):
    """At least 32 rays need this many entries."""
    if name in dt.PLACED:
        return 10
    return 16 if depth >= 17 else 12 if depth >= 15 else 9 if depth >= 10 else 0


@pytest.mark.parametrize("name", dt.NAMES)
def test_case_has_its_depth_and_its_rays_need_the_upper_rows(name):
    """depth8 is the named value, the tree is valid, max_stack4 <= 90 (the case may go to the GPU: the spill area held
    27 + 64 = 91 entries before it was sized from the tree), every level is some ray's winner, every family hits, and at
    least 32 rays need >= 9 entries (depth8 >= 10), >= 12 (depth8 15 / 16), >= 16 (depth8 >= 17).

    Top rows: at depth8 = 16 the deepest need is exactly depth8 - 1 = 15, the last of the 15 entries of deep15_4waves and
    of the PATH instance (the comb 1.35 / 3 / 70 keeps two internal children under the axis rays at every level; the other
    cases stop one or two entries short of depth8 - 1, which is asserted as attained)."""
    c = dt.case_data(name)
    ratio, per, levels, _, depth = dt.CASES[name]
    r = dt.host(c["scene"])
    info = r.bvh_info()
    n8 = r.bvh_read8()
    _, tris = r.bvh_read()
    _, lv = util.check_bvh8(n8, tris)
    up = dt.stack_need8(r, c["scene"], c["o"], c["d"])
    print(f"{name}: ratio {ratio} per {per} levels {levels}: depth8 {info.depth8}, max_stack4 {info.max_stack4}, binary depth {info.max_depth}, "
          f"{len(c['o'])} rays, need histogram {dt.need_histogram(up)}, probe ray needs {c['probe_need']} (4-wide tree: {c['probe_need4']})")
    assert info.depth8 == depth == lv == DEPTH[name]
    assert info.max_stack4 == STACK4[name] <= 90
    assert c["probe_need4"] == NEED4[name] <= info.max_stack4 and (NEED4[name] > 32) == (name in SPILLS4)
    assert info.max_depth <= 32   # (binary pushes <= 31: the LDS-only binary instance)
    won = np.unique(c["want"]["prim"][c["want"]["prim"] >= 0] // per)
    assert len(won) == levels, sorted(set(range(levels)) - set(won.tolist()))
    shares = dt.hit_shares(c["fam"], c["want"])
    assert min(shares.values()) >= sc.MIN_HIT_SHARE, shares
    floor = _need_floor(name, depth)
    assert int((up >= floor).sum()) >= 32, (floor, dt.need_histogram(up))
    assert up.max() < depth                      # (the walk stacks at most depth8 - 1 groups)
    assert up.max() == UPPER[name] and c["probe_need"] == DEEPEST[name]
    # the lower estimate never exceeds the upper one
    low = dt.stack_need8(r, c["scene"], c["o"], c["d"], c["want"]["d2"])
    assert (low <= up).all()


@pytest.mark.parametrize("name", list(dt.PLACED))
def test_two_level_case_has_its_depth_and_needs_ten_entries(name):
    """Six rotated, scaled copies of a comb under a one-node top level: top_depth + mesh depth is 11 / 12, at least 32 rays
    need >= 10 entries across the level switch, and in the depth-12 case the deepest need is exactly 11."""
    c = dt.case_data(name)
    mname, n, total = dt.PLACED[name]
    r = dt.host(c["scene"])
    info = r.bvh_info()
    mesh_depth = dt.params(mname)[4]
    assert info.depth8 == total and len(c["scene"].instances) == n and 6 <= n <= 10
    one = dt.host(dt.case_scene(mname))
    assert one.bvh_info().depth8 == mesh_depth
    util.check_bvh8(one.bvh_read8(), one.bvh_read()[1])
    up = dt.stack_need8(r, c["scene"], c["o"], c["d"])
    shares = dt.hit_shares(c["fam"], c["want"])
    print(f"{name}: {n} copies of {mname}: depth8 {info.depth8} = {info.depth8 - mesh_depth} + {mesh_depth}, {len(c['o'])} rays, need histogram "
          f"{dt.need_histogram(up)}, probe ray needs {c['probe_need']}, hit share {shares}")
    assert min(shares.values()) >= sc.MIN_HIT_SHARE, shares
    assert int((up >= 10).sum()) >= 32, dt.need_histogram(up)
    assert up.max() == c["probe_need"] == DEEPEST[name] == total - 1
    per = dt.params(mname)[1]
    prim = c["want"]["prim"][c["want"]["prim"] >= 0]
    levels = dt.params(mname)[2]
    # every level of the comb wins in some copy, down to the levels smaller than the fp32 spacing of WORLD coordinates at the
    # copies' distance from the origin (6 units: 5e-7; the comb's last levels are 1.5^-43 = 3e-8): no world ray can be aimed
    # at those
    won = np.unique((prim % (per * levels)) // per)
    size = 1.5 ** -np.arange(levels)
    assert set(np.nonzero(size > 2e-6)[0].tolist()) <= set(won.tolist()) and len(won) >= 0.9 * levels, won


def test_two_level_combination_of_13_is_refused_and_the_scene_stays():
    """Ten copies of the 11-level comb on a ring need two top levels: prt_set_scene refuses 2 + 11 with "too deep".  The same
    ten copies close together fit one top-level node (1 + 11 = 12, accepted); moving them onto the ring with a rebuild of
    the top level is refused the same way, and the context keeps the scene it had, tree and all."""
    mname, n, what = dt.PLACED_REFUSED
    mesh = dt.case_mesh(mname)
    with pytest.raises(prt.PrtError, match="too deep") as e:
        dt.host(dt.placed_scene(mesh, n))
    assert what in str(e.value)
    r = dt.host(dt.clustered_scene(mesh, n))
    assert r.bvh_info().depth8 == 12
    before, table = r.bvh_read8().copy(), r.instances_read()
    with pytest.raises(prt.PrtError, match="too deep") as e:
        r.UpdateInstances(dt.placed_scene(mesh, n), "rebuild")
    assert what in str(e.value)
    assert r.bvh_info().depth8 == 12 and np.array_equal(r.bvh_read8(), before) and r.instance_update_info().updates == 0
    assert all(np.array_equal(v, table[k]) for k, v in r.instances_read().items())


def test_spill_rows_cover_every_tree_the_builder_accepts():
    """prt_spill_rows (include/prt.h): rows per thread behind the 27 LDS entries of the 4-wide spill-capable instance and
    the 31 of the binary one.  64 rows = 91 entries were allocated whatever the tree; the builder accepts trees of
    max_stack4 92 .. 99 (checked here on the CPU only)."""
    rows = capi.lib().prt_spill_rows
    assert rows(0, 0) == 64 and rows(36, 20) == 64 and rows(90, 40) == 64 and rows(27 + 63, 63) == 64
    for s4 in range(0, 200):
        for depth in (0, 1, 31, 32, 33, 63):
            n = rows(s4, depth)
            assert n >= 64 and 27 + n > s4 and 31 + n > depth - 1, (s4, depth, n)
    for name, floor in (("big30", 92), ("big34", 92)):
        info = dt.host(dt.case_scene(name)).bvh_info()
        n = rows(info.max_stack4, info.max_depth)
        print(f"{name}: depth8 {info.depth8}, max_stack4 {info.max_stack4}, binary depth {info.max_depth}: {n} spill rows")
        assert floor <= info.max_stack4 <= 99 and info.max_depth <= 63
        assert 27 + n > info.max_stack4 > 27 + 64 and n > 64
    for name in dt.NAMES:
        info = dt.case_data(name)["info"]
        assert rows(info.max_stack4, info.max_depth) == 64
