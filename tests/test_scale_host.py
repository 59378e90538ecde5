"""Coordinate scale / offset, host side (no GPU): the host builder's trees stay valid at every case of
tests/scale_cases.py, the ray families keep their share of hits against the oracle's linear scan, and the box test of
the 8-wide walk, replayed in binary32 along the winner's path (tests/boxtest_replay.py), never cuts the winner off."""
import numpy as np
import pytest

import boxtest_replay as bx
import scale_cases as sc
import util
from util import prt


def _host(scene):
    r = prt.HipWavefrontRenderer(device=-1)
    r.set_scene_host_only(scene)
    return r


@pytest.mark.parametrize("name", sc.NAMES)
def test_host_tree_is_valid_at_every_scale(name):
    scene = sc.case_scene(sc.case(name))
    r = _host(scene)
    n8 = r.bvh_read8()
    _, tris = r.bvh_read()
    fill, depth = util.check_bvh8(n8, tris)
    assert util.check_bvh8_tight(n8, tris) == len(n8)
    info = r.bvh_info()
    assert info.n_nodes8 == len(n8) and info.depth8 == depth and info.n_triangles == scene.n_triangles
    V = tris.reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    flat = int((np.linalg.norm(np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]), axis=1) == 0).sum())
    print(f"{name}: {len(n8)} nodes, depth {depth}, fill {np.mean(fill):.2f}, {flat} of {len(V)} triangles without area")


@pytest.mark.parametrize("scale", [2.0 ** -10, 1.0, 2.0 ** 10])
def test_host_two_level_tree_is_valid_with_scaled_copies(scale):
    """Placed copies at instance scales 2^-10 / 1 / 2^10, translations up to 1e4: the library accepts the scene and
    builds a two-level tree of consistent size.  util.check_bvh8 is a ONE-level checker (leaf slots = triangle records
    in world space); it cannot validate the top level or the sub-trees of the combined read-back, so what is checked of
    the structure here is only that, plus the copied mesh's own tree built alone.  That the two-level tree is RIGHT at
    these scales is held by the GPU test's closest hits against the linear scan."""
    scene = sc.placed_scene(scale)
    r = _host(scene)
    info = r.bvh_info()
    assert info.n_nodes8 == len(r.bvh_read8()) > 0 and info.depth8 <= 16
    alone = prt.Scene(preset=None)
    alone.AddMesh(scene.instanced_meshes[0], alone.AddLambertian((1, 1, 1)))
    one = _host(alone)
    util.check_bvh8(one.bvh_read8(), one.bvh_read()[1])
    util.check_bvh8_tight(one.bvh_read8(), one.bvh_read()[1])


def _replay_case(name, dir_min, n=256):
    c = sc.case(name)
    scene = sc.case_scene(c)
    fam = sc.ray_families(scene, np.random.default_rng([11, sc.NAMES.index(name)]), n=n)
    o, d = sc.all_rays(fam)
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
    shares = sc.hit_shares(fam, want)
    r = _host(scene)
    n8 = r.bvh_read8()
    _, tris = r.bvh_read()
    extent = np.abs(tris.reshape(-1, 3, 4)[:, :, :3]).max()
    bad, n_tests = bx.culled_winners(n8, tris, o, d, want, extent, dir_min)
    return fam, shares, bad, n_tests, o, d


@pytest.mark.parametrize("name", sc.NAMES)
def test_boxtest_replay_keeps_the_winner_at_every_scale(name):
    """T8_BOXTEST in binary32, reciprocal +- 1 ulp, along the root-to-leaf path of every ray's oracle winner: tn <= tf at
    every step, with the clamp the kernels are compiled with.  (With the earlier clamp of 1e-30 this fails at 2^30 and
    2^40 for the axis-parallel and the tiny-component families: see test_the_replay_sees_the_overflow_of_the_old_clamp.)"""
    fam, shares, bad, n_tests, o, d = _replay_case(name, bx.kernel_dir_min())
    print(f"{name}: {len(o)} rays, {n_tests} box tests replayed, hit share per family "
          + ", ".join(f"{f} {shares[f]:.2f}" for f in sc.FAMILIES))
    assert min(shares.values()) >= sc.MIN_HIT_SHARE, shares
    for k, (node, child, tn, tf) in bad[:8]:
        print(f"   ray {k}: o {o[k].tolist()} d {d[k].tolist()} culled at node {node} child {child}: tn {tn!r} > tf {tf!r}")
    assert not bad, f"{len(bad)} winners cut off by the box test"


def test_the_replay_sees_the_overflow_of_the_old_clamp():
    """Sensitivity: with |d| < 1e-30 -> +-1e-30, (o +- pad) * 1e30 overflows at 2^30 x the bunny and the root's children
    are cut off for axis-parallel rays; the replay must see that (and nothing at unit scale)."""
    old = np.float32(1e-30)
    _, _, bad, _, _, _ = _replay_case("s1", old)
    assert not bad
    fam, _, bad, _, o, d = _replay_case("s2^30", old)
    n = len(fam["axis"][0])
    k0 = sc.FAMILIES.index("axis") * n
    axis_bad = [k for k, _ in bad if k0 <= k < k0 + n]
    print(f"clamp 1e-30 at 2^30: {len(bad)} winners cut off, {len(axis_bad)} of them axis-parallel; first: {bad[0]}")
    assert len(axis_bad) > 0.1 * n


def test_direction_clamp_is_a_power_of_two_inside_its_bounds():
    """PRT_DIR_MIN (csrc/prt_kernels.h): small enough that the drift t * dir_min along a clamped axis stays far inside the
    pad for every t <= 2 (|o|_1 + extent) (dir_min <= 2^-21 would do: 2^-18 / (2 * 2)), large enough that
    (coordinate + pad) / dir_min is finite while squared distances are (coordinates < 2^63)."""
    m = float(bx.kernel_dir_min())
    assert np.log2(m) == round(np.log2(m))
    assert m <= 2.0 ** -21 / 1024
    assert np.isfinite(np.float32(2.0 ** 64) * (np.float32(1.0) / np.float32(m)) * np.float32(4.0))


def test_transforms_below_the_documented_scale_bound_are_refused():
    """include/prt.h: a placed copy's transform needs a uniform scale above 1e-10 (s^2 > 1e-20 in the similarity check);
    2^-40 is refused with PRT_ERR_INVALID and a message, 2^-30 and a copy at 2^-10 placed 1e4 away are accepted."""
    ico = sc.asset_mesh("icosahedron.ply")

    def scene(scale, at):
        s = prt.Scene(preset=None)
        s.AddInstance(ico, s.AddLambertian((1, 1, 1)), scale=scale, euler_deg=(20.0, 30.0, 40.0), translation=at)
        return s
    with pytest.raises(prt.PrtError, match="uniform scale"):
        _host(scene(2.0 ** -40, (0.0, 0.0, 0.0)))
    _host(scene(2.0 ** -30, (0.0, 0.0, 0.0)))
    _host(scene(2.0 ** -10, (1e4, -1e4, 1e4)))   # (inv * mat = I holds to fp32 in terms of 1e7: relative, not absolute)
    _host(scene(2.0 ** 10, (1e4, -1e4, 1e4)))


def _balls_case(name, dir_min):
    c = sc.case(name)
    scene = sc.balls_scene(c)
    _host(scene)
    fam = sc.ball_rays(scene, np.random.default_rng([29, sc.NAMES.index(name)]))
    o, d = sc.all_rays(fam)
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
    bad, n_tests = bx.analytic_slab_culled(scene, o, d, want, dir_min)
    return fam, sc.hit_shares(fam, want), bad, n_tests, o, d


# (at 2^-40 the primitives' transforms are below the similarity check's scale bound: the library builds no tree over them
# and scans linearly, so there is no slab test to replay)
@pytest.mark.parametrize("name", [n for n in sc.NAMES if n != "s2^-40"])
def test_analytic_slab_replay_keeps_the_winner_at_every_scale(name):
    """scan_analytic<ABVH>'s slab test in binary32 (pad with its quadratic abvh_q term, IEEE reciprocals with the clamp,
    exact fmas, `tn <= tf * 1.0000005f`) on RANDOM_BALLS_MEDIUM moved by every case: the winner's own world box and the
    root, rebuilt here as csrc/prt_scene.cpp builds them, are never cut off."""
    fam, shares, bad, n_tests, o, d = _balls_case(name, bx.kernel_dir_min())
    print(f"{name}: {len(o)} rays, {n_tests} slab tests replayed, hit share per family " + ", ".join(f"{f} {v:.2f}" for f, v in shares.items()))
    assert min(shares.values()) >= sc.MIN_HIT_SHARE, shares
    for k in bad[:6]:
        print(f"   ray {k}: o {o[k].tolist()} d {d[k].tolist()} cut off")
    assert len(bad) == 0, len(bad)


def test_the_analytic_replay_sees_the_overflow_of_the_old_clamp():
    _, _, bad, _, _, _ = _balls_case("s1", np.float32(1e-30))
    assert len(bad) == 0
    fam, _, bad, _, _, _ = _balls_case("s2^30", np.float32(1e-30))
    n = len(fam["axis"][0])
    assert ((bad >= n) & (bad < 2 * n)).sum() > 0.1 * n, len(bad)
