"""CPU tests that make the float64 replay of triangle lights (tests/mesh_light_replay.py) credible before any kernel is
compared with it:

  * with sources "analytic" it reproduces lighting_replay.replay exactly (values, tolerances, stability, counts) on two of
    lighting_replay's cases: the loop restated there is the one already trusted;
  * its light set under "all" is the one prt_set_scene builds (host-only context): primitives equal, every interval within 2
    units of 2^-32;
  * on every new case the share of light samples left out as undecidable is within lighting_replay.MAX_UNSTABLE, triangle
    lights are sampled, and scattered segments that meet light-set triangles are weighted;
  * independent anchor: a triangulated rectangle with uniform emission is sampled uniformly over the rectangle, so the mean of
    D_tri's replay follows the float64 law of kind D (tests/lighting_laws.py), which knows nothing of triangles;
  * each of the three wrong estimators is told apart from the right one: more than 1 % of the stable pixel samples move by
    more than 10x their tolerance."""
import numpy as np
import pytest

import closed_form as cf
import lighting_laws as ll
import lighting_replay as lr
import mesh_light_replay as mr
from util import orc, prt

W, H = 160, 120


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in mr.CASES:
        c = mr.case(name, W, H)
        c["osc"] = orc.OracleScene(c["scene"].desc())
        out[name] = c
    return out


@pytest.mark.parametrize("name", ["DEFAULT", "bunny"])
@pytest.mark.parametrize("mode", ["mis", "nee"])
def test_analytic_sources_reproduce_the_existing_replay(name, mode):
    c = lr.case(name, 96, 72)
    osc = orc.OracleScene(c["scene"].desc())
    old = lr.replay_case(c, mode, samples=(0, 5), osc=osc)
    new = mr.replay_case(c, mode, samples=(0, 5), osc=osc, sources="analytic")
    assert np.array_equal(old.value, new.value) and np.array_equal(old.tol, new.tol) and np.array_equal(old.stable, new.stable)
    for f in ("shadow_rays", "shadow_occluded", "n_light_samples", "n_unstable", "n_indifferent", "n_weighted", "segments"):
        assert getattr(old, f) == getattr(new, f), f
    assert old.n_light_samples > 5000


@pytest.mark.parametrize("name", mr.CASES)
def test_light_set_is_the_librarys(cases, name):
    c = cases[name]
    r = prt.HipWavefrontRenderer(device=-1)
    r.set_light_sources("all")
    r.set_scene_host_only(c["scene"])
    prim, pmf = r.light_info()
    ls = mr.MeshLightSet(c["scene"], "all")
    assert np.array_equal(prim.astype(np.int64), ls.prim)
    assert np.all(np.abs(r.light_intervals().astype(np.float64) - ls.width) <= 2.0)
    assert ls.T[-1] == mr.TWO32 and (ls.kind == 2).sum() >= 8
    assert r.light_stats().n_emitters_unsampled == ls.n_unsampled_power


@pytest.mark.parametrize("name", mr.CASES)
@pytest.mark.parametrize("mode", ["mis", "nee"])
def test_unstable_share_is_within_the_cap(cases, name, mode):
    c = cases[name]
    r = mr.replay_case(c, mode, osc=c["osc"])
    share = mr.unstable_share(r)
    print(name, mode, dict(light_samples=r.n_light_samples, triangle_samples=r.n_triangle_samples, shadow_rays=r.shadow_rays,
                           occluded=r.shadow_occluded, unstable=r.n_unstable, indifferent=r.n_indifferent, share=share,
                           weighted=r.n_weighted, triangle_hits_weighted=r.n_triangle_hits_weighted))
    assert r.n_light_samples > 10000 and r.n_triangle_samples > 1000
    assert share <= mr.MAX_UNSTABLE, (name, mode, share)
    assert np.all(np.isfinite(r.value)) and np.all(np.isfinite(r.tol))
    if mode == "mis":
        assert r.n_triangle_hits_weighted > 0
    if name == "bunny_light":      # a closed emissive mesh: the samples that face away come back occluded
        assert r.shadow_occluded > 0.3 * r.shadow_rays
    if name == "penumbra_tri":
        assert r.shadow_occluded > 0.02 * r.shadow_rays
    if name == "D_tri":
        assert r.shadow_occluded == 0


@pytest.mark.parametrize("mode", ["mis", "nee"])
def test_d_tri_mean_follows_the_float64_law_of_kind_d(mode):
    w, h, S, D = 32, 24, 512, 5
    sc, ground, emitter = cf.ground_scene(prt)
    light = ("quad", emitter[0], emitter[1], emitter[2])
    tri = prt.scenes.triangulate_quads(sc)
    cam = cf.camera(prt, "ground", w, h)
    o, d = cf.pixel_rays(lambda px, py: orc.camera_rays(cam.desc(), px, py), w, h)
    law = ll.frame_law(o, d, ground, light, mode, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY, rr=0, clamp=0.0, max_depth=D, q=12)
    r = mr.replay(tri, cam, w, h, D, mr.SEED, range(S), mode, (0, 0, 0.0), stability=False, use_bvh=True)
    X = r.value.sum(1).reshape(S, w * h).mean(0)
    g = law["on_g"] & ~law["excluded"] & (law["var"] > 0)
    assert g.sum() > 300
    z = (X[g] - law["mu"][g]) / np.sqrt(law["var"][g] / S)
    Z = z.sum() / np.sqrt(g.sum())
    print(mode, dict(maxz=float(np.abs(z).max()), Z=float(Z), rel=float(X[g].mean() / law["mu"][g].mean() - 1)))
    assert np.abs(z).max() < 5.5 and abs(Z) < 5.0


# wrong estimator -> (case, mode) on which it must show; chosen for what the case contains, not from the result
SEPARATES = {
    "mesh_area": ("D_tri", "nee"),          # 8 triangles: the mesh's area is 8 times a triangle's
    "wb_one": ("bunny_light", "mis"),       # a large emissive mesh beside the ground: many scattered segments meet it
    "u1_linear": ("D_tri", "nee"),          # points crowd towards v0
}


@pytest.mark.parametrize("wrong", mr.WRONG)
def test_wrong_estimators_are_told_apart(cases, wrong):
    name, mode = SEPARATES[wrong]
    c = cases[name]
    right = mr.replay_case(c, mode, osc=c["osc"])
    other = mr.replay_case(c, mode, wrong=wrong, stability=False, osc=c["osc"])
    share = mr.separated_share(right, other, 10.0)
    print(wrong, name, mode, share)
    assert share > 0.01, (wrong, name, mode, share)
