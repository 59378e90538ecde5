"""CPU tests that make the float64 replay of light-sampled frames (tests/lighting_replay.py) credible:

  * its path walker equals OracleScene.render bit for bit (film and ray count), with jitter, roulette and clamp on and off, on
    every replayed scene;
  * the share of light samples it has to leave out as undecidable is within the cap on every replayed scene;
  * its light set is the one prt_set_scene builds (host-only context);
  * independent anchor: on kinds D and E its mean over many samples matches the float64 quadrature of
    tests/lighting_laws.py, which was written without reference to the sampler;
  * every listed wrong estimator is told apart from the right one on a named scene: more than 1 % of the stable pixel
    samples move by more than 10x their tolerance."""
import numpy as np
import pytest

import closed_form as cf
import lighting_laws as ll
import lighting_replay as lr
from parallelraytracing_amd.capi import PrtSampling
from util import orc, prt

W, H = 160, 120


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in lr.CASES:
        c = lr.case(name, W, H)
        c["osc"] = orc.OracleScene(c["scene"].desc())
        out[name] = c
    return out


@pytest.mark.parametrize("name", lr.CASES)
def test_walker_equals_the_oracle_bit_for_bit(cases, name):
    c = cases[name]
    pix = np.arange(W * H)
    samples = (0, 5)
    apix = np.tile(pix, len(samples))
    asamp = np.repeat(samples, len(pix))
    for smp in {(0, 0, 0.0), (0, 1, 1.0), (1, 2, 0.5), c["sampling"]}:
        _, delivered, _, segs = lr.walk(c["scene"], c["osc"], c["cam"], W, H, c["depth"], lr.SEED, apix, asamp, smp,
                                        use_bvh=c["use_bvh"])
        total = 0
        for s in samples:
            a, w, rays = c["osc"].render(c["cam"].desc(), W, H, spp=1, first_sample=s, max_depth=c["depth"], seed=lr.SEED,
                                         iterative=True, use_bvh=c["use_bvh"], n_threads=lr.n_threads_default(),
                                         sampling=PrtSampling(*smp))
            total += rays
            assert np.array_equal(a.reshape(-1, 3).view(np.uint32), delivered[asamp == s].view(np.uint32)), (name, smp, s)
            assert np.all(w == 1.0)
        assert segs == total, (name, smp)
    # and the film of several samples, added in sample order
    smp = c["sampling"]
    _, delivered, _, _ = lr.walk(c["scene"], c["osc"], c["cam"], W, H, c["depth"], lr.SEED, apix, asamp, smp, use_bvh=c["use_bvh"])
    acc = np.zeros((H, W, 3), np.float32)
    wts = np.zeros((H, W), np.float32)
    for s in samples:
        c["osc"].render(c["cam"].desc(), W, H, spp=1, first_sample=s, max_depth=c["depth"], seed=lr.SEED, iterative=True,
                        use_bvh=c["use_bvh"], n_threads=lr.n_threads_default(), sampling=PrtSampling(*smp), accum=acc, weights=wts)
    mine, _ = lr.film_from_delivered(delivered, apix, asamp, W, H)
    assert np.array_equal(mine.view(np.uint32), acc.view(np.uint32))


def test_rng_restatement_is_the_oracles():
    rng = np.random.default_rng(1)
    for st in rng.integers(0, 2 ** 32, 50, dtype=np.uint64):
        want, after = orc.random_floats(int(st), 3)
        s = np.array([st], np.uint32)
        for k in range(3):
            u, s = lr.rnd(s)
            assert np.float32(u[0]) == want[k]
        assert int(s[0]) == after


@pytest.mark.parametrize("name", lr.CASES)
def test_light_set_is_the_librarys(cases, name):
    c = cases[name]
    r = prt.HipWavefrontRenderer(device=-1)
    r.set_scene_host_only(c["scene"])
    prim, pmf = r.light_info()
    ls = lr.LightSet(c["scene"])
    assert np.array_equal(prim.astype(np.int64), ls.prim)
    np.testing.assert_allclose(pmf.astype(np.float64), ls.pmf, rtol=1e-6)
    assert ls.n >= 1


@pytest.mark.parametrize("name", lr.CASES)
@pytest.mark.parametrize("mode", ["mis", "nee"])
def test_unstable_share_is_within_the_cap(cases, name, mode):
    c = cases[name]
    r = lr.replay_case(c, mode, osc=c["osc"])
    share = lr.unstable_share(r)
    print(name, mode, dict(light_samples=r.n_light_samples, shadow_rays=r.shadow_rays, occluded=r.shadow_occluded,
                           unstable=r.n_unstable, indifferent=r.n_indifferent, share=share))
    assert r.n_light_samples > 10000
    assert share <= lr.MAX_UNSTABLE, (name, mode, share)
    assert np.all(np.isfinite(r.value)) and np.all(np.isfinite(r.tol))
    if name in ("DEFAULT", "RANDOM_BALLS_SMALL", "penumbra", "bunny", "placed", "specular"):
        assert r.shadow_occluded > 0.02 * r.shadow_rays      # the case has shadows
    if name == "resting":   # vertices on both sides of the sphere margin
        v = lr.walk(c["scene"], c["osc"], c["cam"], W, H, c["depth"], lr.SEED, np.arange(W * H), np.zeros(W * H, int))[0][0]
        g = v["hit"]["prim"] == 0
        D = np.linalg.norm(v["hit"]["position"][g].astype(np.float64) - r.lights.c[0], axis=1)
        inside = D <= r.lights.R[0] * (1 + lr.SPHERE_MARGIN)
        assert inside.sum() >= 20 and (~inside).sum() >= 1000, (inside.sum(), (~inside).sum())


def test_off_mode_is_the_walker():
    c = lr.case("DEFAULT", 64, 48)
    r = lr.replay_case(c, "off", samples=(0,))
    assert np.array_equal(r.value.astype(np.float32).view(np.uint32), r.delivered.view(np.uint32))
    assert r.shadow_rays == 0 and r.stable.all()


# ---- independent anchor: the float64 laws of kinds D and E -----------------------------------------------------------------
def _kind(kind):
    sc, ground, emitter = cf.ground_scene(prt)
    light = ("quad", emitter[0], emitter[1], emitter[2])
    if kind == "E":
        sc = prt.Scene(preset=None, sky=cf.SKY)
        g = sc.AddLambertian(cf.GROUND_ALBEDO)
        e = sc.AddEmissive(cf.EMISSION)
        sc.AddQuad(20.0, 20.0, g, translation=(0.0, -1.0, 0.0))
        sc.AddCircle(1.0, e, translation=(0.0, 4.0, 0.0))
        light = ("sphere", (0.0, 4.0, 0.0), 1.0)
    return sc, ground, light


@pytest.mark.parametrize("kind", ["D", "E"])
@pytest.mark.parametrize("mode", ["mis", "nee"])
@pytest.mark.parametrize("sampling", [(0, 0, 0.0), (0, 1, 1.0)])
def test_replay_mean_follows_the_float64_laws(kind, mode, sampling):
    w, h, S, D = 32, 24, 512, 5
    sc, ground, light = _kind(kind)
    cam = cf.camera(prt, "ground", w, h)
    o, d = cf.pixel_rays(lambda px, py: orc.camera_rays(cam.desc(), px, py), w, h)
    law = ll.frame_law(o, d, ground, light, mode, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY, rr=sampling[1], clamp=sampling[2],
                       max_depth=D, q=12)
    r = lr.replay(sc, cam, w, h, D, lr.SEED, range(S), mode, sampling, stability=False)
    X = r.value.sum(1).reshape(S, w * h).mean(0)
    g = law["on_g"] & ~law["excluded"] & (law["var"] > 0)
    assert g.sum() > 300
    z = (X[g] - law["mu"][g]) / np.sqrt(law["var"][g] / S)
    Z = z.sum() / np.sqrt(g.sum())
    print(kind, mode, sampling, dict(maxz=float(np.abs(z).max()), Z=float(Z), rel=float(X[g].mean() / law["mu"][g].mean() - 1)))
    assert np.abs(z).max() < 5.5 and abs(Z) < 5.0
    if sampling == (0, 0, 0.0):   # and the closed form a E F + a L (1 - F), no quadrature involved
        hits = orc.OracleScene(sc.desc()).closest_hit(o[g], d[g])
        p = hits["position"].astype(np.float64)
        want = ll.exact_mean(p, np.tile([0.0, 1.0, 0.0], (len(p), 1)), light, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY)
        z2 = (X[g] - want) / np.sqrt(law["var"][g] / S)
        assert np.abs(z2).max() < 5.5 and abs(z2.sum() / np.sqrt(g.sum())) < 5.0
    sky = ~law["on_g"]
    lim = sampling[2] if sampling[2] > 0 else np.inf
    assert np.allclose(X[sky], np.minimum(np.asarray(cf.SKY, np.float32), lim).astype(np.float64).sum(), rtol=1e-6)


# ---- the replay tells wrong estimators apart --------------------------------------------------------------------------------
# wrong estimator -> (case, mode) on which it must show; chosen for what the case contains, not from the result
SEPARATES = {
    "wb_no_pmf": ("DEFAULT", "mis"),                      # three lights: pmf < 1 in every weight
    "balance": ("RANDOM_BALLS_SMALL", "mis"),
    "pb_kept": ("specular", "mis"),                       # ground -> glass / metal -> light
    "thr_after_rr": ("DEFAULT_rr_clamp_jitter", "nee"),
    "clamp_sum": ("DEFAULT_rr_clamp_jitter", "mis"),
    "tmax_no_eps": ("penumbra", "nee"),                   # the quad light then blocks its own samples
    "last_light_never": ("LIGHT_TEST", "mis"),
    "wb_camera": ("resting", "mis"),                      # the light is in view
    "d2_tlight": ("specular", "mis"),                     # a large quad light: d2 of the hit differs from the sample's
}


@pytest.mark.parametrize("wrong", lr.WRONG)
def test_wrong_estimators_are_told_apart(cases, wrong):
    name, mode = SEPARATES[wrong]
    c = cases[name]
    right = lr.replay_case(c, mode, osc=c["osc"])
    other = lr.replay_case(c, mode, wrong=wrong, stability=False, osc=c["osc"])
    share = lr.separated_share(right, other, 10.0)
    print(wrong, name, mode, share)
    assert share > 0.01, (wrong, name, mode, share)


def test_tolerance_is_the_stated_one():
    """One light term of size t at cosines of order 1 carries (1e-5 + c) t + 1e-6 with c = 8 * 2^-24 / min cos, plus the fp32
    additions; at the grazing cut c is 5e-4."""
    assert abs(8 * lr.U / lr.COS_MIN - 4.77e-4) < 1e-5
    c = lr.case("penumbra", 64, 48)
    r = lr.replay_case(c, "nee", samples=(0,))
    one = r.stable & (np.abs(r.value).max(1) > 0.1)
    rel = (r.tol[one] / np.maximum(np.abs(r.value[one]), 1e-30)).max(1)
    assert np.median(rel) < 3e-5 and rel.max() < 2e-3
