"""CPU tests that make the float64 replay of environment-lit frames (tests/environment_replay.py) credible before any kernel
is held to it:

  * with a constant map equal to `sky` and lighting OFF its delivered terms equal OracleScene.render bit for bit;
  * the contract is unbiased: on a ground quad under the sun map (one texel at 1e4) the means of the OFF, NEE and MIS
    replays agree pixel group by pixel group within 4 standard errors of their difference, the standard errors estimated
    from the replays' own samples.  Seeds are fixed; the pixels are a 20 x 15 grid in 4 groups of 75 (by image quadrant), 96
    samples each: 7,200 paths per group.  The sun subtends 1 / 158 of the upper hemisphere's cosine-weighted measure, so a
    group's OFF estimate sees it about 45 times: enough for its own variance estimate to be meaningful, and far too few for
    OFF to have a small error, which is the point of the feature;
  * every listed wrong estimator is told apart from the right one by the comparison the GPU tests use (a stable pixel sample
    moves by more than 10x its tolerance): no T_e factor on the other lights, sin(theta) of the texel centre, a finite tmax
    and w_B left at 1 on replays of whole frames; a second lookup for Le differs from the contract only where fp32 rounding
    carries a sampled direction across a texel edge, so it is shown on light-stream keys whose u1 is 0 (the direction lies on
    the column's left edge)."""
import numpy as np
import pytest

import environment_replay as er
import lighting_replay as lr
from util import orc, prt


@pytest.mark.parametrize("scene", ["DEFAULT", "bunny_env"])
def test_constant_map_with_lighting_off_is_the_oracle_bit_for_bit(scene):
    c = er.case("DEFAULT_sun" if scene == "DEFAULT" else scene)
    sc = c["scene"]
    sky = np.asarray(sc.sky, np.float32)
    env = er.EnvMap(np.broadcast_to(sky, (8, 16, 3)).copy())
    osc = orc.OracleScene(sc.desc())
    samples = (0, 5)
    rep = er.replay(sc, env, c["cam"], c["W"], c["H"], c["depth"], lr.SEED, samples, "off", use_bvh=c["use_bvh"], osc=osc)
    total = 0
    for s in samples:
        a, w, rays = osc.render(c["cam"].desc(), c["W"], c["H"], spp=1, first_sample=s, max_depth=c["depth"], seed=lr.SEED,
                                iterative=True, use_bvh=c["use_bvh"], n_threads=lr.n_threads_default())
        total += rays
        assert np.array_equal(a.reshape(-1, 3).view(np.uint32), rep.delivered[rep.samp == s].view(np.uint32))
    assert rep.segments == total and rep.n_misses > 1000
    assert np.array_equal(rep.value.astype(np.float32).view(np.uint32), rep.delivered.view(np.uint32))
    assert rep.shadow_rays == 0


def test_off_nee_and_mis_agree_within_their_standard_errors():
    c = er.case("ground")
    env = er.case_env(c)
    assert env.t_env(0) == er.TWO32
    W, H = c["W"], c["H"]
    ys, xs = np.meshgrid(np.arange(4, H, 8), np.arange(4, W, 8), indexing="ij")
    pix = (ys * W + xs).ravel()
    group = ((ys >= H // 2) * 2 + (xs >= W // 2)).ravel()
    n_s = 96
    osc = orc.OracleScene(c["scene"].desc())
    means, sems = {}, {}
    for mode in ("off", "nee", "mis"):
        rep = er.replay_case(c, mode, samples=range(n_s), osc=osc, pix=pix, stability=False, env=env)
        lum = rep.value.mean(1).reshape(n_s, len(pix))
        means[mode] = np.array([lum[:, group == g].mean() for g in range(4)])
        sems[mode] = np.array([lum[:, group == g].std(ddof=1) / np.sqrt(lum[:, group == g].size) for g in range(4)])
        if mode != "off":
            assert rep.n_env_samples > 0.5 * len(rep.pix) and rep.shadow_rays > 0
    print({k: (np.round(means[k], 4).tolist(), np.round(sems[k], 4).tolist()) for k in means}, flush=True)
    assert np.all(means["mis"] > 1.0)      # the sun lights the ground
    for a, b in (("off", "nee"), ("off", "mis"), ("nee", "mis")):
        z = np.abs(means[a] - means[b]) / np.sqrt(sems[a] ** 2 + sems[b] ** 2)
        assert np.all(z <= 4.0), (a, b, z)
    # and the estimators are not the same numbers: light sampling has far less variance than scattering alone
    assert np.all(sems["mis"] < 0.5 * sems["off"])


# (w_B left at 1 under NEE: there every miss after a Lambertian vertex has weight 0, so the mistake shows on all of them; under
# the power heuristic it shows only where pL is comparable to pB, next to the sun's texel)
@pytest.mark.parametrize("wrong,mode", [("no_te_factor", "mis"), ("sin_centre", "mis"), ("finite_tmax", "mis"), ("wb_one", "nee")])
def test_wrong_estimators_are_told_apart_on_frames(wrong, mode):
    c = er.case("DEFAULT_sun")
    osc = orc.OracleScene(c["scene"].desc())
    right = er.replay_case(c, mode, samples=(0,), osc=osc)
    other = er.replay_case(c, mode, samples=(0,), osc=osc, wrong=wrong, stability=False)
    share = lr.separated_share(right, other)
    print(wrong, share, flush=True)
    assert share > 0.01, (wrong, share)


def test_a_second_lookup_for_le_is_told_apart_at_texel_edges():
    env = er.EnvMap(er.named_map("sun"), 1.0)
    te = env.t_env(0)
    # keys whose light stream has u1 = 0: the third state's top 24 bits vanish (about one key in 2^24; the first twelve, found
    # by a search over the keys from 0 upwards and checked here)
    keys = np.array([33370035, 35104194, 45196569, 97423633, 120891493, 130773660, 142724731, 148257635, 166583770, 199390034,
                     207681634, 213668975], np.uint32)
    s = lr.pcg((keys.astype(np.uint64) + lr.LIGHT_RNG) & lr.M32)
    assert np.all((lr.pcg(lr.pcg(lr.pcg(s))) >> 8) == 0)
    n = np.tile(np.array([[0.0, 1.0, 0.0]]), (len(keys), 1))
    right = er.env_terms(env, te, n, keys, "mis")
    other = er.env_terms(env, te, n, keys, "mis", wrong="second_lookup")
    up = right["valid"] & (right["cos_n"] > 0)
    t_r = right["le"] * right["f"][:, None]
    t_o = other["le"] * other["f"][:, None]
    tol = (1e-5 + 8.0 * lr.U / np.maximum(np.minimum(right["cos_n"], right["cos_l"]), 1e-6))[:, None] * np.abs(t_r) + lr.ABS_TOL
    apart = up & (np.abs(t_o - t_r) > 10.0 * tol).any(1)
    print(dict(keys=len(keys), upward=int(up.sum()), apart=int(apart.sum())), flush=True)
    assert apart.sum() >= 1
    # away from the edges the two are the same estimator
    rk = np.random.default_rng(2).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    nn = np.tile(np.array([[0.0, 1.0, 0.0]]), (len(rk), 1))
    a, b = er.env_terms(env, te, nn, rk, "mis"), er.env_terms(env, te, nn, rk, "mis", wrong="second_lookup")
    assert np.array_equal(a["le"], b["le"])
