"""The float64 laws of light-sampled pixels (tests/lighting_laws.py) checked on the CPU: the quadrature's mean against the
closed forms, its moments against a plain float64 Monte Carlo of the same estimator, and its frame statistics against
deliberately wrong estimators (double counting, a missing |n_l.w|, a missing 1/pmf, a light sample at the last
segment), which they must reject while passing the right one."""
import numpy as np
import pytest

import closed_form as cf
import lighting_laws as ll


def _lights():
    _, _, emitter = _ground()
    return {"D": ("quad", emitter[0], emitter[1], emitter[2]), "E": ("sphere", (0.0, 4.0, 0.0), 1.0)}


def _ground():
    from util import prt  # (Scene and its transforms only: no device)
    return cf.ground_scene(prt)


def _points(m, seed=3):
    rng = np.random.default_rng(seed)
    p = np.column_stack([rng.uniform(-8, 8, m), np.full(m, -1.0), rng.uniform(-8, 8, m)])
    return p, np.tile([0.0, 1.0, 0.0], (m, 1))


@pytest.mark.parametrize("kind", ["D", "E"])
@pytest.mark.parametrize("mode", ["mis", "nee"])
def test_quadrature_mean_is_the_closed_form(kind, mode):
    light = _lights()[kind]
    p, n = _points(500)
    want = ll.exact_mean(p, n, light, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY)
    for rr in (0, 1):
        mu, var, m4, spread = ll.ground_moments(p, n, light, mode, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY, rr=rr)
        np.testing.assert_allclose(mu, want, rtol=1e-9)
        assert np.all(var > 0) and np.all(m4 > 0) and np.all(spread > 0)


@pytest.mark.parametrize("kind", ["D", "E"])
@pytest.mark.parametrize("mode,rr,clamp", [("mis", 0, 0.0), ("nee", 0, 0.0), ("mis", 1, 0.0), ("nee", 1, 1.0), ("mis", 0, 1.0)])
def test_moments_match_a_float64_monte_carlo(kind, mode, rr, clamp):
    light = _lights()[kind]
    p, n = _points(200, seed=7)
    mu, var, m4, _ = ll.ground_moments(p, n, light, mode, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY, rr=rr, clamp=clamp)
    S = 20000
    x = ll.mc_samples(np.random.default_rng(11), p, n, light, mode, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY, S, rr=rr, clamp=clamp)
    z = (x.mean(1) - mu) / np.sqrt(var / S)
    assert np.abs(z).max() < 5.5, np.abs(z).max()
    assert abs(z.sum() / np.sqrt(len(z))) < 5.0
    # sample variance against the law's: its standard error is sqrt((m4 - var^2) / S)
    zv = (x.var(1) - var) / np.sqrt(np.maximum(m4 - var ** 2, 1e-300) / S)
    assert np.abs(zv).max() < 6.0 and abs(zv.sum() / np.sqrt(len(zv))) < 5.0


def _synthetic_frame(light, mode, wrong=None, pmf=1.0, max_depth=5, S=64, W=48, H=32, seed=5):
    p, n = _points(W * H, seed=seed)
    x = ll.mc_samples(np.random.default_rng(seed + 1), p, n, light, mode, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY, S,
                      pmf=pmf, max_depth=max_depth, wrong=wrong)
    acc = np.zeros((W * H, 3), np.float32)
    acc[:, 0] = x.sum(1)            # (frame_stats reads the channel sum)
    mu, var, m4, spread = ll.ground_moments(p, n, light, mode, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY, pmf=pmf,
                                            max_depth=max_depth)
    exact = np.full((W * H, 3), np.nan, np.float32)
    zero = var == 0
    exact[zero] = 0.0
    law = dict(mu=mu, var=var, m4=m4, spread=spread, exact=exact, excluded=np.zeros(W * H, bool))
    return ll.frame_stats(acc, np.full(W * H, S, np.float32), S, law, W, H)


@pytest.mark.parametrize("kind", ["D", "E"])
@pytest.mark.parametrize("mode", ["mis", "nee"])
def test_statistics_pass_the_estimator_and_reject_wrong_ones(kind, mode):
    light = _lights()[kind]
    r = _synthetic_frame(light, mode)
    assert ll.passes(r), r
    r = _synthetic_frame(light, mode, pmf=0.5)
    assert ll.passes(r), r
    bad = [dict(wrong="double"), dict(wrong="no_pmf", pmf=0.5), dict(wrong="last", max_depth=1)]
    if kind == "D":
        bad.append(dict(wrong="no_cos_l"))
    for kw in bad:
        r = _synthetic_frame(light, mode, **kw)
        assert not ll.passes(r), (kw, r)


def test_last_segment_law_is_a_point():
    light = _lights()["D"]
    p, n = _points(50)
    mu, var, m4, spread = ll.ground_moments(p, n, light, "mis", cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY, max_depth=1)
    assert np.all(mu == 0) and np.all(var == 0)
