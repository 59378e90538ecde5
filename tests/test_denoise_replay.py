"""CPU-side tests of the film denoiser's contract (include/prt.h "The filter contract") through its numpy restatement
(tests/denoise_replay.py): what the filter is worth on oracle frames, that a feature edge is exact, and that nothing is
filtered when nothing is asked for.

Quality fixture: (5, 5, 8) camera toward the origin, 44 x 28 film, depth 5, seed 3; the noisy frame is the oracle's samples
0..7 (moments from the eight one-sample frames, as the film statistics add them), the features are the oracle's linear-scan
closest hit of the pixel-centre rays, the target is the mean of the 1024 samples 8..1031.  Gate: with the default settings
the denoised MSE is below half the noisy MSE on CORNELL, LIGHT_TEST and DEFAULT.  This build measures the ratios
0.089 (CORNELL), 0.042 (LIGHT_TEST) and 0.177 (DEFAULT).  MATERIAL_TEST is the stated counter-example (nearly noise-free at
8 samples, and its mirrors and glass show what the first-hit features cannot see): its ratio, 1.106, is reported, not gated."""
import functools

import numpy as np
import pytest

import adaptive_replay as ar
import denoise_replay as dr
import util
from util import prt

F = np.float32
FX = dict(cam_pos=(5.0, 5.0, 8.0), W=44, H=28, depth=5, seed=3, spp=8, target_spp=1024)


@functools.lru_cache(maxsize=None)
def quality(preset):
    scene = prt.Scene(preset)
    osc = util.oracle_scene(scene)
    W, H = FX["W"], FX["H"]
    cam = prt.Camera(position=FX["cam_pos"], width=W, height=H).desc()
    kw = dict(max_depth=FX["depth"], seed=FX["seed"], iterative=True, n_threads=8)
    frames = [osc.render(cam, W, H, spp=1, first_sample=s, **kw)[0] for s in range(FX["spp"])]
    accum = np.zeros((H, W, 3), F)
    for f in frames:
        accum += f
    A, Q = ar.moments(frames)
    weights = np.full((H, W), F(FX["spp"]))
    mean, var = dr.film_inputs(accum, weights, A, Q)
    feat = dr.oracle_features(osc, scene, cam, W, H)
    target = osc.render(cam, W, H, spp=FX["target_spp"], first_sample=FX["spp"], **kw)[0].astype(np.float64) / FX["target_spp"]
    info = {}
    # (guard off: the MSE needs no bit-exactness, and DEFAULT's spheres take max(0, N.N)^64 through the subnormal range)
    out, _ = dr.denoise(mean, var, feat["albedo"], feat["normal"], feat["position"], feat["prim"], info=info, guard=False)
    mse = lambda a: float(np.mean((a.astype(np.float64) - target) ** 2))  # noqa: E731
    return dict(noisy=mse(mean), denoised=mse(out), info=info, out=out)


@pytest.mark.parametrize("preset", ["CORNELL", "LIGHT_TEST", "DEFAULT"])
def test_denoised_mse_is_below_half_the_noisy_mse(preset):
    r = quality(preset)
    ratio = r["denoised"] / r["noisy"]
    print(f"{preset}: noisy MSE {r['noisy']:.4e}, denoised {r['denoised']:.4e}, ratio {ratio:.3f}, smallest intermediate {r['info']['smallest']:.2e}")
    assert np.isfinite(r["out"]).all()
    assert r["denoised"] < 0.5 * r["noisy"], ratio


def test_material_test_is_the_reported_counter_example():
    r = quality("MATERIAL_TEST")
    print(f"MATERIAL_TEST: noisy MSE {r['noisy']:.4e}, denoised {r['denoised']:.4e}, ratio {r['denoised'] / r['noisy']:.3f}")
    assert np.isfinite(r["out"]).all()   # reported only: mirrors, glass and next to no noise (DESIGN.md section 3 "Denoising")


# ---- synthetic fixtures ------------------------------------------------------------------------------------------------
def two_regions(kind, W=37, H=23, seed=5):
    """Left region: a plane facing +z.  Right region (x >= 17, plus a single-pixel island inside the left one): a plane
    facing +x (perpendicular normals) or a miss."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    right = xs >= 17
    right[9, 5] = True
    N = np.zeros((H, W, 3), F)
    N[..., 2] = 1
    P = np.stack([xs * 0.1, ys * 0.1, np.zeros_like(xs)], axis=-1).astype(F)
    prim = np.zeros((H, W), np.int32)
    alb = rng.uniform(0.2, 0.9, (H, W, 3)).astype(F)
    if kind == "perpendicular":
        N[right] = (1, 0, 0)
        P[right] = np.stack([np.full(right.sum(), 1.7), ys[right] * 0.1, xs[right] * 0.1], axis=-1).astype(F)
        prim[right] = 1
    else:
        N[right] = 0
        P[right] = 0
        prim[right] = -1
    mean = rng.uniform(0.0, 2.0, (H, W, 3)).astype(F)
    var = (rng.uniform(0.0, 0.05, (H, W)) * (rng.random((H, W)) < 0.8)).astype(F)
    return dict(mean=mean, var=var, albedo=alb, normal=N, position=P, prim=prim), right


@pytest.mark.parametrize("kind", ["perpendicular", "miss"])
@pytest.mark.parametrize("demodulate", [0, 1])
def test_a_feature_edge_is_exact(kind, demodulate):
    """Changing the colours of one region leaves the other region's output bit-identical.  The contract's variance
    prefilter is not edge-aware: a region sees its neighbour only through the neighbour's variance images, which do not
    depend on the neighbour's colours in the first iteration (any variances) and never when the variances are zero (they
    stay zero).  Both cases are held here, the second over all the iterations of the defaults and of the maximum; with
    non-zero variances and two or more iterations the colours of one region reach the other's guide, by the contract."""
    a, right = two_regions(kind)
    rng = np.random.default_rng(9)
    b = dict(a)
    b["mean"] = a["mean"].copy()
    b["mean"][right] = rng.uniform(0.0, 50.0, (int(right.sum()), 3)).astype(F)
    cases = [(dict(iterations=1), a["var"]), (dict(iterations=5), np.zeros_like(a["var"])), (dict(iterations=6, normal_power_log2=0), np.zeros_like(a["var"]))]
    for cfg, var in cases:
        oa, va = dr.denoise(**dict(a, var=var), demodulate=demodulate, **cfg)
        ob, vb = dr.denoise(**dict(b, var=var), demodulate=demodulate, **cfg)
        left = ~right
        assert np.array_equal(oa[left].view(np.uint32), ob[left].view(np.uint32)), (kind, cfg)
        assert np.array_equal(va[left].view(np.uint32), vb[left].view(np.uint32)), (kind, cfg)
        assert not np.array_equal(oa[right], ob[right])
        # ... and the other way round: the right region does not see the left one's colours
        c = dict(a, var=var)
        c["mean"] = a["mean"].copy()
        c["mean"][left] = rng.uniform(0.0, 50.0, (int(left.sum()), 3)).astype(F)
        oc, _ = dr.denoise(**c, demodulate=demodulate, **cfg)
        assert np.array_equal(oa[right].view(np.uint32), oc[right].view(np.uint32)), (kind, cfg)
    # the island is alone in its region within reach of the first iteration: it keeps its own colour, (h c) / h
    o1, _ = dr.denoise(**a, demodulate=0, iterations=1)
    h = F(9.0 / 64.0)
    assert np.array_equal(o1[9, 5], ((h * a["mean"][9, 5]).astype(F) / h).astype(F))


def test_no_iterations_and_no_demodulation_return_the_input():
    a, _ = two_regions("miss")
    out, vout = dr.denoise(**a, iterations=0, demodulate=0)
    assert np.array_equal(out.view(np.uint32), a["mean"].view(np.uint32)) and np.array_equal(vout.view(np.uint32), a["var"].view(np.uint32))


def test_a_flat_image_stays_flat_and_its_variance_falls():
    H, W = 12, 70
    flat = dict(mean=np.full((H, W, 3), F(0.5)), var=np.full((H, W), F(0.01)), albedo=np.full((H, W, 3), F(0.5)),
                normal=np.tile(np.array([0, 1, 0], F), (H, W, 1)), position=np.zeros((H, W, 3), F), prim=np.zeros((H, W), np.int32))
    ys, xs = np.mgrid[0:H, 0:W]
    flat["position"][..., 0], flat["position"][..., 2] = xs, ys
    out, vout = dr.denoise(**flat)
    assert np.allclose(out, 0.5, rtol=1e-6) and (vout < 0.01 * 0.05).all() and (vout > 0).all()


def test_the_guard_refuses_a_fixture_with_subnormal_intermediates():
    a, _ = two_regions("miss")
    a["var"] = np.full_like(a["var"], F(2.0 ** -125))
    with pytest.raises(AssertionError):
        dr.denoise(**a)
    info = {}
    dr.denoise(**a, guard=False, info=info)
    assert info["below_guard"] > 0


def test_film_inputs_follow_the_exported_rule():
    rng = np.random.default_rng(3)
    n = rng.choice([0, 1, 2, 3, 8, 64], 500).astype(F)
    y = rng.uniform(0.0, 3.0, 500)
    A = (n * y).astype(F)
    Q = (n * (y * y + rng.uniform(0, 1, 500) * (rng.random(500) < 0.7))).astype(F)
    Q[::7] = (A[::7].astype(np.float64) ** 2 / np.maximum(n[::7], 1) * 0.9999).astype(F)   # Q / n below m^2
    acc = rng.uniform(0, 5, (500, 3)).astype(F)
    mean, var = dr.film_inputs(acc, n, A, Q)
    lib = prt.capi.lib()
    got = np.array([lib.prt_denoise_variance(float(a), float(b), float(c)) for a, b, c in zip(n, A, Q)], F)
    assert np.array_equal(got.view(np.uint32), var.view(np.uint32))
    assert (var[n == 0] == 0).all() and (mean[n == 0] == 0).all() and (var >= 0).all()
    one = n == 1
    assert np.array_equal(var[one], (A[one] * A[one]).astype(F))
