"""CPU-side tests of the sampled guide features (include/prt.h "Sampled guide features"): the host-only behaviour of
prt_set_feature_sampling, and the numpy restatement of the sums and the finish (tests/feature_samples_replay.py) on hand-made
per-sample records."""
import ctypes as C

import numpy as np
import pytest

import feature_samples_replay as fsr
from util import prt

F = np.float32


def _get(r):
    fs = r.get_feature_sampling()
    return fs.samples, fs.seed, fs.first_sample


def _read(r):
    return prt.capi.lib().prt_features_read_sampled(r._ctx, None, None, None, None, None, None)


def test_feature_sampling_on_a_host_only_context():
    L = prt.capi.lib()
    assert C.sizeof(prt.capi.PrtFeatureSampling) == 12
    r = prt.HipWavefrontRenderer(device=-1, seed=11)
    d = prt.capi.PrtFeatureSampling(7, 7, 7)
    L.prt_feature_sampling_defaults(C.byref(d))
    assert (d.samples, d.seed, d.first_sample) == (0, 0, 0)
    assert _get(r) == (0, 0, 0)
    r.set_feature_sampling(16)                                               # seed=None: the renderer's own
    assert _get(r) == (16, 11, 0)
    r.set_feature_sampling(64, seed=5, first_sample=9)
    assert _get(r) == (64, 5, 9)
    for bad in (65, 1000, 0xFFFFFFFF):
        assert L.prt_set_feature_sampling(r._ctx, C.byref(prt.capi.PrtFeatureSampling(bad, 1, 2))) == 1, bad
        assert b"feature sampling" in L.prt_last_error(r._ctx)
        with pytest.raises(prt.PrtError):
            r.set_feature_sampling(bad)
        assert _get(r) == (64, 5, 9), bad                                    # the previous setting, intact
    # kept across scene, film and camera
    r.set_scene_host_only(prt.Scene("CORNELL"))
    assert L.prt_set_film(r._ctx, 16, 8, 0, 1) == 0
    r.SetCamera(prt.Camera((3.0, 2.0, 1.0), width=16, height=8))
    assert _get(r) == (64, 5, 9)
    # nothing has been rendered (and nothing can be, here): every set is refused, after the setter and after a refusal
    for call in (lambda: r.set_feature_sampling(4), lambda: L.prt_set_feature_sampling(r._ctx, C.byref(prt.capi.PrtFeatureSampling(65, 0, 0)))):
        call()
        assert _read(r) == 1 and b"feature" in L.prt_last_error(r._ctx)
        assert L.prt_features_read(r._ctx, None, None, None, None, None) == 1
        assert L.prt_features_read_guide(r._ctx, None, None, None, None, None, None) == 1
    assert L.prt_render_features(r._ctx) != 0
    assert L.prt_set_feature_sampling(r._ctx, None) == 0 and _get(r) == (0, 0, 0)   # NULL: the defaults
    assert L.prt_set_sampling(r._ctx, C.byref(prt.capi.PrtSampling(1, 0, 0.0))) == 0   # (jitter while off: as ever)
    assert L.prt_get_feature_sampling(r._ctx, None) == 1 and L.prt_get_feature_sampling(None, C.byref(d)) == 1


def _rec(albedo, normal, position, depth, prim):
    return dict(albedo=np.array([albedo], F), normal=np.array([normal], F), position=np.array([position], F), depth=np.array([depth], F),
                prim=np.array([prim], np.int32))


MISS = _rec((0.9, 0.5, 1.0), (0, 0, 0), (0, 0, 0), 0.0, -1)


def test_all_misses():
    s = fsr.reduce_samples([MISS] * 3)
    third = F(1) / F(3)
    want = [((F(0.9) + F(0.9)) + F(0.9)) * third, ((F(0.5) + F(0.5)) + F(0.5)) * third, F(3) * third]
    assert s["albedo"][0].tolist() == [F(v) for v in want]
    assert not s["normal"].any() and not s["position"].any() and s["depth"][0] == 0
    assert s["prim"][0] == -1 and s["hits"][0] == 0


def test_one_hit_of_four():
    hit = _rec((0.2, 0.4, 0.6), (0.0, 0.6, 0.8), (1.0, 2.0, 3.0), 5.0, 7)
    s = fsr.reduce_samples([MISS, MISS, hit, MISS])
    assert s["hits"][0] == 1 and s["prim"][0] == 7
    assert s["position"][0].tolist() == [1.0, 2.0, 3.0] and s["depth"][0] == 5.0          # the mean over the HITS, not over K
    q = F(1) / F(4)
    assert s["albedo"][0, 0] == (((F(0.9) + F(0.9)) + F(0.2)) + F(0.9)) * q                # the mean over all K
    n = np.array([0.0, 0.6, 0.8], F)
    l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    assert np.array_equal(s["normal"][0], n * (F(1) / np.sqrt(l2)))


def test_prim_is_that_of_the_first_sample_that_hit():
    a = _rec((0.2, 0.2, 0.2), (0, 1, 0), (0, 0, 0), 1.0, 3)
    b = _rec((0.2, 0.2, 0.2), (0, 1, 0), (2, 2, 2), 3.0, 9)
    s = fsr.reduce_samples([MISS, b, a])
    assert s["prim"][0] == 9 and s["hits"][0] == 2
    assert s["position"][0].tolist() == [1.0, 1.0, 1.0] and s["depth"][0] == 2.0


def test_opposite_normals_give_a_zero_normal_and_keep_the_hit():
    up = _rec((0.5, 0.5, 0.5), (0.0, 1.0, 0.0), (0, 1, 0), 2.0, 4)
    down = _rec((0.5, 0.5, 0.5), (0.0, -1.0, 0.0), (0, 3, 0), 4.0, 5)
    s = fsr.reduce_samples([up, down])
    assert not s["normal"].any() and np.isfinite(s["normal"]).all()
    assert s["prim"][0] == 4 and s["hits"][0] == 2 and s["depth"][0] == 3.0 and s["position"][0].tolist() == [0.0, 2.0, 0.0]


def test_one_sample_is_the_record_itself_except_for_the_renormalised_normal():
    rng = np.random.default_rng(5)
    n = 200
    nr = rng.normal(size=(n, 3)).astype(F)
    nr = (nr * (F(1) / np.sqrt(((nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]).astype(F)))[:, None]).astype(F)
    prim = rng.integers(-1, 50, n).astype(np.int32)
    hit = prim >= 0
    rec = dict(albedo=rng.random((n, 3)).astype(F), normal=np.where(hit[:, None], nr, 0).astype(F),
               position=np.where(hit[:, None], rng.normal(size=(n, 3)) * 10, 0).astype(F), depth=np.where(hit, rng.random(n) * 9, 0).astype(F), prim=prim)
    s = fsr.reduce_samples([rec])
    for k in ("albedo", "position", "depth", "prim"):
        assert np.array_equal(s[k], rec[k]), k
    assert np.array_equal(s["hits"], hit.astype(np.uint32)) and (~hit).any() and hit.any()
    assert np.abs(s["normal"] - rec["normal"]).max() <= 2.0 ** -23                          # one more rounding, no more
    assert not s["normal"][~hit].any()
