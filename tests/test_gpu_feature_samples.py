"""Sampled guide features on the GPU (include/prt.h "Sampled guide features").  The sampled set is compared bit for bit
with the numpy restatement of the sums and the finish (tests/feature_samples_replay.py) fed with per-sample records that come
from the function-level entry points alone: the render's keys and jitter draws (tests/lens_replay.py), the context's
prt_camera_rays_lens for the rays, and the guide rule (tests/guide_features_replay.py) over the context's prt_closest_hit and
prt_hit_uv.  The rays are shown to be the render's own by counting emitter hits against the film; the degenerate case, the
chunking, the invalidation list, the consumers and the off state are each held to equality."""
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_replay as dr
import feature_samples_replay as fsr
import guide_features_replay as gr
import lens_replay as lr
import temporal_replay as tr
import util
from test_gpu_guide_features import (BUNNY_CAM, CAM, DEPTH, SEED, _assert_set, _diff, _equal_sets, _film_state, _mesh_scene, _renderer,
                                     _same, _textured_albedo)
from util import prt

pytestmark = pytest.mark.gpu

U32 = np.uint32
F = np.float32
LENS = dict(aperture=0.2, focus_distance=6.0)
FIRST = ("albedo", "normal", "position", "depth", "prim")


def _read_sampled(r):
    return prt.capi.lib().prt_features_read_sampled(r._ctx, None, None, None, None, None, None)


def _first(feat):
    return {k: feat[k] for k in FIRST}


def _assert_sampled(got, want, what):
    assert np.array_equal(got["hits"], want["hits"]), (what, "hits", int((got["hits"] != want["hits"]).sum()))
    _assert_set(got, want, what)


def _equal_sampled(a, b):
    return _equal_sets(a, b) and np.array_equal(a["hits"], b["hits"])


def _replay(r, scene, w, h, K, seed, first_sample, jitter, max_specular):
    """The sampled set from per-sample records made by the function-level entry points."""
    n = w * h
    px, py, keys = fsr.sample_keys_and_points(w, h, K, seed, first_sample, jitter)
    o, d, _ = r.camera_rays_lens(px, py, keys)
    g = gr.guide_features(r.closest_hit, scene, o, d, K * n, 1, max_specular=max_specular, roughness_max=0.1,
                          albedo_of=_textured_albedo(r, scene) if scene.material_texture else None)
    recs = [{k: g[k].reshape((K * n,) + g[k].shape[2:])[s * n:(s + 1) * n] for k in FIRST} for s in range(K)]
    return fsr.reshape(fsr.reduce_samples(recs), w, h)


@functools.lru_cache(maxsize=None)
def _room():
    return gr.mirror_room(pane=True)


# ---- 1. bit for bit against the restatement ------------------------------------------------------------------------------
# 37 x 29: 1073 pixels, neither a multiple of 64 nor of 256, several blocks; 70 x 5 and 1 x 1: less than a block, one pixel;
# 130 x 67: 8710 pixels x 8 samples, some tens of thousands of live chains per round.  K = 64: the cap; first_sample != 0.
CASES = [(37, 29, K, ms, j) for K in (1, 3, 8, 64) for ms in (0, 4) for j in (0, 1)] + [(70, 5, 8, 4, 1), (1, 1, 3, 4, 1), (130, 67, 8, 4, 1),
                                                                                              (130, 67, 3, 0, 0)]


@pytest.mark.parametrize("w,h,K,max_specular,jitter", CASES)
def test_sampled_set_equals_the_restatement_bit_for_bit(w, h, K, max_specular, jitter):
    scene = _room()
    r, _ = _renderer(scene, w, h, trace=(max_specular, 0.1), lens=LENS)
    r.set_sampling(jitter=jitter)
    first_sample = 0 if K == 64 else 5
    r.set_feature_sampling(K, first_sample=first_sample)
    got = r.render_features()
    s = got["sampled"]
    want = _replay(r, scene, w, h, K, SEED, first_sample, jitter, max_specular)
    partial = int(((want["hits"] > 0) & (want["hits"] < K)).sum())
    print(f"{w}x{h}, K {K}, max_specular {max_specular}, jitter {jitter}: {partial} pixels with 0 < hits < K")
    _assert_sampled(s, want, (w, h, K, max_specular, jitter))
    if K > 1 and (w, h) != (1, 1):
        assert partial >= 1                                                     # otherwise the case shows nothing
    assert (max_specular > 0) == ("guide" in got)
    again = r.render_features()["sampled"]
    assert _equal_sampled(again, s)


def test_mesh_scene_with_textures_and_a_partition():
    w, h, K = 44, 28, 8
    scene, _, _ = _mesh_scene()
    lens = dict(fov_y=0.8, aperture=0.05, focus_distance=3.5)
    sets = {}
    for ms in (0, 4):
        r, _ = _renderer(scene, w, h, BUNNY_CAM, trace=(ms, 0.1), lens=lens)
        r.set_sampling(jitter=1)
        r.set_feature_sampling(K)
        s = r.render_features()["sampled"]
        want = _replay(r, scene, w, h, K, SEED, 0, 1, ms)
        _assert_sampled(s, want, ("bunny", ms))
        assert ((want["hits"] > 0) & (want["hits"] < K)).any()
        assert len(np.unique(want["albedo"].reshape(-1, 3), axis=0)) > 50       # textured, and mixed
        sets[ms] = s
        rp, _ = _renderer(scene, w, h, BUNNY_CAM, rank=1, world=3, trace=(ms, 0.1), lens=lens)   # rank 1 of 3: the whole image
        rp.set_sampling(jitter=1)
        rp.set_feature_sampling(K)
        assert _equal_sampled(rp.render_features()["sampled"], s), ms
        assert _read_sampled(r) == 0
        r.UpdateInstances(scene)                                                # the placed copies' transforms given again: dropped
        assert _read_sampled(r) == 1
        assert _equal_sampled(r.render_features()["sampled"], s), ms
    assert not _same(sets[0]["albedo"], sets[4]["albedo"])                      # the mirrors are followed


# ---- 2. chunking -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_specular", [0, 4])
def test_the_chunk_size_changes_nothing(max_specular):
    w, h, K = 37, 29, 8
    r, _ = _renderer(_room(), w, h, trace=(max_specular, 0.1), lens=LENS)
    r.set_sampling(jitter=1)
    r.set_feature_sampling(K)
    want = r.render_features()["sampled"]
    for chunk in (1, 3, 8, 64, 0):                                              # 3: chunks of 3, 3 and 2 samples
        r.set_param("feature_chunk", chunk)
        r.set_feature_sampling(K)                                               # (drops the sets)
        assert _read_sampled(r) == 1
        assert _equal_sampled(r.render_features()["sampled"], want), chunk
    with pytest.raises(prt.PrtError):
        r.set_param("feature_chunk", 65)


# ---- 3. the rays are the render's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [0, 1])
def test_hits_equal_the_film_of_the_same_samples(jitter):
    """Sky 0 and one triangle of emission 1: at depth 1 the film's red sum of a pixel is the number of its samples whose
    primary ray hit the triangle, a small integer that is exact in fp32, and so is hits."""
    K = 16
    scene, cam = lr.edge_scene()
    w, h = int(cam.width), int(cam.height)
    for first_sample in (0, 5):
        film = prt.Film(w, h)
        r = prt.HipWavefrontRenderer(device=0, max_depth=1, seed=SEED)
        r.Init(film, scene, cam)
        r.set_lens(*lr.edge_lens())
        r.set_sampling(jitter=jitter)
        r.frame_index = first_sample
        r.ProgressiveRender(K)
        r.download()
        red = film.accum[..., 0].copy()
        assert np.array_equal(film.weights, np.full((h, w), F(K)))
        r.set_feature_sampling(K, first_sample=first_sample)
        hits = r.render_features()["sampled"]["hits"]
        assert np.array_equal(red, hits.astype(F)), (first_sample, int((red != hits).sum()))
        assert ((hits > 0) & (hits < K)).sum() > 100                            # the defocused edge
        for wrong in (dict(seed=SEED + 1, first_sample=first_sample), dict(first_sample=first_sample + 1)):   # the check has teeth
            r.set_feature_sampling(K, **wrong)
            assert not np.array_equal(red, r.render_features()["sampled"]["hits"].astype(F)), wrong


# ---- 4. the degenerate case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_specular", [0, 8])
def test_without_jitter_and_aperture_it_is_the_centre_ray_set(max_specular):
    w, h = 37, 29
    r, _ = _renderer(_room(), w, h, trace=(max_specular, 0.1), lens=dict(fov_y=0.9))
    r.set_feature_sampling(16)
    feat = r.render_features()
    centre = feat["guide"] if max_specular else _first(feat)
    s = feat["sampled"]
    assert _equal_sets({k: s[k] for k in FIRST}, {k: centre[k] for k in FIRST})
    assert np.array_equal(s["hits"], (centre["prim"] >= 0).astype(U32)) and s["hits"].min() == 0 and s["hits"].max() == 1
    st0 = r.stats()
    r.set_feature_sampling(64)
    r.render_features()
    assert r.stats().rays_total == st0.rays_total                               # (the feature pass counts no render rays)


# ---- 5. off changes nothing --------------------------------------------------------------------------------------------------------
def _everything(r, film):
    feat = r.render_features()
    r.ProgressiveRender(2)
    dn = r.denoise()
    state = _film_state(r, film)
    st = r.stats()
    return feat, dn, state, (st.rays_total, list(st.rays_per_depth), st.samples)


def test_off_changes_nothing_and_on_leaves_the_other_sets_alone():
    scene = _room()
    w, h = 44, 28
    mk = lambda: _renderer(scene, w, h, stats=True, trace=(8, 0.1), lens=LENS)    # noqa: E731
    r0, film0 = mk()
    r0.set_sampling(jitter=1)
    feat0, dn0, state0, counts0 = _everything(r0, film0)                           # never touched
    assert "sampled" not in feat0 and _read_sampled(r0) == 1

    r1, film1 = mk()
    r1.set_sampling(jitter=1)
    r1.set_feature_sampling(8)
    r1.render_features()
    r1.set_feature_sampling(0)                                                     # on and off again
    feat1, dn1, state1, counts1 = _everything(r1, film1)
    assert "sampled" not in feat1 and _read_sampled(r1) == 1
    assert b"sampled" in prt.capi.lib().prt_last_error(r1._ctx)
    assert _equal_sets(_first(feat1), _first(feat0)) and _equal_sets(feat1["guide"], feat0["guide"])
    assert _same(dn1, dn0) and all(_same(a, b) for a, b in zip(state1, state0)) and counts1 == counts0

    r2, film2 = mk()
    r2.set_sampling(jitter=1)
    r2.set_feature_sampling(8)                                                     # on: only the filter's choice changes
    feat2, dn2, state2, counts2 = _everything(r2, film2)
    assert "sampled" in feat2
    assert _equal_sets(_first(feat2), _first(feat0)) and _equal_sets(feat2["guide"], feat0["guide"])
    assert all(_same(a, b) for a, b in zip(state2, state0)) and counts2 == counts0 and counts0[0] > 0
    assert not _same(dn2, dn0)
    g = {k: np.zeros_like(v) for k, v in feat0["guide"].items()}                   # the readers of the other sets: as ever
    fp, ip, up = (prt.capi.C.POINTER(t) for t in (prt.capi.C.c_float, prt.capi.C.c_int32, prt.capi.C.c_uint32))
    assert prt.capi.lib().prt_features_read_guide(r2._ctx, g["albedo"].ctypes.data_as(fp), g["normal"].ctypes.data_as(fp),
                                                  g["position"].ctypes.data_as(fp), g["depth"].ctypes.data_as(fp), g["prim"].ctypes.data_as(ip),
                                                  g["bounces"].ctypes.data_as(up)) == 0
    assert _equal_sets(g, feat0["guide"])


# ---- 6. invalidation -------------------------------------------------------------------------------------------------------------
def test_stale_sampled_features_are_refused():
    L = prt.capi.lib()
    scene = _room()
    w, h = 37, 29
    r, _ = _renderer(scene, w, h, trace=(2, 0.1), lens=LENS)
    r.set_feature_sampling(4)
    assert _read_sampled(r) == 1                                                 # none yet
    r.render_features()
    assert _read_sampled(r) == 0
    for change in (lambda: r.SetCamera(prt.Camera(position=(4.0, 5.0, 8.0), width=w, height=h)), lambda: r.set_lens(fov_y=0.7, **LENS),
                   lambda: r.set_textures(None), lambda: L.prt_set_film(r._ctx, w, h, 0, 1),
                   lambda: r.Init(prt.Film(w, h), scene, prt.Camera(position=CAM, width=w, height=h)), lambda: r.set_feature_trace(3, 0.1),
                   lambda: r.set_feature_sampling(4), lambda: r.set_feature_sampling(5, seed=9, first_sample=2),
                   lambda: r.set_sampling(jitter=1), lambda: r.set_sampling(jitter=0)):
        change()
        assert _read_sampled(r) == 1 and b"feature" in L.prt_last_error(r._ctx)
        assert L.prt_features_read(r._ctx, None, None, None, None, None) == 1
        assert L.prt_features_read_guide(r._ctx, None, None, None, None, None, None) == 1
        r.render_features()
        assert _read_sampled(r) == 0
    r.set_sampling(jitter=0, rr_depth=3)                                         # jitter unchanged: nothing is dropped
    assert _read_sampled(r) == 0
    assert L.prt_set_feature_sampling(r._ctx, prt.capi.C.byref(prt.capi.PrtFeatureSampling(65, 0, 0))) == 1    # a refusal drops the sets too
    assert _read_sampled(r) == 1 and r.get_feature_sampling().samples == 5
    assert L.prt_features_read(r._ctx, None, None, None, None, None) == 1
    # while off, prt_set_sampling drops nothing
    r.set_feature_sampling(0)
    r.render_features()
    for j in (1, 0):
        r.set_sampling(jitter=j)
        assert L.prt_features_read(r._ctx, None, None, None, None, None) == 0
        assert L.prt_features_read_guide(r._ctx, None, None, None, None, None, None) == 0
    assert _read_sampled(r) == 1


# ---- 7. the filter takes it ----------------------------------------------------------------------------------------------------
SPP = 8


def test_film_denoise_is_guided_by_the_sampled_set():
    w, h = 44, 28
    r, film = _renderer(_room(), w, h, stats=True, trace=(8, 0.1), lens=LENS)
    r.set_sampling(jitter=1)
    r.set_feature_sampling(SPP)
    r.ProgressiveRender(SPP)
    state = _film_state(r, film)
    got, got_var = r.denoise(return_variance=True)
    assert all(_same(a, b) for a, b in zip(state, _film_state(r, film)))
    feat = r.render_features()
    s, g = feat["sampled"], feat["guide"]
    mean, var = dr.film_inputs(*state)
    want, want_var = r.denoise_arrays(mean, var, s["albedo"], s["normal"], s["position"], s["prim"], return_variance=True)
    assert _same(got, want), _diff(got, want)
    assert _same(got_var, want_var), _diff(got_var, want_var)
    centre = r.denoise_arrays(mean, var, g["albedo"], g["normal"], g["position"], g["prim"])
    assert not _same(got, centre) and np.isfinite(got).all()
    r.set_feature_sampling(0)
    assert _same(r.denoise(), centre)


def test_a_group_of_two_ranks_on_one_device_equals_the_single_context():
    w, h = 44, 28
    scene = _room()
    r, _ = _renderer(scene, w, h, stats=True, trace=(8, 0.1), lens=LENS)
    r.set_sampling(jitter=1)
    r.set_feature_sampling(SPP)
    r.ProgressiveRender(SPP)
    want = r.denoise()
    g = prt.HipWavefrontGroupRenderer([0, 0], max_depth=DEPTH, seed=SEED)
    g.Init(prt.Film(w, h), scene, prt.Camera(position=CAM, width=w, height=h))
    g.set_film_statistics(True)
    g.set_lens(**LENS)
    g.set_sampling(jitter=1)
    g.set_feature_trace(8, 0.1)
    g.ProgressiveRender(SPP)
    off = g.denoise()
    g.set_feature_sampling(SPP)
    got = g.denoise()
    assert _same(got, want), _diff(got, want)
    assert not _same(off, got)
    assert _equal_sampled(g.render_features()["sampled"], r.render_features()["sampled"])
    fs = prt.capi.PrtFeatureSampling()
    for rank in range(2):
        assert prt.capi.lib().prt_get_feature_sampling(prt.capi.lib().prt_group_context(g._grp, rank), prt.capi.C.byref(fs)) == 0
        assert (fs.samples, fs.seed, fs.first_sample) == (SPP, SEED, 0)
    assert g.get_feature_sampling().samples == SPP
    with pytest.raises(prt.PrtError):
        g.set_feature_sampling(65)


def test_temporal_step_filters_by_the_sampled_set():
    w, h = 44, 28
    r, film = _renderer(_room(), w, h, stats=True, trace=(8, 0.1), lens=LENS)
    r.set_sampling(jitter=1)
    r.set_feature_sampling(SPP)
    r.ProgressiveRender(SPP)
    state = _film_state(r, film)
    feat = r.render_features()
    K = r.camera_basis()
    got, got_var = r.temporal_step(return_variance=True, denoise={})
    c, n = tr.frame_inputs(*state)
    blend = r.temporal_arrays(K, c, n, state[2], state[3], feat["prim"], feat["position"], feat["normal"], history=None)
    s = feat["sampled"]
    want, want_var = r.denoise_arrays(blend["c"], blend["var"], s["albedo"], s["normal"], s["position"], s["prim"], return_variance=True)
    assert _same(got, want), _diff(got, want)
    assert _same(got_var, want_var), _diff(got_var, want_var)
    g = feat["guide"]
    assert not _same(got, r.denoise_arrays(blend["c"], blend["var"], g["albedo"], g["normal"], g["position"], g["prim"]))


# ---- 8. it helps where it should --------------------------------------------------------------------------------------------------
DEFOCUS = dict(W=64, H=48, spp=16, K=16, ref_spp=4096, cam=(0.0, 2.5, 6.0), aperture=0.5, seed=SEED)
# MSE(sampled) / MSE(centre) on the defocused pixels, measured once on an MI355X (the test prints every figure), and the gate:
# the measured ratio plus a quarter of its distance to 1.
DEFOCUS_RATIO_MEASURED = 0.0548
DEFOCUS_RATIO_BOUND = DEFOCUS_RATIO_MEASURED + 0.25 * (1.0 - DEFOCUS_RATIO_MEASURED)   # 0.291


def defocus_scene():
    """A checker-textured ground (2-unit checks), a Lambertian ball on it, an emissive quad above."""
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.5, 0.5, 0.5))
    light = sc.AddEmissive((6.0, 6.0, 6.0))
    ball = sc.AddLambertian((0.7, 0.3, 0.2))
    sc.AddQuad(60.0, 60.0, ground)
    sc.AddQuad(10.0, 10.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 9.0, -2.0))
    sc.AddCircle(1.0, ball, translation=(0.0, 1.0, 0.0))
    sc.SetMaterialTexture(ground, sc.AddTexture(prt.scenes.checker(30, (0.9, 0.9, 0.9), (0.1, 0.1, 0.1)), "nearest", "repeat"))
    return sc


def defocus_figures():
    """MSE against the 4096-spp film of the same renderer (the render path, not the code under test) of the film denoised by
    the sampled set and by the centre-ray set, on the defocused and on the in-focus pixels."""
    fx = DEFOCUS
    w, h, K = fx["W"], fx["H"], fx["K"]
    scene = defocus_scene()
    focus = float(np.linalg.norm(np.array(fx["cam"]) - np.array((0.0, 1.0, 0.0)))) - 1.0       # the ball's near pole
    film = prt.Film(w, h)
    r = prt.HipWavefrontRenderer(device=0, max_depth=DEPTH, seed=fx["seed"])
    r.Init(film, scene, prt.Camera(position=fx["cam"], width=w, height=h))
    r.set_lens(aperture=fx["aperture"], focus_distance=focus)
    r.set_sampling(jitter=1)
    r.set_lighting("mis")
    r.set_film_statistics(True)
    r.ProgressiveRender(fx["spp"])
    centre = r.denoise()
    r.set_feature_sampling(K)
    sampled = r.denoise()
    s = r.render_features()["sampled"]
    # circle of confusion (diameter, pixels) from the sampled depth: the depth along the optical axis is the ray length times
    # the cosine between the centre ray and the axis; a point at axial distance z is spread over 2 R |1 / f - 1 / z| at unit
    # distance, and a pixel is 2 tan(fov_y / 2) / H there.
    basis = r.camera_basis()
    ys, xs = np.mgrid[0:h, 0:w]
    _, d = r.camera_rays(xs.ravel().astype(F) + F(0.5), ys.ravel().astype(F) + F(0.5))
    cosine = (d.astype(np.float64) @ np.asarray(basis["front"], np.float64)).reshape(h, w)
    z = s["depth"].astype(np.float64) * cosine
    pixel = 2.0 * float(basis["tan_fov_y"]) / h
    with np.errstate(all="ignore"):
        coc = np.where(s["hits"] > 0, 2.0 * fx["aperture"] * np.abs(1.0 / focus - 1.0 / z) / pixel, 0.0)
    defocused = ((s["hits"] > 0) & (s["hits"] < K)) | (coc > 2.0)
    film.Clear()
    r.frame_index = fx["spp"]
    r.ProgressiveRender(fx["ref_spp"])
    r.download()
    ref = film.accum.astype(np.float64) / film.weights.astype(np.float64)[..., None]
    mse = lambda a, sel: float(np.mean((a.astype(np.float64)[sel] - ref[sel]) ** 2))    # noqa: E731
    out = dict(pixels=(int(defocused.sum()), int((~defocused).sum())), coc_max=float(coc.max()),
               defocused=(mse(sampled, defocused), mse(centre, defocused)), in_focus=(mse(sampled, ~defocused), mse(centre, ~defocused)))
    print("defocus fixture:", out)
    return out


def test_the_sampled_set_helps_where_the_image_is_defocused():
    """Gates: (a) on the defocused pixels MSE(sampled) < MSE(centre), and <= DEFOCUS_RATIO_BOUND (0.291) x MSE(centre);
    (b) on the in-focus pixels MSE(sampled) <= 1.1 x MSE(centre).  Measured on an MI355X, against the 4096-spp film: 1828
    defocused pixels (circle of confusion up to 7.5 pixels) 0.00902 against 0.16447, a ratio of 0.0548; 1244 in-focus pixels
    0.00558 against 0.02518, a ratio of 0.222 (a circle of up to two pixels and the jitter still mix the ground's checks)."""
    f = defocus_figures()
    assert min(f["pixels"]) > 200 and f["coc_max"] > 4.0, f
    (sd, cd), (si, ci) = f["defocused"], f["in_focus"]
    assert sd < cd, f
    assert sd <= DEFOCUS_RATIO_BOUND * cd, f
    assert si <= 1.1 * ci, f


# ---- 9. the command line -------------------------------------------------------------------------------------------------------
def test_prt_render_feature_samples_writes_what_the_python_call_returns(tmp_path):
    w, h, K = 44, 28, 4
    exe = os.path.join(util.ROOT, "parallelraytracing_amd", "csrc", "prt_render")
    out = str(tmp_path / "frame")
    p = subprocess.run([exe, "--preset", "MATERIAL_TEST", "--width", str(w), "--height", str(h), "--depth", str(DEPTH), "--seed", str(SEED),
                        "--camera", "5", "5", "8", "--spp", str(SPP), "--aperture", "0.2", "--focus", "9", "--denoise",
                        "--feature-samples", str(K), "--features-out", out, "--out", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    r, film = _renderer(prt.Scene("MATERIAL_TEST"), w, h, stats=True, lens=dict(aperture=0.2, focus_distance=9.0))
    r.set_feature_sampling(K)
    r.ProgressiveRender(SPP)
    want = r.denoise()
    assert _same(prt.read_pfm(out + "_denoised.pfm"), want)
    feat = r.render_features()
    s = feat["sampled"]
    assert ((s["hits"] > 0) & (s["hits"] < K)).sum() > 5
    for k in ("albedo", "normal", "position"):
        assert _same(prt.read_pfm(f"{out}_{k}.pfm"), feat[k]), k
        assert _same(prt.read_pfm(f"{out}_sampled_{k}.pfm"), s[k]), k
    assert _same(prt.read_pfm(out + "_sampled_depth.pfm")[..., 0], s["depth"])
    assert np.array_equal(prt.read_pfm(out + "_sampled_hits.pfm")[..., 0], s["hits"].astype(F))
    r.set_feature_sampling(0)
    assert not _same(r.denoise(), want)
    bad = subprocess.run([exe, "--preset", "MATERIAL_TEST", "--width", "8", "--height", "8", "--feature-samples", "4", "--out", out],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--feature-samples" in bad.stderr
