"""First-hit feature images and the film denoiser on the GPU (include/prt.h "First-hit feature images and the edge-avoiding
film denoiser").  Every comparison is bit for bit: prt_denoise against the numpy restatement (tests/denoise_replay.py) on
synthetic arrays at the sizes where the kernel takes another path, the feature images against the oracle's linear-scan closest
hit of the same centre rays, and prt_film_denoise against the restatement fed with the film, the moments and the features the
context itself reports.  Rendered frames are 44 x 28 (partial tiles on two edges), 8 samples, depth 5, seed 3."""
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_replay as dr
import texture_replay as tr
import util
from util import prt

pytestmark = pytest.mark.gpu

U32 = np.uint32
F = np.float32
W, H, DEPTH, SEED, SPP = 44, 28, 5, 3, 8
CAM = (5.0, 5.0, 8.0)
BUNNY_CAM = (2.0, 1.5, 3.0)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(U32), np.ascontiguousarray(b, F).view(U32))


def _diff(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    bad = a.view(U32) != b.view(U32)
    return f"{int(bad.sum())} of {bad.size} values differ, max |a - b| = {float(np.max(np.abs(a - b))):.3e}"


@functools.lru_cache(maxsize=None)
def _device():
    return prt.HipWavefrontRenderer(device=0)


# ---- 1. prt_denoise against the restatement on synthetic arrays ---------------------------------------------------------
# 37 x 29: narrower than a wave, and the step-16 taps leave the image on both sides; 70 x 5: a partial second wave and fewer
# rows than a tap column (and than a block); 1 x 1; 130 x 67 with 6 iterations: several blocks both ways, step 32.
SYNTHETIC = [
    ("37x29 defaults", 37, 29, False, {}),
    ("37x29 no demodulation", 37, 29, False, dict(demodulate=0)),
    ("37x29 normal power 0", 37, 29, False, dict(normal_power_log2=0)),
    ("37x29 normal power 8", 37, 29, False, dict(normal_power_log2=8)),
    ("37x29 sigmas", 37, 29, False, dict(sigma_l=0.5, sigma_z=1.0)),
    ("37x29 1 iteration", 37, 29, False, dict(iterations=1)),
    ("37x29 2 iterations", 37, 29, False, dict(iterations=2)),
    ("37x29 3 iterations", 37, 29, False, dict(iterations=3)),
    ("37x29 4 iterations", 37, 29, False, dict(iterations=4)),
    ("37x29 sphere", 37, 29, True, {}),
    ("37x29 sphere, normal power 8", 37, 29, True, dict(normal_power_log2=8)),
    ("70x5 defaults", 70, 5, False, {}),
    ("70x5 6 iterations", 70, 5, False, dict(iterations=6)),
    ("70x5 sphere", 70, 5, True, {}),
    ("1x1 defaults", 1, 1, False, {}),
    ("1x1 nothing to do", 1, 1, False, dict(iterations=0, demodulate=0)),
    ("130x67 sphere, 6 iterations", 130, 67, True, dict(iterations=6)),
    ("130x67 sphere, 6 iterations, power 8, no demodulation", 130, 67, True, dict(iterations=6, normal_power_log2=8, demodulate=0)),
    ("130x67 planes, 6 iterations", 130, 67, False, dict(iterations=6)),
]


@pytest.mark.parametrize("name,w,h,cap,cfg", SYNTHETIC, ids=[s[0] for s in SYNTHETIC])
def test_denoise_equals_the_restatement_bit_for_bit(name, w, h, cap, cfg):
    a = dr.synthetic(w, h, seed=w + h, cap=cap)
    want, want_var = dr.denoise(**a, **cfg)          # (guard on: a fixture holds no intermediate below 2^-120)
    got, got_var = _device().denoise_arrays(**a, return_variance=True, **cfg)
    assert _same(got, want), _diff(got, want)
    assert _same(got_var, want_var), _diff(got_var, want_var)
    assert np.isfinite(got).all()
    if w > 1:
        assert (a["var"] == 0).any() and (a["prim"] < 0).any() and (a["prim"] >= 0).any()
    if cfg.get("iterations", 5) == 0 and not cfg.get("demodulate", 1):
        assert _same(got, a["mean"]) and _same(got_var, a["var"])
    again = _device().denoise_arrays(**a, **cfg)     # var_out = NULL: the same colours
    assert _same(again, got)
    for lds in (0, 2):                               # no iteration / steps 1 and 2 staged in LDS (default: step 1): the same bits
        _device().set_param("denoise_lds", lds)
        try:
            ab, ab_var = _device().denoise_arrays(**a, return_variance=True, **cfg)
        finally:
            _device().set_param("denoise_lds", 1)
        assert _same(ab, got) and _same(ab_var, got_var), (lds, _diff(ab, got))


def test_non_finite_inputs_never_fault():
    a = dr.synthetic(70, 9, seed=4)
    a["mean"][3, 20] = np.nan
    a["var"][5, 40] = np.inf
    a["position"][1, 60] = np.inf
    a["normal"][7, 5] = np.nan
    out = _device().denoise_arrays(**a, iterations=1)
    ys, xs = np.mgrid[0:9, 0:70]
    reach = np.zeros((9, 70), bool)
    for (y, x) in ((3, 20), (5, 40), (1, 60), (7, 5)):
        reach |= (np.abs(ys - y) <= 3) & (np.abs(xs - x) <= 3)   # taps at step 1 and the 3 x 3 prefilter of their den
    clean = dict(a)
    want, _ = dr.denoise(**{k: np.nan_to_num(v, nan=0.5, posinf=0.5) if v.dtype == F else v for k, v in clean.items()}, iterations=1, guard=False)
    assert _same(out[~reach], want[~reach]) and np.isfinite(out[~reach]).all()


# ---- 2. device arrays ----------------------------------------------------------------------------------------------------
def test_denoise_device_on_torch_tensors_equals_the_host_entry():
    import torch
    r = _device()
    a = dr.synthetic(70, 29, seed=8, cap=True)
    host, host_var = r.denoise_arrays(**a, return_variance=True)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in a.items()}
    got, got_var = r.denoise_arrays(**t, return_variance=True)
    assert got.device == dev and got.dtype == torch.float32 and tuple(got.shape) == (29, 70, 3)
    assert _same(got.cpu().numpy(), host) and _same(got_var.cpu().numpy(), host_var)
    only = r.denoise_arrays(**t, iterations=2, demodulate=0)
    assert _same(only.cpu().numpy(), r.denoise_arrays(**a, iterations=2, demodulate=0))
    with pytest.raises(ValueError):
        r.denoise_arrays(**dict(t, prim=t["prim"].float()))
    with pytest.raises(ValueError):
        r.denoise_arrays(**dict(t, var=t["var"][:5]))


# ---- 3. features ---------------------------------------------------------------------------------------------------------
def _renderer(scene, cam_pos=CAM, w=W, h=H, rank=0, world=1, stats=True, setup=None, depth=DEPTH):
    film = prt.Film(w, h)
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=SEED, rank=rank, world_size=world)
    r.Init(film, scene, prt.Camera(position=cam_pos, width=w, height=h))
    if setup:
        setup(r)
    if stats:
        r.set_film_statistics(True)
    return r, film


@functools.lru_cache(maxsize=None)
def _bunny_scene():
    """A bunny (a world-space mesh) on the ground under a light, with a textured placed copy of cube_uv beside it."""
    sc = prt.scenes.mesh_scene(prt.Mesh(prt.scenes.asset("bunny.ply")))
    body = sc.AddLambertian((0.7, 0.6, 0.5))
    sc.AddInstance(prt.Mesh(prt.scenes.asset("cube_uv.ply")), body, scale=0.5, euler_deg=(0.0, 30.0, 0.0), translation=(1.1, -0.5, 0.4))
    sc.SetMaterialTexture(body, sc.AddTexture(tr._random_image(5, 3, 1), "bilinear", "repeat"))
    sc.SetMaterialTexture(0, sc.AddTexture(prt.scenes.checker(4, (0.9, 0.85, 0.8), (0.15, 0.2, 0.1)), "nearest", "repeat"))
    return sc


SCENES = {
    "CORNELL": (lambda: prt.Scene("CORNELL"), CAM),
    "RANDOM_BALLS_SMALL": (lambda: prt.Scene("RANDOM_BALLS_SMALL"), CAM),
    "bunny": (_bunny_scene, BUNNY_CAM),
}


def _centre_rays(r, w=W, h=H):
    ys, xs = np.mgrid[0:h, 0:w]
    return r.camera_rays(xs.ravel().astype(F) + F(0.5), ys.ravel().astype(F) + F(0.5))


def _expected_features(r, scene, w=W, h=H):
    """The oracle's linear-scan closest hit of the context's own centre rays; albedo from the material table, and for a
    textured material from prt_texture_eval at the UV prt_hit_uv reports."""
    o, d = _centre_rays(r, w, h)
    hits = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
    tex_alb = None
    if scene.material_texture:
        _, uv, _ = r.hit_uv(o, d)
        mats = np.where(hits["prim"] >= 0, hits["material_id"], 0)
        tex_alb = np.array([[m.rgb[0], m.rgb[1], m.rgb[2]] for m in scene.materials], F)[mats]
        for m, t in scene.material_texture.items():
            sel = (hits["prim"] >= 0) & (hits["material_id"] == m)
            if sel.any():
                tex_alb[sel] = r.texture_eval(t, uv[sel])
    return dr.features_from_hits(hits, scene, w, h, textured_albedo=tex_alb), hits


def _assert_features(got, want, what):
    assert np.array_equal(got["prim"], want["prim"]), what
    for k in ("normal", "position", "depth", "albedo"):
        assert _same(got[k], want[k]), (what, k, _diff(got[k], want[k]))


FEATURE_CASES = [("plain", {}, None), ("fov", dict(fov_y=0.6), None), ("aperture", dict(fov_y=0.6, aperture=0.2, focus_distance=6.0), "fov"),
                 ("rank1of3", {}, None)]


@pytest.mark.parametrize("scene_name", sorted(SCENES))
def test_features_equal_the_oracles_closest_hit_of_the_centre_rays(scene_name):
    make, cam = SCENES[scene_name]
    scene = make()
    seen = {}
    for case, lens, same_as in FEATURE_CASES:
        rank, world = (1, 3) if case == "rank1of3" else (0, 1)
        r, _ = _renderer(scene, cam, rank=rank, world=world, stats=False, setup=(lambda r: r.set_lens(**lens)) if lens else None)
        got = r.render_features()
        want, hits = _expected_features(r, scene)
        _assert_features(got, want, (scene_name, case))
        assert got["prim"].shape == (H, W) and (got["prim"] >= 0).any()
        miss = got["prim"] < 0
        assert (got["albedo"][miss] == 1).all() and not got["normal"][miss].any() and not got["depth"][miss].any()
        seen[case] = got
        if same_as:   # an aperture leaves the features alone
            assert all(_same(got[k], seen[same_as][k]) for k in ("albedo", "normal", "position", "depth")) and np.array_equal(got["prim"], seen[same_as]["prim"])
    assert all(_same(seen["rank1of3"][k], seen["plain"][k]) for k in ("albedo", "normal", "position", "depth"))   # the whole image
    assert not _same(seen["fov"]["position"], seen["plain"]["position"])
    if scene_name == "CORNELL":
        mt = np.array([m.type for m in scene.materials])
        hit = seen["plain"]["prim"] >= 0
        assert (seen["plain"]["albedo"][hit] != 1).any() and set(np.unique(mt)) >= {1, 4}   # diffuse walls and the light
    if scene_name == "bunny":
        assert len(np.unique(seen["plain"]["albedo"].reshape(-1, 3), axis=0)) > 20                # textured albedo


def test_stale_features_are_refused():
    L = prt.capi.lib()
    scene = prt.Scene("CORNELL")
    r, _ = _renderer(scene, stats=False)
    read = lambda: L.prt_features_read(r._ctx, None, None, None, None, None)  # noqa: E731
    assert read() == 1                                         # none yet
    r.render_features()
    assert read() == 0
    r.SetCamera(prt.Camera(position=(4.0, 5.0, 8.0), width=W, height=H))
    assert read() == 1 and b"feature" in L.prt_last_error(r._ctx)
    r.render_features()
    for change in (lambda: r.set_lens(fov_y=0.7), lambda: r.set_textures(None),
                   lambda: L.prt_set_film(r._ctx, W, H, 0, 1), lambda: r.Init(prt.Film(W, H), scene, prt.Camera(position=CAM, width=W, height=H))):
        change()
        assert read() == 1
        r.render_features()
        assert read() == 0


# ---- 4. prt_film_denoise end to end ---------------------------------------------------------------------------------------
ROUTES = {
    "compact": None,
    "jitter": lambda r: r.set_sampling(jitter=1),
    "mis": lambda r: r.set_lighting("mis"),
}


def _film_state(r, film):
    r.download()
    A, Q = r.film_statistics()
    return film.accum.copy(), film.weights.copy(), A, Q


def _check_film_denoise(r, film, what, **cfg):
    before = _film_state(r, film)
    got, got_var = r.denoise(return_variance=True, **cfg)
    after = _film_state(r, film)
    assert all(_same(a, b) for a, b in zip(before, after)), what           # film and moments: not a bit
    feat = r.render_features()
    mean, var = dr.film_inputs(*before)
    info = {}
    want, want_var = dr.denoise(mean, var, feat["albedo"], feat["normal"], feat["position"], feat["prim"], guard=False, info=info, **cfg)
    print(f"{what}: {info}")
    assert _same(got, want), (what, _diff(got, want), info)
    assert _same(got_var, want_var), (what, _diff(got_var, want_var), info)
    return got


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("scene_name", ["CORNELL", "bunny"])
def test_film_denoise_equals_the_restatement(scene_name, route):
    make, cam = SCENES[scene_name]
    r, film = _renderer(make(), cam, setup=ROUTES[route])
    r.ProgressiveRender(SPP)
    out = _check_film_denoise(r, film, (scene_name, route))
    r.download()
    assert np.isfinite(out).all() and not _same(out, film.mean())
    if route == "compact":
        _check_film_denoise(r, film, (scene_name, route, "settings"), iterations=3, sigma_l=2.0, sigma_z=0.5, normal_power_log2=3, demodulate=0)


def test_film_denoise_after_adaptive_sampling_and_on_an_empty_film():
    r, film = _renderer(prt.Scene("CORNELL"))
    _check_film_denoise(r, film, "empty film")                              # every pixel of weight 0: mean 0, variance 0
    info = r.render_adaptive(0.10, min_spp=2, step_spp=4, max_spp=14)
    r.download()
    assert len(np.unique(film.weights)) > 1 and info.passes >= 1            # unequal n
    _check_film_denoise(r, film, "adaptive")
    film.Clear()
    r.frame_index = 0
    r.ProgressiveRender(1)                                                   # n = 1 everywhere: var = fl(m)^2
    _check_film_denoise(r, film, "one sample")


# ---- 5. group and command line --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", ["CORNELL", "bunny"])
def test_a_group_of_three_ranks_on_one_device_equals_the_single_context(scene_name):
    make, cam = SCENES[scene_name]
    scene = make()
    r, film = _renderer(scene, cam)
    r.ProgressiveRender(SPP)
    want, want_var = r.denoise(return_variance=True)
    g = prt.HipWavefrontGroupRenderer([0, 0, 0], max_depth=DEPTH, seed=SEED)
    g.Init(prt.Film(W, H), scene, prt.Camera(position=cam, width=W, height=H))
    g.set_film_statistics(True)
    with pytest.raises(prt.PrtError):
        prt.capi.lib().prt_group_set_film_statistics(g._grp, 0)
        g.denoise()                                                          # statistics off: refused
    g.set_film_statistics(True)
    g.ProgressiveRender(SPP)
    got, got_var = g.denoise(return_variance=True)
    assert _same(got, want), _diff(got, want)
    assert _same(got_var, want_var)
    gf, sf = g.render_features(), r.render_features()
    assert all(_same(gf[k], sf[k]) for k in ("albedo", "normal", "position", "depth")) and np.array_equal(gf["prim"], sf["prim"])
    assert _same(g.denoise(iterations=2, demodulate=0), r.denoise(iterations=2, demodulate=0))


def test_prt_render_denoise_writes_what_the_python_call_returns(tmp_path):
    exe = os.path.join(util.ROOT, "parallelraytracing_amd", "csrc", "prt_render")
    out = str(tmp_path / "frame")
    p = subprocess.run([exe, "--preset", "CORNELL", "--width", str(W), "--height", str(H), "--depth", str(DEPTH), "--seed", str(SEED),
                        "--camera", "5", "5", "8", "--spp", str(SPP), "--denoise", "--denoise-iterations", "4", "--denoise-sigma-l", "3",
                        "--denoise-sigma-z", "0.2", "--features-out", out, "--out", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    r, film = _renderer(prt.Scene("CORNELL"))
    r.ProgressiveRender(SPP)
    want = r.denoise(iterations=4, sigma_l=3.0, sigma_z=0.2)
    assert _same(prt.read_pfm(out + "_denoised.pfm"), want)
    r.download()
    assert _same(prt.read_pfm(out + ".pfm"), film.mean())                    # the noisy frame beside it
    assert os.path.getsize(out + "_denoised.ppm") > W * H * 3
    feat = r.render_features()
    for k in ("albedo", "normal", "position"):
        assert _same(prt.read_pfm(f"{out}_{k}.pfm"), feat[k]), k
    assert _same(prt.read_pfm(out + "_depth.pfm")[..., 0], feat["depth"])


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_statistics_off_and_a_partitioned_context_are_refused():
    scene = prt.Scene("CORNELL")
    r, _ = _renderer(scene, stats=False)
    r.ProgressiveRender(2)
    with pytest.raises(prt.PrtError, match="statistics"):
        r.denoise()
    r.render_features()                                                      # features need no statistics
    rp, _ = _renderer(scene, rank=1, world=3)
    rp.ProgressiveRender(2)
    with pytest.raises(prt.PrtError, match="prt_group_film_denoise"):
        rp.denoise()
    with pytest.raises(prt.PrtError, match="iterations"):
        _renderer(scene)[0].denoise(iterations=7)
