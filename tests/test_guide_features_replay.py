"""CPU-side tests of the guide features through specular chains (include/prt.h "Guide features through specular chains")
through their numpy restatement (tests/guide_features_replay.py): what following mirrors and glass is worth to the film
denoiser on oracle frames, that max_specular = 0 is the first-hit set, that MIRROR_ROOM holds every case of the chain, and the
host-only behaviour of prt_set_feature_trace.

Quality fixture: test_denoise_replay.py's ((5, 5, 8) camera, 44 x 28, depth 5, seed 3, 8 one-sample oracle frames, target =
samples 8..1031, denoise_replay.denoise(guard=False)) on MIRROR_ROOM, max_specular 8, roughness_max 0.1.  The yardstick is the
first-hit features of the same fixture.  Chain pixels: replay bounces > 0.  Gates and what this build measures:
  (a) chain pixels  MSE(followed) <= 0.5 x MSE(first-hit)   measured 0.249 (382 of 1232 pixels)
  (b) other pixels  MSE(followed) <= 1.1 x MSE(first-hit)   measured 1.034
  (c) whole frame   followed ratio < first-hit ratio         measured 0.0759 < 0.1381 (denoised / noisy MSE)
DEFAULT (54 chain pixels: chain 0.649, other 0.992, whole frame 0.1770 -> 0.1643) and MATERIAL_TEST (54 chain pixels: chain
0.587, other 1.011, whole frame 1.1055 -> 0.9950, nearly noise-free either way) are printed, not gated."""
import ctypes as C
import functools

import numpy as np
import pytest

import adaptive_replay as ar
import denoise_replay as dr
import guide_features_replay as gr
import util
from util import prt

F = np.float32
U32 = np.uint32
FX = dict(cam_pos=(5.0, 5.0, 8.0), W=44, H=28, depth=5, seed=3, spp=8, target_spp=1024)


def _scene(name):
    if name.startswith("MIRROR_ROOM"):
        return gr.mirror_room(pane=name.endswith("+pane"))
    return prt.Scene(name)


@functools.lru_cache(maxsize=None)
def replay(name, max_specular, W=FX["W"], H=FX["H"]):
    scene = _scene(name)
    osc = util.oracle_scene(scene)
    cam = prt.Camera(position=FX["cam_pos"], width=W, height=H).desc()
    o, d = gr.centre_rays(cam, W, H)
    trace = {}
    g = gr.guide_features(gr.linear_scan(osc), scene, o, d, W, H, max_specular=max_specular, roughness_max=0.1, trace=trace)
    return g, trace, scene, osc, cam


@functools.lru_cache(maxsize=None)
def quality(name):
    guide, _, scene, osc, cam = replay(name, 8)
    W, H = FX["W"], FX["H"]
    kw = dict(max_depth=FX["depth"], seed=FX["seed"], iterative=True, n_threads=8)
    frames = [osc.render(cam, W, H, spp=1, first_sample=s, **kw)[0] for s in range(FX["spp"])]
    accum = np.zeros((H, W, 3), F)
    for f in frames:
        accum += f
    A, Q = ar.moments(frames)
    mean, var = dr.film_inputs(accum, np.full((H, W), F(FX["spp"])), A, Q)
    first = dr.oracle_features(osc, scene, cam, W, H)
    target = osc.render(cam, W, H, spp=FX["target_spp"], first_sample=FX["spp"], **kw)[0].astype(np.float64) / FX["target_spp"]
    outs = {k: dr.denoise(mean, var, f["albedo"], f["normal"], f["position"], f["prim"], guard=False)[0] for k, f in (("first", first), ("guide", guide))}
    chain = guide["bounces"] > 0
    mse = lambda a, sel: float(np.mean((a.astype(np.float64)[sel] - target[sel]) ** 2))  # noqa: E731
    everything = np.ones((H, W), bool)
    r = dict(chain_pixels=int(chain.sum()), noisy=mse(mean, everything), outs=outs)
    for k in ("first", "guide"):
        r[k] = dict(frame=mse(outs[k], everything), chain=mse(outs[k], chain) if chain.any() else 0.0, other=mse(outs[k], ~chain))
    return r


def _report(name):
    r = quality(name)
    print(f"{name}: {r['chain_pixels']} chain pixels of {FX['W'] * FX['H']}; denoised / noisy MSE, first-hit -> followed: whole frame "
          f"{r['first']['frame'] / r['noisy']:.4f} -> {r['guide']['frame'] / r['noisy']:.4f}; followed / first-hit MSE: chain pixels "
          f"{r['guide']['chain'] / max(r['first']['chain'], 1e-300):.3f}, other pixels {r['guide']['other'] / r['first']['other']:.3f}")
    return r


def test_following_specular_chains_pays_on_mirror_room():
    r = _report("MIRROR_ROOM")
    assert all(np.isfinite(o).all() for o in r["outs"].values())
    assert r["chain_pixels"] > 200
    assert r["guide"]["chain"] <= 0.5 * r["first"]["chain"]          # (a)
    assert r["guide"]["other"] <= 1.1 * r["first"]["other"]          # (b)
    assert r["guide"]["frame"] / r["noisy"] < r["first"]["frame"] / r["noisy"]   # (c)


@pytest.mark.parametrize("name", ["DEFAULT", "MATERIAL_TEST"])
def test_presets_with_few_chain_pixels_are_reported(name):
    r = _report(name)
    assert all(np.isfinite(o).all() for o in r["outs"].values())     # reported only: 54 chain pixels each


@pytest.mark.parametrize("name", ["MIRROR_ROOM", "MATERIAL_TEST"])
def test_no_specular_vertices_is_the_first_hit_set(name):
    g, _, scene, osc, cam = replay(name, 0)
    want = dr.oracle_features(osc, scene, cam, FX["W"], FX["H"])
    assert not g["bounces"].any() and np.array_equal(g["prim"], want["prim"])
    for k in ("albedo", "normal", "position", "depth"):
        assert np.array_equal(g[k].view(U32), want[k].view(U32)), k


@pytest.mark.parametrize("W,H", [(37, 29), (130, 67)])
def test_the_gpu_tests_scene_holds_every_case_of_the_chain(W, H):
    """MIRROR_ROOM's glass ball gives a dielectric vertex that reflects at some sizes only (none at the quality fixture's
    44 x 28), so the GPU tests' scene adds a glass pane seen from behind (guide_features_replay.mirror_room(pane=True)):
    total internal reflection at every size."""
    name = "MIRROR_ROOM+pane"
    g, trace, scene, _, _ = replay(name, 8, W, H)
    mtype = np.array([m.type for m in scene.materials])
    prim_mat = np.array([p.material_id for p in scene.primitives])
    type_of = lambda prim: np.where(prim >= 0, mtype[prim_mat[np.where(prim >= 0, prim, 0)]], 0)  # noqa: E731
    hit = g["prim"] >= 0
    assert ((type_of(g["prim"]) == 1) & (g["bounces"] >= 2) & trace["dielectric"]).any()   # a Lambertian through the glass
    first = replay(name, 0, W, H)[0]
    after_mirror = ~hit & (g["bounces"] == 1) & (type_of(first["prim"]) == 2)
    assert after_mirror.any()                                                        # a terminal miss after a mirror
    assert (g["albedo"][after_mirror] == F(0.9)).all() and not g["depth"][after_mirror].any()   # it carries T, and depth 0
    assert trace["dielectric_reflect"].any()                                         # a dielectric vertex that reflects
    assert not replay("MIRROR_ROOM", 8)[1]["dielectric_reflect"].any()              # (which the quality fixture lacks)
    one, trace1 = replay(name, 1, W, H)[:2]
    assert (trace1["capped"] & (one["bounces"] == 1)).any()                          # ends AT a specular surface: the cap
    assert (type_of(one["prim"])[trace1["capped"]] >= 2).all() and not trace["capped"].any()
    seen = hit & (g["bounces"] > 0)
    assert (g["depth"][seen] > first["depth"][seen]).all()                           # the chain's whole length


# ---- host-only context -------------------------------------------------------------------------------------------------
def _get(r):
    ft = r.get_feature_trace()
    return ft.max_specular, ft.roughness_max


def test_feature_trace_on_a_host_only_context():
    L = prt.capi.lib()
    r = prt.HipWavefrontRenderer(device=-1)
    d = prt.capi.PrtFeatureTrace(7, 7.0)
    L.prt_feature_trace_defaults(C.byref(d))
    assert (d.max_specular, d.roughness_max) == (0, F(0.1))
    assert _get(r) == (0, F(0.1))
    r.set_feature_trace(5, 0.25)
    assert _get(r) == (5, F(0.25))
    for bad in ((9, 0.1), (3, -0.5), (3, float("nan")), (3, float("inf")), (3, float("-inf")), (0xFFFFFFFF, 0.0)):
        assert L.prt_set_feature_trace(r._ctx, C.byref(prt.capi.PrtFeatureTrace(*bad))) == 1, bad
        assert b"feature trace" in L.prt_last_error(r._ctx)
        with pytest.raises(prt.PrtError):
            r.set_feature_trace(*bad)
        assert _get(r) == (5, F(0.25)), bad                                      # the previous setting, intact
    r.set_feature_trace(8, 0.0)
    assert _get(r) == (8, F(0.0))
    # kept across scene, film and camera
    r.set_scene_host_only(prt.Scene("CORNELL"))
    assert L.prt_set_film(r._ctx, 16, 8, 0, 1) == 0
    r.SetCamera(prt.Camera((3.0, 2.0, 1.0), width=16, height=8))
    assert _get(r) == (8, F(0.0))
    # nothing has been rendered (and nothing can be, here)
    assert L.prt_features_read_guide(r._ctx, None, None, None, None, None, None) == 1
    assert b"feature" in L.prt_last_error(r._ctx)
    assert L.prt_render_features(r._ctx) != 0
    assert L.prt_set_feature_trace(r._ctx, None) == 0 and _get(r) == (0, F(0.1))   # NULL: the defaults
