"""Guide features through specular chains on the GPU (include/prt.h "Guide features through specular chains").  Every
comparison is bit for bit against the numpy restatement (tests/guide_features_replay.py) fed with the context's own centre
rays and the oracle's linear-scan closest hit per round: albedo, normal, position, depth, prim and bounces.  The scene is
MIRROR_ROOM with the glass pane of the restatement's mirror_room(pane=True) (tests/test_guide_features_replay.py shows that it
holds every case of the chain); sizes are those at which the stream compaction of the live chains can go wrong."""
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_replay as dr
import guide_features_replay as gr
import temporal_replay as tr
import texture_replay as txr
import util
from util import prt

pytestmark = pytest.mark.gpu

U32 = np.uint32
F = np.float32
DEPTH, SEED, SPP = 5, 3, 8
CAM = (5.0, 5.0, 8.0)
BUNNY_CAM = (2.0, 1.5, 3.0)
FLOATS = ("albedo", "normal", "position", "depth")


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(U32), np.ascontiguousarray(b, F).view(U32))


def _diff(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    bad = a.view(U32) != b.view(U32)
    return f"{int(bad.sum())} of {bad.size} values differ, max |a - b| = {float(np.max(np.abs(a - b))):.3e}"


def _assert_set(got, want, what):
    assert np.array_equal(got["prim"], want["prim"]), (what, "prim", int((got["prim"] != want["prim"]).sum()))
    if "bounces" in want and "bounces" in got:
        assert np.array_equal(got["bounces"], want["bounces"]), (what, "bounces", int((got["bounces"] != want["bounces"]).sum()))
    for k in FLOATS:
        assert _same(got[k], want[k]), (what, k, _diff(got[k], want[k]))


def _equal_sets(a, b):
    return all(_same(a[k], b[k]) for k in FLOATS) and np.array_equal(a["prim"], b["prim"]) and np.array_equal(a.get("bounces"), b.get("bounces"))


def _renderer(scene, w, h, cam_pos=CAM, rank=0, world=1, stats=False, trace=None, lens=None):
    film = prt.Film(w, h)
    r = prt.HipWavefrontRenderer(device=0, max_depth=DEPTH, seed=SEED, rank=rank, world_size=world)
    r.Init(film, scene, prt.Camera(position=cam_pos, width=w, height=h))
    if lens:
        r.set_lens(**lens)
    if trace is not None:
        r.set_feature_trace(*trace)
    if stats:
        r.set_film_statistics(True)
    return r, film


def _centre_rays(r, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return r.camera_rays(xs.ravel().astype(F) + F(0.5), ys.ravel().astype(F) + F(0.5))


def _textured_albedo(r, scene):
    """albedo_of for the restatement: the material table, and for a textured material prt_texture_eval at the UV prt_hit_uv
    reports for the segment (what test_gpu_denoise.py builds the first-hit albedo from)."""
    table = np.array([[m.rgb[0], m.rgb[1], m.rgb[2]] for m in scene.materials], F)

    def albedo_of(o, d, hits):
        _, uv, _ = r.hit_uv(o, d)
        alb = table[np.where(hits["prim"] >= 0, hits["material_id"], 0)]
        for m, t in scene.material_texture.items():
            sel = (hits["prim"] >= 0) & (hits["material_id"] == m)
            if sel.any():
                alb[sel] = r.texture_eval(t, uv[sel])
        return alb
    return albedo_of


def _replay(r, scene, w, h, max_specular, roughness_max=0.1, trace=None):
    o, d = _centre_rays(r, w, h)
    return gr.guide_features(gr.linear_scan(util.oracle_scene(scene)), scene, o, d, w, h, max_specular=max_specular, roughness_max=roughness_max,
                             albedo_of=_textured_albedo(r, scene) if scene.material_texture else None, trace=trace)


@functools.lru_cache(maxsize=None)
def _room():
    return gr.mirror_room(pane=True)


# ---- 1. sizes and depths ---------------------------------------------------------------------------------------------------
# 37 x 29: 1073 pixels, some 400 live chains after the start kernel (not a multiple of 64 or 256) and fewer than a wave in
# the late rounds; 70 x 5: 13 live chains, less than a wave from the start; 1 x 1: one chain (the glass ball); 130 x 67:
# 8710 pixels and some 2700 live chains, beyond 1024 entries over several blocks.
@pytest.mark.parametrize("w,h,max_specular", [(37, 29, 8), (70, 5, 8), (1, 1, 8), (130, 67, 8), (37, 29, 1), (37, 29, 3)])
def test_guide_set_equals_the_restatement_bit_for_bit(w, h, max_specular):
    scene = _room()
    r, _ = _renderer(scene, w, h, trace=(max_specular, 0.1))
    got = r.render_features()
    trace = {}
    want = _replay(r, scene, w, h, max_specular, trace=trace)
    live = int((want["bounces"] > 0).sum())
    print(f"{w}x{h}, max_specular {max_specular}: {live} chains, bounces up to {int(want['bounces'].max())}, {int(trace['capped'].sum())} at the cap")
    _assert_set(got["guide"], want, (w, h, max_specular))
    _assert_set({k: got[k] for k in FLOATS + ("prim",)}, _replay(r, scene, w, h, 0), (w, h, "first-hit set"))
    assert live >= 1 and want["bounces"].max() >= min(2, max_specular)
    if (w, h) == (130, 67):
        assert live > 1024
    if (w, h) == (37, 29):
        assert live % 64 and trace["dielectric_reflect"].any() and ((want["prim"] < 0) & (want["bounces"] > 0)).any()
        assert trace["capped"].any() == (max_specular < 8)
    again = r.render_features()                                              # the list's order may differ; nothing written does
    assert _equal_sets(again["guide"], got["guide"])


def test_without_specular_vertices_there_is_no_guide_set():
    L = prt.capi.lib()
    scene = _room()
    r, _ = _renderer(scene, 37, 29)
    feat = r.render_features()
    assert "guide" not in feat
    g = dict(albedo=np.zeros((29, 37, 3), F), normal=np.zeros((29, 37, 3), F), position=np.zeros((29, 37, 3), F), depth=np.zeros((29, 37), F),
             prim=np.zeros((29, 37), np.int32), bounces=np.full((29, 37), 7, U32))
    fp, ip, up = prt.capi.C.POINTER(prt.capi.C.c_float), prt.capi.C.POINTER(prt.capi.C.c_int32), prt.capi.C.POINTER(prt.capi.C.c_uint32)
    assert L.prt_features_read_guide(r._ctx, g["albedo"].ctypes.data_as(fp), g["normal"].ctypes.data_as(fp), g["position"].ctypes.data_as(fp),
                                     g["depth"].ctypes.data_as(fp), g["prim"].ctypes.data_as(ip), g["bounces"].ctypes.data_as(up)) == 0
    assert not g["bounces"].any()
    _assert_set(g, feat, "max_specular 0")
    r.set_feature_trace(2, 0.1)
    r.set_feature_trace(0, 0.1)                                              # on and off again: the same
    _assert_set(r.render_features(), feat, "off again")


def test_a_rough_metal_is_an_ordinary_surface():
    scene = gr.mirror_room(pane=True)
    scene.materials[2].scalar = 0.25                                         # the mirrors, now rougher than roughness_max
    r, _ = _renderer(scene, 37, 29, trace=(8, 0.1))
    got = r.render_features()["guide"]
    _assert_set(got, _replay(r, scene, 37, 29, 8), "roughness 0.25 > 0.1")
    r.set_feature_trace(8, 0.25)                                             # <=: a mirror again
    wide = r.render_features()["guide"]
    _assert_set(wide, _replay(r, scene, 37, 29, 8, roughness_max=0.25), "roughness 0.25 <= 0.25")
    assert (wide["bounces"] > 0).sum() > (got["bounces"] > 0).sum() > 0


# ---- 2. a mesh scene: a two-level tree, textured T and textured terminal albedo ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh_scene():
    """A bunny (a world-space mesh) on a checkered ground under a light, a mirror placed copy of it, and a placed copy of
    cube_uv whose mirror material is textured."""
    sc = prt.scenes.mesh_scene(prt.Mesh(prt.scenes.asset("bunny.ply")))
    mirror = sc.AddMetal((0.9, 0.9, 0.9), 0.0)
    sc.AddInstance(prt.Mesh(prt.scenes.asset("bunny.ply")), mirror, scale=0.8, euler_deg=(0.0, 40.0, 0.0), translation=(-1.3, -0.3, 0.2))
    tinted = sc.AddMetal((0.8, 0.8, 0.8), 0.05)
    sc.AddInstance(prt.Mesh(prt.scenes.asset("cube_uv.ply")), tinted, scale=0.7, euler_deg=(0.0, 30.0, 0.0), translation=(1.2, -0.3, 0.4))
    sc.SetMaterialTexture(tinted, sc.AddTexture(txr._random_image(5, 3, 1), "bilinear", "repeat"))
    sc.SetMaterialTexture(0, sc.AddTexture(prt.scenes.checker(4, (0.9, 0.85, 0.8), (0.15, 0.2, 0.1)), "nearest", "repeat"))
    return sc, mirror, tinted


def test_mesh_scene_with_textures_a_lens_and_a_partition():
    w, h = 44, 28
    scene, mirror, tinted = _mesh_scene()
    fov = dict(fov_y=0.8)
    r, _ = _renderer(scene, w, h, BUNNY_CAM, trace=(4, 0.1), lens=fov)
    got = r.render_features()
    want = _replay(r, scene, w, h, 4)
    _assert_set(got["guide"], want, "bunny, fov")
    first = {k: got[k] for k in FLOATS + ("prim",)}
    _assert_set(first, _replay(r, scene, w, h, 0), "bunny, fov, first-hit set")
    # both mirrors are seen and followed; behind the textured one lies the textured ground: T and the albedo are textured
    o, d = _centre_rays(r, w, h)
    hits = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8).reshape(h, w)
    chain = want["bounces"] > 0
    via_tinted = chain & (hits["material_id"] == tinted) & (want["prim"] == 0)
    assert (chain & (hits["material_id"] == mirror)).sum() > 10 and via_tinted.sum() > 5
    assert len(np.unique(want["albedo"][via_tinted].reshape(-1, 3), axis=0)) > 3
    assert not _same(got["guide"]["albedo"], got["albedo"])
    # an aperture is ignored, as for the first-hit set; rank 1 of 3 covers the whole image
    ra, _ = _renderer(scene, w, h, BUNNY_CAM, trace=(4, 0.1), lens=dict(fov_y=0.8, aperture=0.2, focus_distance=6.0))
    rp, _ = _renderer(scene, w, h, BUNNY_CAM, rank=1, world=3, trace=(4, 0.1), lens=fov)
    for other, what in ((ra, "aperture"), (rp, "rank 1 of 3")):
        f = other.render_features()
        assert _equal_sets(f["guide"], got["guide"]), what
        assert _equal_sets({k: f[k] for k in FLOATS + ("prim",)}, first), what
    # the placed copies' transforms given again drop both sets, like every call of the invalidation list
    L = prt.capi.lib()
    assert L.prt_features_read_guide(r._ctx, None, None, None, None, None, None) == 0
    r.UpdateInstances(scene)
    assert L.prt_features_read_guide(r._ctx, None, None, None, None, None, None) == 1
    assert _equal_sets(r.render_features()["guide"], got["guide"])
    # without the binding the material table is used
    r.set_textures(None)
    plain = prt.Scene(preset=None)
    plain.materials, plain.primitives, plain.meshes = scene.materials, scene.primitives, scene.meshes
    plain.instanced_meshes, plain.instances = scene.instanced_meshes, scene.instances
    _assert_set(r.render_features()["guide"], _replay(r, plain, w, h, 4), "bunny, no binding")


# ---- 3. the cap -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_specular", [1, 3])
def test_two_facing_mirrors_reach_the_cap(max_specular):
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.6, 0.6, 0.6))
    light = sc.AddEmissive((4.0, 4.0, 4.0))
    mirror = sc.AddMetal((0.9, 0.8, 0.7), 0.0)
    sc.AddQuad(40.0, 40.0, ground)
    sc.AddCircle(0.5, light, translation=(0.0, 9.0, 4.0))
    sc.AddQuad(30.0, 12.0, mirror, euler_deg=(90.0, 0.0, 0.0), translation=(0.0, 6.0, -4.0))
    sc.AddQuad(30.0, 12.0, mirror, euler_deg=(-90.0, 0.0, 0.0), translation=(0.0, 6.0, 12.0))
    w, h = 37, 29
    r, _ = _renderer(sc, w, h, trace=(max_specular, 0.1))
    trace = {}
    want = _replay(r, sc, w, h, max_specular, trace=trace)
    capped = trace["capped"]
    assert capped.sum() > 20 and (want["bounces"][capped] == max_specular).all()      # pixels that end AT a mirror
    got = r.render_features()["guide"]
    _assert_set(got, want, ("facing mirrors", max_specular))
    t = np.array([0.9, 0.8, 0.7], F)
    end = np.ones(3, F)
    for _ in range(max_specular + 1):                                                 # T of max_specular mirrors times the last one's rgb
        end = (end * t).astype(F)
    assert (got["albedo"][capped] == end).all()


# ---- 4. the mode leaves everything else alone ---------------------------------------------------------------------------------
def test_first_hit_set_film_moments_and_ray_counts_do_not_change():
    scene = _room()
    w, h = 44, 28
    state = []
    for trace in (None, (8, 0.1)):
        r, film = _renderer(scene, w, h, stats=True, trace=trace)
        feat = r.render_features()
        r.ProgressiveRender(2)
        r.download()
        A, Q = r.film_statistics()
        st = r.stats()
        state.append((feat, film.accum.copy(), film.weights.copy(), A, Q, st.rays_total, list(st.rays_per_depth), st.samples))
    off, on = state
    assert "guide" in on[0] and "guide" not in off[0]
    assert _equal_sets({k: on[0][k] for k in FLOATS + ("prim",)}, off[0])
    assert all(_same(a, b) for a, b in zip(on[1:5], off[1:5]))
    assert on[5:] == off[5:] and on[5] > 0


def test_stale_guide_features_are_refused():
    L = prt.capi.lib()
    scene = _room()
    w, h = 37, 29
    r, _ = _renderer(scene, w, h, trace=(8, 0.1))
    read = lambda: L.prt_features_read_guide(r._ctx, None, None, None, None, None, None)  # noqa: E731
    assert read() == 1                                                       # none yet
    r.render_features()
    assert read() == 0
    for change in (lambda: r.SetCamera(prt.Camera(position=(4.0, 5.0, 8.0), width=w, height=h)), lambda: r.set_lens(fov_y=0.7),
                   lambda: r.set_textures(None), lambda: L.prt_set_film(r._ctx, w, h, 0, 1),
                   lambda: r.Init(prt.Film(w, h), scene, prt.Camera(position=CAM, width=w, height=h)), lambda: r.set_feature_trace(3, 0.1),
                   lambda: r.set_feature_trace(0, 0.1), lambda: L.prt_set_feature_trace(r._ctx, None)):
        change()
        assert read() == 1 and b"feature" in L.prt_last_error(r._ctx)
        assert L.prt_features_read(r._ctx, None, None, None, None, None) == 1
        r.render_features()
        assert read() == 0
    assert L.prt_set_feature_trace(r._ctx, prt.capi.C.byref(prt.capi.PrtFeatureTrace(9, 0.1))) == 1      # a refusal drops the set too
    assert read() == 1 and r.get_feature_trace().max_specular == 0


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------
def _film_state(r, film):
    r.download()
    A, Q = r.film_statistics()
    return film.accum.copy(), film.weights.copy(), A, Q


def test_film_denoise_is_guided_by_the_guide_set():
    w, h = 44, 28
    r, film = _renderer(_room(), w, h, stats=True, trace=(8, 0.1))
    r.ProgressiveRender(SPP)
    state = _film_state(r, film)
    got, got_var = r.denoise(return_variance=True)
    assert all(_same(a, b) for a, b in zip(state, _film_state(r, film)))
    feat = r.render_features()
    g = feat["guide"]
    mean, var = dr.film_inputs(*state)
    want, want_var = r.denoise_arrays(mean, var, g["albedo"], g["normal"], g["position"], g["prim"], return_variance=True)
    assert _same(got, want), _diff(got, want)
    assert _same(got_var, want_var), _diff(got_var, want_var)
    replayed, _ = dr.denoise(mean, var, g["albedo"], g["normal"], g["position"], g["prim"], guard=False)
    assert _same(got, replayed), _diff(got, replayed)
    r.set_feature_trace(0)
    off = r.denoise()
    assert _same(off, r.denoise_arrays(mean, var, feat["albedo"], feat["normal"], feat["position"], feat["prim"]))
    assert not _same(off, got)
    chain = g["bounces"] > 0
    assert np.isfinite(got).all() and (off[chain] != got[chain]).any()


def _orbit(pos, deg):
    a = np.deg2rad(deg)
    return (float(pos[0] * np.cos(a) + pos[2] * np.sin(a)), float(pos[1]), float(-pos[0] * np.sin(a) + pos[2] * np.cos(a)))


def test_temporal_step_reprojects_by_the_first_hit_and_filters_by_the_guide_set():
    w, h = 44, 28
    scene = _room()
    reprojected = {}
    for mode in ("on", "off"):
        r, film = _renderer(scene, w, h, stats=True, trace=(8, 0.1) if mode == "on" else None)
        hist, Kprev, pos = None, None, CAM
        for f in range(2):
            if f:
                pos = _orbit(pos, 2.0)
                r.SetCamera(prt.Camera(position=pos, width=w, height=h))
                film.Clear()
            r.ProgressiveRender(SPP)
            state = _film_state(r, film)
            feat = r.render_features()
            K = r.camera_basis()
            got, got_var = r.temporal_step(return_variance=True, denoise={})
            reprojected.setdefault(mode, []).append(r.temporal_info().reprojected)
            if mode == "off":
                continue
            c, n = tr.frame_inputs(*state)
            blend = r.temporal_arrays(Kprev if Kprev is not None else K, c, n, state[2], state[3], feat["prim"], feat["position"], feat["normal"],
                                      history=hist)
            g = feat["guide"]
            want, want_var = r.denoise_arrays(blend["c"], blend["var"], g["albedo"], g["normal"], g["position"], g["prim"], return_variance=True)
            assert _same(got, want), (f, _diff(got, want))
            assert _same(got_var, want_var), (f, _diff(got_var, want_var))
            assert r.temporal_info().reprojected == int(blend["status"].sum())
            first_only = r.denoise_arrays(blend["c"], blend["var"], feat["albedo"], feat["normal"], feat["position"], feat["prim"])
            assert not _same(got, first_only)
            hist = tr.next_history(blend, feat["position"], feat["normal"], feat["prim"])
            Kprev = K
    assert reprojected["on"] == reprojected["off"] and reprojected["on"][0] == 0 and reprojected["on"][1] > 0.5 * w * h


def test_a_group_of_three_ranks_on_one_device_equals_the_single_context():
    w, h = 44, 28
    scene = _room()
    r, _ = _renderer(scene, w, h, stats=True, trace=(8, 0.1))
    r.ProgressiveRender(SPP)
    want = r.denoise()
    g = prt.HipWavefrontGroupRenderer([0, 0, 0], max_depth=DEPTH, seed=SEED)
    g.Init(prt.Film(w, h), scene, prt.Camera(position=CAM, width=w, height=h))
    g.set_film_statistics(True)
    g.ProgressiveRender(SPP)
    off = g.denoise()
    g.set_feature_trace(8, 0.1)
    got = g.denoise()
    assert _same(got, want), _diff(got, want)
    assert not _same(off, got)
    gf, sf = g.render_features(), r.render_features()
    assert _equal_sets(gf["guide"], sf["guide"]) and _equal_sets({k: gf[k] for k in FLOATS + ("prim",)}, {k: sf[k] for k in FLOATS + ("prim",)})
    ft = prt.capi.PrtFeatureTrace()
    for rank in range(3):
        assert prt.capi.lib().prt_get_feature_trace(prt.capi.lib().prt_group_context(g._grp, rank), prt.capi.C.byref(ft)) == 0
        assert (ft.max_specular, ft.roughness_max) == (8, F(0.1))
    with pytest.raises(prt.PrtError):
        g.set_feature_trace(9, 0.1)


def test_prt_render_follow_specular_writes_what_the_python_call_returns(tmp_path):
    w, h = 44, 28
    exe = os.path.join(util.ROOT, "parallelraytracing_amd", "csrc", "prt_render")
    out = str(tmp_path / "frame")
    p = subprocess.run([exe, "--preset", "MATERIAL_TEST", "--width", str(w), "--height", str(h), "--depth", str(DEPTH), "--seed", str(SEED),
                        "--camera", "5", "5", "8", "--spp", str(SPP), "--denoise", "--follow-specular", "8", "--mirror-roughness", "0.1",
                        "--features-out", out, "--out", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    r, film = _renderer(prt.Scene("MATERIAL_TEST"), w, h, stats=True, trace=(8, 0.1))
    r.ProgressiveRender(SPP)
    want = r.denoise()
    assert _same(prt.read_pfm(out + "_denoised.pfm"), want)
    feat = r.render_features()
    assert (feat["guide"]["bounces"] > 0).sum() > 20
    for k in ("albedo", "normal", "position"):
        assert _same(prt.read_pfm(f"{out}_{k}.pfm"), feat[k]), k
        assert _same(prt.read_pfm(f"{out}_guide_{k}.pfm"), feat["guide"][k]), k
    assert _same(prt.read_pfm(out + "_guide_depth.pfm")[..., 0], feat["guide"]["depth"])
    assert np.array_equal(prt.read_pfm(out + "_guide_bounces.pfm")[..., 0], feat["guide"]["bounces"].astype(F))
    r.set_feature_trace(0)
    assert not _same(r.denoise(), want)
