"""Image textures (include/prt.h "Image textures") on one MI355X, against the numpy-float32 restatement
(tests/texture_replay.py, whose gate and laws tests/test_texture_replay.py checks on the CPU).

  1. prt_texture_eval equals the restatement bit for bit: both filters, both wraps, 1 x 1, 3 x 5 and 16 x 16, on a UV grid
     with 0, 1, every texel edge and centre and their fp32 neighbours, negative values and values above 1.
  2. prt_hit_uv: hits equal prt_closest_hit, UVs and albedo equal the restatement bit for bit (scenes A and B, primary and
     random rays).
  3. Frames, lighting off: the film equals the replay's per-pixel fp32 sum in sample order bit for bit and rays_per_depth its
     segment counts (A x jitter 0 / 1 x 1, 3, 9 samples per call, B, roulette + clamp).
  4. A 1 x 1 texture equals the constant material bit for bit (against the untextured scene on its compact / fused routes;
     lighting off, mis, mis with an environment); a checker changes the frame.
  5. Lighting modes through the existing float64 replays with the textured walker (tolerances and checks are the replays').
  6. The frame of scene B does not depend on tunables, batching, the partition, the builder or the node stride.
  7. After Refit, UpdateInstances (both modes) and a clone the frame equals a fresh Init of the same description.
  8. The group renderer and the prt_render command line equal the single-context frame.
Every frame is 48 x 36 or 40 x 30 at depth 4.

Figures of the first run on an MI355X (all 40 cases pass, the file in under 10 s): every bit-for-bit comparison exact; the
lighting replays (compared / left out as undecidable / worst error over tolerance / shadow rays GPU = replay / occluded):
  A_mis_analytic  6912 / 0 / 0.053 / 3918 = 3918 / 142      B_nee_analytic  4799 / 1 / 0.046 / 3038 = 3038 / 375
  B_mis_mesh      4800 / 0 / 0.042 / 3041 = 3041 / 413      A_mis_env       6909 / 3 / 0.239 / 3968 = 3968 / 94
  B_nee_mesh_env  4800 / 0 / 0.220 / 3207 = 3207 / 272"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import environment_replay as er
import lighting_replay as lr
import mesh_light_replay as mr
import texture_replay as tr
import util
from parallelraytracing_amd import scenes
from util import orc, prt

pytestmark = pytest.mark.gpu
F = np.float32
capi = prt.capi


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _renderer(c, sif=4, sampling=None, lighting=None, sources=None, env=None, rank=0, world=1, params=(), group=None, seed=tr.SEED):
    film = prt.Film(c["W"], c["H"])
    if group:
        r = prt.HipWavefrontGroupRenderer(group, max_depth=c["depth"], seed=seed)
    else:
        r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=seed, rank=rank, world_size=world)
    for k, v in params:
        r.set_param(k, v)
    if sources:
        r.set_light_sources(sources)
    if env is not None:
        r.set_environment(env[0], env[1])
    r.Init(film, c["scene"], c["cam"])
    r.set_samples_in_flight(sif)
    if sampling:
        r.set_sampling(*sampling)
    if lighting:
        r.set_lighting(lighting)
    return r, film


def _frame(c, spp=4, calls=None, **kw):
    r, film = _renderer(c, **kw)
    for k in (calls or [spp]):
        r.ProgressiveRender(k)
    r.download()
    return film.accum.copy(), film.weights.copy(), r


# ---- 1. the lookup ------------------------------------------------------------------------------------------------------------
def test_texture_eval_equals_the_restatement_bit_for_bit():
    sc = prt.Scene(preset=None)
    sc.AddQuad(4.0, 4.0, sc.AddLambertian((0.5, 0.5, 0.5)))
    combos = []
    for k, (h, w) in enumerate(((1, 1), (5, 3), (16, 16))):
        img = tr._random_image(h, w, 20 + k)
        for filt in ("nearest", "bilinear"):
            for wrp in ("repeat", "clamp"):
                combos.append((sc.AddTexture(img, filt, wrp), img, capi.TEX_FILTERS[filt], capi.TEX_WRAPS[wrp]))
    c = dict(scene=sc, cam=prt.Camera(width=8, height=8), W=8, H=8, depth=2)
    r, _ = _renderer(c)
    info = r.texture_info()
    assert (info.is_set, info.n_textures, info.n_textured_materials) == (1, 12, 0) and info.device_bytes > 0
    n = 0
    for t, img, filt, wrp in combos:
        uv = tr.eval_grid(img.shape[1], img.shape[0])
        got = r.texture_eval(t, uv)
        want = tr.lookup(img, filt, wrp, uv[:, 0], uv[:, 1])
        bad = np.nonzero((_bits(got) != _bits(want)).any(1))[0]
        assert len(bad) == 0, (img.shape, filt, wrp, uv[bad[:4]], got[bad[:4]], want[bad[:4]])
        n += len(uv)
    assert n > 10000
    for n in util.WORKSPACE_COUNTS:      # (the last combination's grid, cut to each length)
        got = r.texture_eval(t, uv[:n])
        assert np.array_equal(_bits(got), _bits(tr.lookup(img, filt, wrp, uv[:n, 0], uv[:n, 1]))), n
    # refusals of the eval call itself
    with pytest.raises(prt.PrtError, match="out of range"):
        r.texture_eval(12, [[0.5, 0.5]])
    with pytest.raises(prt.PrtError, match="finite"):
        r.texture_eval(0, [[np.nan, 0.5]])


# ---- 2. UV and albedo of hits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_hit_uv_equals_the_restatement_bit_for_bit(name):
    c = tr.scene_a() if name == "A" else tr.scene_b()
    ts = tr.TexScene(c["scene"])
    o, d = tr.primary_and_random_rays(c)
    r, _ = _renderer(c)
    hits, uv, alb = r.hit_uv(o, d)
    assert util.hits_equal(hits, r.closest_hit(o, d)) == []
    want_hits = orc.OracleScene(c["scene"].desc()).closest_hit(o, d, use_bvh=True, n_threads=lr.n_threads_default())
    assert util.hits_equal(hits, want_hits) == []
    want_uv, _ = ts.hit_uv(o, d, hits)
    want_alb = ts.albedo(hits, want_uv)
    assert np.array_equal(uv, want_uv), np.abs(uv - want_uv).max()
    assert np.array_equal(_bits(alb), _bits(want_alb))
    hit = hits["prim"] >= 0
    assert ts.textured(hits).sum() > 500 and (~hit).sum() > 500
    assert np.all(uv[~hit] == 0) and np.all(alb[~hit] == 0)
    if name == "A":   # the cube's UVs reach beyond [0, 1] on both sides, the ground's stay inside
        cube = (hits["prim"] >= ts.n_prims) & (hits["prim"] < ts.n_prims + ts.n_world)
        assert uv[cube].min() < -0.2 and uv[cube].max() > 1.2
        ground = hits["prim"] == 0
        assert uv[ground].min() >= 0.0 and uv[ground].max() <= 1.0 and ground.sum() > 500
    o, d = tr.primary_and_random_rays(c, n_random=3000, seed=4)
    want_hits = orc.OracleScene(c["scene"].desc()).closest_hit(o, d, use_bvh=True, n_threads=lr.n_threads_default())
    for n in util.WORKSPACE_COUNTS:
        hits, uv, alb = r.hit_uv(o[:n], d[:n])
        assert util.hits_equal(hits, want_hits[:n]) == [], n
        want_uv, _ = ts.hit_uv(o[:n], d[:n], hits)
        assert np.array_equal(uv, want_uv) and np.array_equal(_bits(alb), _bits(ts.albedo(hits, want_uv))), n


# ---- 3. frames, lighting off --------------------------------------------------------------------------------------------------
_REPLAYS = {}


def _replay_frame(key, c, spp, sampling):
    if key not in _REPLAYS:
        osc = orc.OracleScene(c["scene"].desc())
        _REPLAYS[key] = tr.frame(c["scene"], osc, c["cam"], c["W"], c["H"], c["depth"], tr.SEED, 0, spp, sampling)
    return _REPLAYS[key]


def _check_frame(c, key, spp, calls, sampling, sif=4):
    want, wwts, per_depth = _replay_frame(key, c, spp, sampling)
    got, wts, r = _frame(c, calls=calls, sampling=sampling if sampling != (0, 0, 0.0) else None, sif=sif)
    bad = np.nonzero((_bits(got) != _bits(want)).any(2))
    assert len(bad[0]) == 0, (key, calls, len(bad[0]), got[bad][:3], want[bad][:3])
    assert np.array_equal(wts, wwts)
    st = r.stats()
    assert list(st.rays_per_depth[:c["depth"]]) == per_depth.tolist() and st.rays_total == per_depth.sum()


@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("per_call", [1, 3, 9])
def test_scene_a_film_equals_the_replay_bit_for_bit(jitter, per_call):
    _check_frame(tr.scene_a(), ("A", jitter), 9, [per_call] * (9 // per_call), (jitter, 0, 0.0))


def test_scene_b_film_equals_the_replay_bit_for_bit():
    _check_frame(tr.scene_b(), ("B", 0), 4, [4], (0, 0, 0.0))


@pytest.mark.parametrize("name", ["A", "B"])
def test_roulette_and_clamp_film_equals_the_replay_bit_for_bit(name):
    c = tr.scene_a() if name == "A" else tr.scene_b()
    _check_frame(c, (name, "rr"), 4, [1, 3], (1, 1, 0.75))


# ---- 4. a 1 x 1 texture is the constant material ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["off", "mis", "mis_env"])
def test_one_by_one_textures_equal_the_untextured_scene_bit_for_bit(mode):
    kw = dict(lighting=None if mode == "off" else "mis", env=(er.named_map("sun"), 0.5) if mode == "mis_env" else None)
    flat, wf, rf = _frame(tr.scene_a("flat"), spp=4, **kw)
    none, wn, rn = _frame(tr.scene_a("none"), spp=4, **kw)
    assert rf.texture_info().n_textured_materials == 3 and rn.texture_info().is_set == 0
    assert np.array_equal(_bits(flat), _bits(none)) and np.array_equal(wf, wn)
    assert list(rf.stats().rays_per_depth) == list(rn.stats().rays_per_depth)
    full, _, _ = _frame(tr.scene_a("full"), spp=4, **kw)
    changed = (_bits(full) != _bits(none)).any(2).mean()
    assert changed > 0.3, changed     # the checkered ground alone covers more than that
    # taking the binding away again gives the untextured frame on the same context
    rf.set_textures(None)
    rf.film.Clear()
    rf.frame_index = 0
    rf.ProgressiveRender(4)
    rf.download()
    assert np.array_equal(_bits(rf.film.accum), _bits(none))


# ---- 5. lighting modes through the existing replays ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.LIGHTING_CASES)
def test_lighting_modes_match_the_float64_replays(monkeypatch, name):
    tr.patch_walk(monkeypatch)
    c, mode, fn = tr.lighting_case(name)
    rep = fn(c, orc.OracleScene(c["scene"].desc()))
    with_env = name.endswith("_env")
    r, film = _renderer(c, sif=4, lighting=mode, sources="all" if c["sources"] == "all" else None,
                        env=(er.named_map(c["env"]), c["light_share"]) if with_env else None, seed=lr.SEED)
    r.reset_stats()
    frames = lr.render_samples(r, film, lr.SAMPLES)
    r.synchronize()
    if with_env:
        rec = er.check_against_gpu(rep, frames, r.light_stats())
    elif c["sources"] == "all":
        rec = mr.check_gpu(rep, frames, r.light_stats(), r.light_info(), r.light_intervals())
    else:
        rec = lr.check_against_gpu(rep, frames, r.light_stats(), r.light_info())
    assert rec["compared"] >= 0.995 * len(rep.pix)


# ---- 6. independence of the route ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def b_frame():
    c = tr.scene_b()
    acc, wts, r = _frame(c, spp=4)
    return c, acc, wts, list(r.stats().rays_per_depth)


@pytest.mark.parametrize("route", ["fuse0", "fuse1", "exact_grids2", "primary_walk0", "path_kernel2", "sif1", "sif16", "calls_1_3",
                                   "gpu_build1", "gpu_build2", "node_stride5", "node_stride8"])
def test_scene_b_frame_does_not_depend_on_the_route(b_frame, route):
    c, want, wwts, per_depth = b_frame
    kw = {}
    if route.startswith("sif"):
        kw["sif"] = int(route[3:])
    elif route == "calls_1_3":
        kw["calls"] = [1, 3]
    else:
        name = route.rstrip("0123456789")
        kw["params"] = [(name, int(route[len(name):]))]
    got, wts, r = _frame(c, spp=4, **kw)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(wts, wwts)
    assert list(r.stats().rays_per_depth) == per_depth
    if route.startswith("gpu_build"):
        assert r.bvh_info().built_on_device == 1


def test_scene_b_frame_does_not_depend_on_the_partition(b_frame):
    c, want, wwts, per_depth = b_frame
    acc, wts, rays = np.zeros_like(want), np.zeros_like(wwts), np.zeros(len(per_depth), np.int64)
    for rank in range(3):
        a, w, r = _frame(c, spp=4, rank=rank, world=3)
        assert np.all((w == 0) | (wts == 0))   # every pixel belongs to one rank
        acc += a
        wts += w
        rays += np.array(list(r.stats().rays_per_depth), np.int64)
    assert np.array_equal(_bits(acc), _bits(want)) and np.array_equal(wts, wwts) and rays.tolist() == per_depth


# ---- 7. refit, instance update, clone -----------------------------------------------------------------------------------------
def test_refit_keeps_the_binding():
    c = tr.scene_b(copies=False)
    r, film = _renderer(c)
    r.ProgressiveRender(2)
    info = r.texture_info()
    bunny = c["scene"].meshes[0][0]
    v = bunny.GetVertices()
    bent = prt.Mesh(vertices=v * F(1.0) + F(0.05) * np.sin(v[:, [1, 2, 0]] * F(7.0)).astype(F), normals=bunny.GetNormals(),
                    indices=bunny.GetIndices(), uvs=bunny.GetUVs())
    c["scene"].meshes[0] = (bent, c["scene"].meshes[0][1])
    r.Refit(c["scene"])
    after = r.texture_info()
    assert (after.is_set, after.n_uv_triangles, after.n_texels, after.device_bytes) == (1, info.n_uv_triangles, info.n_texels, info.device_bytes)
    film.Clear()
    r.frame_index = 0
    r.ProgressiveRender(4)
    r.download()
    want, wwts, _ = _frame(c, spp=4)
    assert np.array_equal(_bits(film.accum), _bits(want)) and np.array_equal(film.weights, wwts)
    ref, _, _ = _frame(tr.scene_b(copies=False), spp=4)
    assert not np.array_equal(ref, want)    # the deformation is visible


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_instance_update_keeps_the_binding(mode):
    c = tr.scene_b()
    r, film = _renderer(c)
    r.ProgressiveRender(1)
    before, _, _ = _frame(c, spp=4)
    c["scene"].SetInstanceTransform(0, scale=0.55, euler_deg=(40.0, 10.0, 5.0), translation=(1.4, -0.2, 1.0))
    c["scene"].SetInstanceTransform(1, scale=0.35, euler_deg=(0.0, 20.0, 0.0), translation=(-1.5, -0.4, 0.9))
    r.UpdateInstances(c["scene"], mode)
    assert r.texture_info().n_textured_materials == 3
    film.Clear()
    r.frame_index = 0
    r.ProgressiveRender(4)
    r.download()
    want, wwts, _ = _frame(c, spp=4)
    assert np.array_equal(_bits(film.accum), _bits(want)) and np.array_equal(film.weights, wwts)
    assert not np.array_equal(before, want)
    # and the UVs of the moved copies are still those of the restatement
    ts = tr.TexScene(c["scene"])
    o, d = tr.primary_and_random_rays(c, n_random=500)
    hits, uv, alb = r.hit_uv(o, d)
    want_uv, _ = ts.hit_uv(o, d, hits)
    assert np.array_equal(uv, want_uv) and np.array_equal(_bits(alb), _bits(ts.albedo(hits, want_uv)))


def test_clone_copies_the_binding():
    c = tr.scene_b()
    want, wwts, src = _frame(c, spp=4)
    film = prt.Film(c["W"], c["H"])
    dst = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=tr.SEED)
    L = capi.lib()
    assert L.prt_clone_scene(dst._ctx, src._ctx) == 0
    assert L.prt_set_film(dst._ctx, c["W"], c["H"], 0, 1) == 0
    dst.film = film
    film._renderer = dst
    dst.SetCamera(c["cam"])
    dst.set_samples_in_flight(4)
    a, b = dst.texture_info(), src.texture_info()
    assert (a.is_set, a.n_textures, a.n_textured_materials, a.n_uv_triangles, a.n_texels, a.device_bytes) == \
           (1, b.n_textures, b.n_textured_materials, b.n_uv_triangles, b.n_texels, b.device_bytes)
    del src     # the clone owns its copy
    dst.ProgressiveRender(4)
    dst.download()
    assert np.array_equal(_bits(film.accum), _bits(want)) and np.array_equal(film.weights, wwts)


# ---- 8. group renderer and command line ---------------------------------------------------------------------------------------
def test_group_renderer_binds_the_textures_on_every_rank():
    c = tr.scene_b()
    want, wwts, _ = _frame(c, spp=4)
    g, film = _renderer(c, group=[0, 0])
    for rank in range(2):
        assert g.texture_info(rank).n_textured_materials == 3
    g.ProgressiveRender(4)
    g.download()
    assert np.array_equal(_bits(film.accum), _bits(want)) and np.array_equal(film.weights, wwts)
    # moving the copies keeps the binding on every rank
    c["scene"].SetInstanceTransform(0, scale=0.5, euler_deg=(0.0, 50.0, 0.0), translation=(-1.2, -0.3, 1.2))
    g.UpdateInstances(c["scene"], "refit")
    g.Clear()
    g.ProgressiveRender(4)
    g.download()
    moved, mw, _ = _frame(c, spp=4)
    assert np.array_equal(_bits(film.accum), _bits(moved)) and np.array_equal(film.weights, mw)


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_cli_renders_the_textured_frame_of_the_python_path(tmp_path, filt):
    exe = os.path.join(util.ROOT, "parallelraytracing_amd", "csrc", "prt_render")
    out, pfm = str(tmp_path / "frame"), str(tmp_path / "checker.pfm")
    img = scenes.checker(8, (0.9, 0.2, 0.1), (0.1, 0.3, 0.8))
    img[0, 0] = (0.0, 1.0, 0.0)       # not symmetric: a flipped or transposed read would show
    prt.write_pfm(pfm, img)
    assert np.array_equal(prt.read_pfm(pfm), img)
    W, H = 48, 36
    ply = scenes.asset("cube_uv.ply")
    p = subprocess.run([exe, "--ply", ply, "--width", str(W), "--height", str(H), "--spp", "3", "--depth", "4", "--seed", "7",
                        "--camera", "2.5", "2.0", "4.0", "--ground-texture", pfm, "--mesh-texture", pfm, "--texture-filter", filt,
                        "--out", out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    raw = open(out + ".pfm", "rb").read()
    hdr = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(hdr)
    got = np.frombuffer(raw[len(hdr):], "<f4").reshape(H, W, 3)[::-1]
    sc = scenes.mesh_scene(prt.Mesh(ply))                      # the scene the command line builds around a PLY
    t = sc.AddTexture(img, filt, "repeat")
    sc.SetMaterialTexture(0, t)
    sc.SetMaterialTexture(2, t)
    cam = prt.Camera((2.5, 2.0, 4.0), front=(-2.5, -2.0, -4.0), width=W, height=H)
    c = dict(scene=sc, cam=cam, W=W, H=H, depth=4)
    acc, wts, r = _frame(c, spp=3, sif=1)
    assert np.array_equal(got, acc / wts[..., None])
    assert f"{r.stats().rays_total} rays" in p.stdout
    plain, _, _ = _frame(dict(c, scene=scenes.mesh_scene(prt.Mesh(ply))), spp=3, sif=1)
    assert not np.array_equal(plain, acc)
