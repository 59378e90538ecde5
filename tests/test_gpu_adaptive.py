"""Film statistics and tile-adaptive sampling on the GPU (include/prt.h "Film statistics and adaptive sampling").  Every
comparison is bit for bit: the moments against the numpy restatement (tests/adaptive_replay.py) of one-sample frames, the
adaptive film, sample counts, ray totals and info against the replay of the oracle's frames, and, where no oracle exists,
every pixel against the uniform render of its own sample count.  The film is 44 x 28 (partial tiles on two edges, 24 tiles:
every tile list fits one wave) unless stated otherwise; the tests "on the wide film" run 444 x 348 (2464 tiles)."""
import concurrent.futures
import functools
import os
import subprocess

import numpy as np
import pytest

import adaptive_replay as ar
import util
from util import prt

pytestmark = pytest.mark.gpu

FX = ar.FIXTURE
W, H = FX["W"], FX["H"]
U32 = np.uint32


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(U32), np.ascontiguousarray(b, np.float32).view(U32))


def _renderer(scene, cam_pos=FX["cam_pos"], w=W, h=H, depth=FX["depth"], seed=FX["seed"], setup=None, pre=None, sif=None, stats=True,
              rank=0, world=1):
    film = prt.Film(w, h)
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=seed, rank=rank, world_size=world)
    if pre:
        pre(r)   # what has to be set before the scene (builders)
    r.Init(film, scene, prt.Camera(position=cam_pos, width=w, height=h))
    if setup:
        setup(r)
    if sif:
        r.set_samples_in_flight(sif)
    if stats:
        r.set_film_statistics(True)
    return r, film


def _one_sample_frames(r, film, n, first=0):
    """The context's own frames of samples first .. first + n - 1 (a cleared film plus one sample is that sample, exactly)."""
    frames = []
    for s in range(first, first + n):
        film.Clear()
        r.frame_index = s
        r.ProgressiveRender(1)
        r.download()
        frames.append(film.accum.copy())
    film.Clear()
    r.frame_index = 0
    return frames


@functools.lru_cache(maxsize=None)
def _bunny():
    return prt.scenes.mesh_scene(prt.Mesh(prt.scenes.asset("bunny.ply")))


BUNNY_CAM = (2.0, 1.5, 3.0)


# ---- 1. moments --------------------------------------------------------------------------------------------------------------
MOMENT_ROUTES = {
    "compact": dict(),
    "jitter": dict(setup=lambda r: r.set_sampling(jitter=1)),
    "mis": dict(setup=lambda r: r.set_lighting("mis")),
    "rank0of3": dict(rank=0, world=3), "rank1of3": dict(rank=1, world=3), "rank2of3": dict(rank=2, world=3),
}


@pytest.mark.parametrize("route", sorted(MOMENT_ROUTES))
def test_moments_equal_the_restatement(route):
    kw = MOMENT_ROUTES[route]
    spp = 12
    r, film = _renderer(_bunny(), BUNNY_CAM, depth=4, **kw)
    frames = _one_sample_frames(r, film, spp)
    A, Q = ar.moments(frames)
    r0, film0 = _renderer(_bunny(), BUNNY_CAM, depth=4, stats=False, **kw)
    r0.set_samples_in_flight(5)
    r0.ProgressiveRender(spp)
    r0.download()
    owned = film0.weights > 0
    assert owned.any() and (route.startswith("rank") or owned.all())
    for sif in (1, 5, 16):
        film.Clear()
        r.frame_index = 0
        r.set_samples_in_flight(sif)
        r.ProgressiveRender(spp)
        r.download()
        gA, gQ = r.film_statistics()
        assert _same(gA[owned], A[owned]) and _same(gQ[owned], Q[owned]), (route, sif)
        assert not gA[~owned].any() and not gQ[~owned].any()
        assert _same(film.accum, film0.accum) and _same(film.weights, film0.weights), (route, sif)   # statistics change no bit
        noise = r.noise_map(0.01)
        want = ar.noise_map(film.weights, A, Q, 0.01)
        assert np.array_equal(noise[owned].view(U32), want[owned].view(U32)) and np.isinf(noise[~owned]).all()
        if sif == 5:
            assert r.shade_instance() == r0.shade_instance() and r.kernel_instance() == r0.kernel_instance()
    if route in ("compact", "jitter"):   # lighting off: the oracle's frames give the same moments
        osc = util.oracle_scene(_bunny())
        cam = prt.Camera(position=BUNNY_CAM, width=W, height=H).desc()
        sp = prt.capi.PrtSampling(1, 0, 0.0) if route == "jitter" else None
        oframes = [osc.render(cam, W, H, spp=1, first_sample=s, max_depth=4, seed=FX["seed"], iterative=True, use_bvh=True,
                              n_threads=8, sampling=sp)[0] for s in range(spp)]
        oA, oQ = ar.moments(oframes)
        assert _same(oA, A) and _same(oQ, Q)
    if route == "compact":               # the default route of a mesh scene: compact primary rays and their shade instance
        assert r0.shade_instance().startswith("k_shade<")
    assert (Q > 0).any()


def test_switching_statistics_clears_the_film_and_read_back_needs_them():
    r, film = _renderer(prt.Scene("CORNELL"), stats=False)
    r.ProgressiveRender(2)
    with pytest.raises(prt.PrtError):
        r.film_statistics()
    r.set_film_statistics(True)
    r.download()
    assert not film.weights.any() and r.frame_index == 0
    r.ProgressiveRender(2)
    assert r.film_statistics()[0].any()
    r.set_film_statistics(True)          # no change: nothing happens
    r.download()
    assert (film.weights == 2).all()
    film.Clear()
    assert not r.film_statistics()[0].any()
    r.set_film_statistics(False)
    with pytest.raises(prt.PrtError):
        r.render_adaptive(0.1)


# ---- 2. adaptive against the replay of the oracle's frames -----------------------------------------------------------------------
def _oracle_scene_of(key):
    """(scene, oracle keywords) of a preset name or of a key of MESH_SCENES (the oracle walks a mesh through its BVH)."""
    if key in MESH_SCENES:
        return MESH_SCENES[key](), dict(use_bvh=True)
    return prt.Scene(key), dict()


@functools.lru_cache(maxsize=None)
def _oracle_frames(preset, cam_pos=FX["cam_pos"], w=W, h=H):
    scene, kw = _oracle_scene_of(preset)
    osc = util.oracle_scene(scene)
    cam = prt.Camera(position=cam_pos, width=w, height=h).desc()
    threads = 16 if w * h > 64 * 64 else 8

    @functools.lru_cache(maxsize=None)
    def frame(s):
        f = osc.render(cam, w, h, spp=1, first_sample=s, max_depth=FX["depth"], seed=FX["seed"], iterative=True, n_threads=threads, **kw)[0]
        f.setflags(write=False)
        return f

    return osc, cam, frame


def _oracle_rect_film(preset, ranges_per_tile, cam_pos=FX["cam_pos"], w=W, h=H):
    """The oracle's film of per-tile rect renders: for every tile each (first_sample, count) range in turn; and its rays."""
    osc, cam, _ = _oracle_frames(preset, cam_pos, w, h)
    kw = dict(use_bvh=True) if preset in MESH_SCENES else {}
    acc = np.zeros((h, w, 3), np.float32)
    wts = np.zeros((h, w), np.float32)

    def some(jobs):
        rays = 0
        for rect, ranges in jobs:
            for first, count in ranges:
                if count:
                    rays += osc.render(cam, w, h, spp=count, first_sample=first, max_depth=FX["depth"], seed=FX["seed"], iterative=True,
                                       n_threads=1, rect=rect, accum=acc, weights=wts, **kw)[2]
        return rays

    jobs = list(zip(ar.tiles(w, h), ranges_per_tile))
    if len(jobs) <= 64:
        rays = some(jobs)
    else:   # tiles are disjoint and a tile's ranges stay in order within one job, so threads change no bit
        workers = min(16, len(os.sched_getaffinity(0)))
        with concurrent.futures.ThreadPoolExecutor(workers) as pool:
            rays = sum(pool.map(some, [jobs[i::4 * workers] for i in range(4 * workers)]))
    return acc, wts, rays


def _check_against_the_replay(scene, want, rp, ref_film, cfg, sif, w=W, h=H):
    """One adaptive frame of `scene` against the replay `want` of the oracle's frames and the oracle's per-tile rect film."""
    thr, mn, step, mx, floor = cfg
    r, film = _renderer(scene, w=w, h=h, sif=sif)
    info = r.render_adaptive(thr, mn, step, mx, floor)
    r.download()
    assert np.array_equal(film.weights, rp.count_map(want["counts"]))
    acc, wts, rays = ref_film
    assert _same(film.accum, acc) and _same(film.weights, wts)
    st = r.stats()
    assert st.rays_total == rays
    assert st.rays_per_depth[0] == int(wts.sum()) and st.samples == mn
    assert ar.info_dict(info) == ar.replay_info(want)
    gA, gQ = r.film_statistics()
    assert _same(gA, rp.A) and _same(gQ, rp.Q)
    assert r.frame_index == mx
    return film


@pytest.mark.parametrize("preset", sorted(ar.FIXTURE_THRESHOLDS))
def test_adaptive_equals_the_replay(preset):
    thr = ar.FIXTURE_THRESHOLDS[preset]
    cfg = (thr, FX["min_spp"], FX["step_spp"], FX["max_spp"], FX["noise_floor"])
    rp = ar.Replay(W, H, _oracle_frames(preset)[2])
    want = rp.run(*cfg[1:4], thr, FX["noise_floor"])
    ref_film = _oracle_rect_film(preset, [[rg] for rg in want["ranges"]])
    _check_against_the_replay(prt.Scene(preset), want, rp, ref_film, cfg, 16)


# The same on 444 x 348 (adaptive_replay.FIXTURE_WIDE: 2464 tiles, 822 / 821 / 821 as three ranks): the tile lists take several
# trips of 1024 flags through k_tile_compact, with a carry and with ranks in every wave, and a listed batch has ~100 k compact
# pixels (tests/test_adaptive_replay.py asserts that the fixture's lists are that long, shrink and are ragged).
WIDE = ar.FIXTURE_WIDE
WW, WH = WIDE["W"], WIDE["H"]
WIDE_CFG = (WIDE["threshold"], WIDE["min_spp"], WIDE["step_spp"], WIDE["max_spp"], WIDE["noise_floor"])
MESH_WIDE_CFG = (0.2, 4, 4, 24, 0.01)
assert (WIDE["depth"], WIDE["seed"], WIDE["cam_pos"]) == (FX["depth"], FX["seed"], FX["cam_pos"])


@functools.lru_cache(maxsize=None)
def _wide_reference(key, cfg, ranks=1):
    """(replay, its result, the oracle's rect film) of a 444 x 348 frame; computed once, read only."""
    thr, mn, step, mx, floor = cfg
    rp = ar.Replay(WW, WH, _oracle_frames(key, FX["cam_pos"], WW, WH)[2])
    want = rp.run(mn, step, mx, thr, floor, ranks=ranks)
    ref_film = _oracle_rect_film(key, [[rg] for rg in want["ranges"]], FX["cam_pos"], WW, WH) if ranks == 1 else None
    return rp, want, ref_film


@pytest.mark.parametrize("sif", [16, 3])   # 3: a step of 4 samples is two listed batches, 3 + 1
def test_adaptive_equals_the_replay_on_the_wide_film(sif):
    rp, want, ref_film = _wide_reference(WIDE["preset"], WIDE_CFG)
    assert sum(1 for n_in, _ in want["selects"][0][1:] if n_in > 1024) >= 3   # (test_adaptive_replay.py holds the fixture to more)
    _check_against_the_replay(prt.Scene(WIDE["preset"]), want, rp, ref_film, WIDE_CFG, sif, WW, WH)


def test_adaptive_equals_the_replay_on_the_wide_film_of_a_mesh_scene():
    """RANDOM_BALLS_SMALL plus the bunny: the listed batches run the primitive BVH and the mesh tree at ~120 k compact pixels."""
    rp, want, ref_film = _wide_reference("balls_bunny", MESH_WIDE_CFG)
    sel = want["selects"][0]
    print("selects", [(n_in, len(kept)) for n_in, kept in sel], "runs", max(ar.runs(kept) for _, kept in sel))
    assert sum(1 for n_in, _ in sel[1:] if n_in > 1024) >= 3 and max(ar.runs(kept) for _, kept in sel) >= 100
    _check_against_the_replay(_balls_and_bunny(), want, rp, ref_film, MESH_WIDE_CFG, 16, WW, WH)


def _wide_frame(rank=0, world=1):
    r, film = _renderer(prt.Scene(WIDE["preset"]), w=WW, h=WH, sif=16, rank=rank, world=world)
    info = r.render_adaptive(*WIDE_CFG)
    r.download()
    return film, info


def test_three_ranks_of_the_wide_film():
    want3 = _wide_reference(WIDE["preset"], WIDE_CFG, 3)[1]
    one, info1 = _wide_frame()
    acc = np.zeros_like(one.accum)
    wts = np.zeros_like(one.weights)
    for rank in range(3):
        film, info = _wide_frame(rank, 3)
        assert ar.info_dict(info) == {k: int(want3["per_rank"][rank][k]) for k in ar.INFO_FIELDS}, rank
        assert not film.accum[film.weights == 0].any() and not wts[film.weights > 0].any()
        acc += film.accum
        wts += film.weights
    assert _same(acc, one.accum) and _same(wts, one.weights)
    assert ar.info_dict(info1) == ar.replay_info(want3)   # (the totals of the three loops are the one-rank loop's)
    # the same three ranks as a group on one device
    gfilm = prt.Film(WW, WH)
    g = prt.HipWavefrontGroupRenderer([0, 0, 0], max_depth=FX["depth"], seed=FX["seed"])
    g.Init(gfilm, prt.Scene(WIDE["preset"]), prt.Camera(position=FX["cam_pos"], width=WW, height=WH))
    g.set_samples_in_flight(16)
    g.set_film_statistics(True)
    ginfo = g.render_adaptive(*WIDE_CFG)
    g.download()
    assert _same(gfilm.accum, one.accum) and _same(gfilm.weights, one.weights)
    assert ar.info_dict(ginfo) == ar.replay_info(want3)


def test_tile_lists_regrow_with_the_film():
    """One renderer at 44 x 28, then 444 x 348, then 44 x 28 again: each frame is a fresh renderer's (the selection buffers of
    prt_render_adaptive are sized by the first call and regrown by the second)."""
    small_cfg = (ar.FIXTURE_THRESHOLDS["CORNELL"], FX["min_spp"], FX["step_spp"], FX["max_spp"], FX["noise_floor"])

    def frame(r, film):
        info = r.render_adaptive(*cfg)
        r.download()
        A, Q = r.film_statistics()
        return film.accum.copy(), film.weights.copy(), A, Q, ar.info_dict(info)

    r = None
    for w, h, cfg in ((W, H, small_cfg), (WW, WH, WIDE_CFG), (W, H, small_cfg)):
        fresh = frame(*_renderer(prt.Scene("CORNELL"), w=w, h=h, sif=16))
        if r is None:
            r, film = _renderer(prt.Scene("CORNELL"), w=w, h=h, sif=16)
        else:
            film = prt.Film(w, h)
            r.Init(film, prt.Scene("CORNELL"), prt.Camera(position=FX["cam_pos"], width=w, height=h))
        got = frame(r, film)
        assert all(_same(a, b) for a, b in zip(got[:4], fresh[:4])) and got[4] == fresh[4], (w, h)
        assert len(np.unique(got[1])) >= 3


# ---- 3. self-consistency where no oracle exists ----------------------------------------------------------------------------------
def _emissive_mesh_scene():
    sc = _bunny_scene_copy()
    glow = sc.AddEmissive((6.0, 5.0, 4.0))
    ico = prt.Mesh(prt.scenes.asset("icosahedron.ply"))
    mat, inv = prt.make_transform((0.3, 0.3, 0.3), (0, 0, 0), (1.2, 0.4, 0.6))
    sc.AddMesh(ico.transform(mat, inv), glow)
    return sc


def _bunny_scene_copy():
    return prt.scenes.mesh_scene(prt.Mesh(prt.scenes.asset("bunny.ply")))


def _textured_scene():
    mesh = prt.Mesh(prt.scenes.asset("bunny.ply"))
    mesh.SetUVs(prt.scenes.planar_uvs(mesh))
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.5, 0.5, 0.5))
    light = sc.AddEmissive((15.0, 15.0, 15.0))
    body = sc.AddLambertian((0.8, 0.8, 0.8))
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    sc.AddMesh(mesh, body)
    sc.SetMaterialTexture(body, sc.AddTexture(prt.scenes.checker(8), filter="bilinear"))
    sc.SetMaterialTexture(ground, sc.AddTexture(prt.scenes.checker(4, (0.9, 0.6, 0.3), (0.2, 0.2, 0.4))))
    return sc


def _placed_scene():
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.5, 0.5, 0.5))
    light = sc.AddEmissive((15.0, 15.0, 15.0))
    body = sc.AddLambertian((0.8, 0.7, 0.6))
    glass = sc.AddDielectric(1.5)
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    ico = prt.Mesh(prt.scenes.asset("icosahedron.ply")).refine(300)
    sc.AddInstance(ico, body, scale=0.8, euler_deg=(10.0, 25.0, 0.0), translation=(-0.9, 0.0, 0.0))
    sc.AddInstance(ico, glass, scale=0.6, euler_deg=(0.0, 50.0, 20.0), translation=(0.9, -0.2, 0.6))
    return sc


def _balls_and_bunny():
    sc = prt.Scene("RANDOM_BALLS_SMALL")   # more than 16 analytic primitives: the primitive BVH and its kernel instances
    sc.AddMesh(prt.Mesh(prt.scenes.asset("bunny.ply")), sc.AddLambertian((0.8, 0.8, 0.8)))
    return sc


MESH_SCENES = {"balls_bunny": _balls_and_bunny}   # oracle scene keys that are not presets


def _env_image():
    rng = np.random.default_rng(5)
    img = rng.uniform(0.05, 0.6, (8, 16, 3)).astype(np.float32)
    img[2, 5] = (30.0, 28.0, 20.0)
    return img


SELF_CASES = {
    "mis_mesh_lights": dict(scene=_emissive_mesh_scene, cam=BUNNY_CAM, lit=True,
                            setup=lambda r: (r.set_light_sources("all"), r.set_lighting("mis"))),
    "environment_nee": dict(scene=_bunny_scene_copy, cam=BUNNY_CAM, lit=True,
                            setup=lambda r: (r.set_environment(_env_image()), r.set_lighting("nee"))),
    "environment": dict(scene=_bunny_scene_copy, cam=BUNNY_CAM, setup=lambda r: r.set_environment(_env_image())),
    "textures_lens": dict(scene=_textured_scene, cam=BUNNY_CAM, setup=lambda r: r.set_lens(0.0, 0.06, 3.6)),
    "jitter_rr_clamp": dict(scene=_bunny_scene_copy, cam=BUNNY_CAM, setup=lambda r: r.set_sampling(jitter=1, rr_depth=2, clamp=4.0)),
    "placed_copies": dict(scene=_placed_scene, cam=(1.5, 1.5, 4.0)),
    "balls_bunny_prim_bvh": dict(scene=_balls_and_bunny, cam=FX["cam_pos"]),
}


def _check_every_pixel_against_uniform_renders(case, w=W, h=H):
    cs = SELF_CASES[case]
    scene = cs["scene"]()
    r, film = _renderer(scene, cs["cam"], w, h, depth=4, setup=cs.get("setup"), sif=4)
    info = r.render_adaptive(0.12, 4, 4, 16, 0.01)
    r.download()
    acc, wts = film.accum.copy(), film.weights.copy()
    st = r.stats()
    counts = sorted(set(int(v) for v in np.unique(wts)))
    print(case, "counts", {n: int((wts == n).sum()) for n in counts}, ar.info_dict(info))
    assert set(counts) <= {4, 8, 12, 16} and len(counts) >= 2          # (a frame with one count would test nothing)
    assert info.pixel_samples == int(wts.sum()) == st.rays_per_depth[0] and st.samples == 4
    for x0, y0, x1, y1 in ar.tiles(w, h):                               # whole tiles share a count
        assert (wts[y0:y1, x0:x1] == wts[y0, x0]).all()
    if cs.get("lit"):
        assert r.light_stats().shadow_rays > 0
    r.set_film_statistics(False)   # the uniform renders run the routes they always ran
    for n in counts:
        film.Clear()
        r.frame_index = 0
        r.ProgressiveRender(n)
        r.download()
        at = wts == n
        assert _same(film.accum[at], acc[at]), (case, n)
    return wts, info


@pytest.mark.parametrize("case", sorted(SELF_CASES))
def test_every_pixel_equals_the_uniform_render_of_its_count(case):
    _check_every_pixel_against_uniform_renders(case)


def test_every_pixel_equals_the_uniform_render_of_its_count_on_the_wide_film():
    """mis_mesh_lights at 444 x 348: a lit route (shadow rays, the lit accumulation) through listed batches of ~100 k compact
    pixels, from lists that span trips of 1024 flags: more than 1024 tiles are still active after the first select, so the
    second one reads a list of that length."""
    wts, info = _check_every_pixel_against_uniform_renders("mis_mesh_lights", WW, WH)
    beyond_min = sum(1 for x0, y0, x1, y1 in ar.tiles(WW, WH) if wts[y0, x0] > 4)
    assert info.tiles_local == 2464 and info.passes >= 2 and beyond_min > 1024


# ---- 4. invariance ---------------------------------------------------------------------------------------------------------------
INV_CFG = (0.12, 4, 4, 16, 0.01)


def _inv_frame(setup=None, pre=None, sif=4, rank=0, world=1):
    r, film = _renderer(_balls_and_bunny(), depth=4, setup=setup, pre=pre, sif=sif, rank=rank, world=world)
    info = r.render_adaptive(*INV_CFG)
    r.download()
    return film.accum.copy(), film.weights.copy(), ar.info_dict(info), [int(v) for v in r.stats().rays_per_depth]


@pytest.fixture(scope="module")
def inv_base():
    return _inv_frame()


INV_VARIANTS = {
    "sif1": dict(sif=1), "sif3": dict(sif=3), "sif64": dict(sif=64),
    "prim_bvh0": dict(pre=lambda r: r.set_param("prim_bvh", 0)),
    "exact_grids2": dict(setup=lambda r: r.set_param("exact_grids", 2)),
    "gpu_build1": dict(pre=lambda r: r.set_param("gpu_build", 1)),
    "gpu_build2": dict(pre=lambda r: r.set_param("gpu_build", 2)),
    "path_kernel2_compact0": dict(setup=lambda r: (r.set_param("path_kernel", 2), r.set_param("compact_primary", 0))),
}


@pytest.mark.parametrize("variant", sorted(INV_VARIANTS))
def test_adaptive_frame_does_not_depend_on_a_tunable(inv_base, variant):
    acc, wts, info, rays = _inv_frame(**INV_VARIANTS[variant])
    assert _same(acc, inv_base[0]) and _same(wts, inv_base[1]) and info == inv_base[2] and rays == inv_base[3]
    assert len(np.unique(inv_base[1])) >= 2


def test_three_ranks_assemble_to_the_one_rank_frame(inv_base):
    acc = np.zeros_like(inv_base[0])
    wts = np.zeros_like(inv_base[1])
    rays = np.zeros(len(inv_base[3]), np.int64)
    tiles = conv = capped = samples = 0
    for rank in range(3):
        a, w, info, per_depth = _inv_frame(rank=rank, world=3)
        assert not a[w == 0].any() and not (wts[w > 0]).any()
        acc += a
        wts += w
        rays += np.array(per_depth)
        tiles += info["tiles_local"]
        conv += info["tiles_converged"]
        capped += info["tiles_capped"]
        samples += info["pixel_samples"]
    assert _same(acc, inv_base[0]) and _same(wts, inv_base[1]) and rays.tolist() == inv_base[3]
    b = inv_base[2]
    assert (tiles, conv, capped, samples) == (b["tiles_local"], b["tiles_converged"], b["tiles_capped"], b["pixel_samples"])


def test_group_of_one_device_listed_three_times(inv_base):
    film = prt.Film(W, H)
    g = prt.HipWavefrontGroupRenderer([0, 0, 0], max_depth=4, seed=FX["seed"])
    g.Init(film, _balls_and_bunny(), prt.Camera(position=FX["cam_pos"], width=W, height=H))
    g.set_samples_in_flight(4)
    g.set_film_statistics(True)
    info = g.render_adaptive(*INV_CFG)
    g.download()
    assert _same(film.accum, inv_base[0]) and _same(film.weights, inv_base[1])
    got, b = ar.info_dict(info), inv_base[2]
    for k in ("tiles_local", "tiles_converged", "tiles_capped", "pixel_samples", "min_tile_spp", "max_tile_spp"):
        assert got[k] == b[k], k
    assert got["passes"] <= b["passes"]
    # the single-context read-backs, assembled from the ranks that own the tiles
    r, f1 = _renderer(_balls_and_bunny(), depth=4, sif=4)
    r.render_adaptive(*INV_CFG)
    A, Q = r.film_statistics()
    gA, gQ = g.film_statistics()
    assert _same(gA, A) and _same(gQ, Q)
    assert np.array_equal(g.noise_map(0.01).view(U32), r.noise_map(0.01).view(U32))


def test_command_line(tmp_path):
    """prt_render --adaptive on the CORNELL fixture: --samples-out is the replay's count map, the mean image the library's."""
    exe = os.path.join(util.ROOT, "parallelraytracing_amd", "csrc", "prt_render")
    out, samples, noise = (str(tmp_path / n) for n in ("frame", "samples.pfm", "noise.pfm"))
    p = subprocess.run([exe, "--preset", "CORNELL", "--width", str(W), "--height", str(H), "--depth", str(FX["depth"]), "--seed", str(FX["seed"]),
                        "--camera", "5", "5", "8", "--adaptive", "0.10", "--min-spp", "8", "--spp-step", "8", "--max-spp", "96",
                        "--noise-floor", "0.01", "--sif", "16", "--samples-out", samples, "--noise-out", noise, "--out", out],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "11 passes" in p.stdout and "15 at the cap" in p.stdout
    rp = ar.Replay(W, H, _oracle_frames("CORNELL")[2])
    want = rp.run(FX["min_spp"], FX["step_spp"], FX["max_spp"], 0.10, FX["noise_floor"])
    got = prt.read_pfm(samples)
    assert np.array_equal(got[..., 0], rp.count_map(want["counts"])) and np.array_equal(got[..., 0], got[..., 2])
    mean = prt.read_pfm(out + ".pfm")
    assert _same(mean, rp.accum / rp.n[..., None])
    assert np.array_equal(prt.read_pfm(noise)[..., 1].view(U32), ar.noise_map(rp.n, rp.A, rp.Q, 0.01).view(U32))


# ---- 5. edges ----------------------------------------------------------------------------------------------------------------------
INSIDE_CAM = (0.0, 1.0, 3.0)   # inside the box: every tile sees surfaces, none is constant


def _edge(cfg, cam_pos=FX["cam_pos"], w=W, h=H, first=None, r_film=None, preset="CORNELL"):
    r, film = r_film or _renderer(prt.Scene(preset), cam_pos, w, h, sif=8)
    info = r.render_adaptive(*cfg, first_sample=first)
    r.download()
    return r, film, info


def _edge_replay(cfg, cam_pos=FX["cam_pos"], w=W, h=H, preset="CORNELL"):
    thr, mn, step, mx, floor = cfg
    rp = ar.Replay(w, h, _oracle_frames(preset, cam_pos, w, h)[2])
    return rp, rp.run(mn, step, mx, thr, floor)


def _check_edge(cfg, cam_pos=FX["cam_pos"], w=W, h=H, preset="CORNELL"):
    rp, want = _edge_replay(cfg, cam_pos, w, h, preset)
    r, film, info = _edge(cfg, cam_pos, w, h, preset=preset)
    assert np.array_equal(film.weights, rp.count_map(want["counts"])) and _same(film.accum, rp.accum)
    assert ar.info_dict(info) == ar.replay_info(want)
    return want, film, info


def test_threshold_zero_takes_every_tile_to_the_cap():
    """(lhs > 0 needs variance: a tile of identical samples stops at once whatever the threshold, so the camera stands where
    every tile sees lit surfaces.)"""
    want, film, info = _check_edge((0.0, 8, 8, 24, 0.01), INSIDE_CAM)
    assert (film.weights == 24).all() and info.tiles_capped == 24 and info.tiles_converged == 0 and info.passes == 2


def test_huge_threshold_stops_every_tile_at_min():
    want, film, info = _check_edge((1e9, 8, 8, 24, 0.01))
    assert (film.weights == 8).all() and info.passes == 0 and info.tiles_converged == 24 and info.pixel_samples == 8 * W * H


def test_max_equal_to_min():
    want, film, info = _check_edge((0.1, 8, 0, 8, 0.01))
    assert (film.weights == 8).all() and info.passes == 0 and info.tiles_capped + info.tiles_converged == 24 and info.tiles_capped > 0


def test_last_step_is_cut_at_the_cap():
    want, film, info = _check_edge((0.1, 8, 8, 20, 0.01))
    assert sorted(np.unique(film.weights).tolist()) == [8.0, 16.0, 20.0]


def test_one_active_tile_and_all_tiles_active():
    """An 8 x 8 film is one tile: its passes have exactly ONE active tile (64 paths per sample).  A 1 x 1 film is one tile
    with one pixel inside the image (DEFAULT: CORNELL's centre pixel has no variance and stops at once).  The first pass of
    the inside camera has all 24 tiles active."""
    want, film, info = _check_edge((0.0, 4, 4, 12, 0.01), INSIDE_CAM, 8, 8)
    assert info.tiles_local == 1 and info.passes == 2 and (film.weights == 12).all()
    want, film, info = _check_edge((0.0, 4, 4, 12, 0.01), FX["cam_pos"], 1, 1, preset="DEFAULT")
    assert info.tiles_local == 1 and info.passes == 2 and info.pixel_samples == 12 and film.weights[0, 0] == 12
    want, film, info = _check_edge((0.0, 4, 4, 8, 0.01), INSIDE_CAM)
    assert info.passes == 1 and info.pixel_samples == 8 * W * H


def test_continuing_a_finished_frame_uses_no_index_twice():
    thr = ar.FIXTURE_THRESHOLDS["CORNELL"]
    cfg = (thr, FX["min_spp"], FX["step_spp"], FX["max_spp"], FX["noise_floor"])
    rp, first = _edge_replay(cfg)
    more = rp.run(0, 8, 16, thr, FX["noise_floor"], first_sample=96)
    r, film, _ = _edge(cfg)
    st0 = r.stats()
    r, film, info = _edge((thr, 0, 8, 16, FX["noise_floor"]), first=96, r_film=(r, film))
    assert np.array_equal(film.weights, rp.n) and film.weights.max() == 112
    acc, wts, rays = _oracle_rect_film("CORNELL", [[a, b] for a, b in zip(first["ranges"], more["ranges"])])
    assert _same(film.accum, acc) and _same(film.weights, wts)
    st = r.stats()
    assert st.rays_total == rays and st.samples == st0.samples == FX["min_spp"]
    assert ar.info_dict(info) == ar.replay_info(more) and info.min_tile_spp == 0 and info.max_tile_spp == 16
    assert (more["counts"][first["counts"] < 96] == 0).all()
