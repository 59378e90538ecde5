"""Triangle lights (include/prt.h "Triangle lights", prt_set_light_sources) on one MI355X.  Time budget: about 60 s, most
of it the float64 law quadrature and the replay on the CPU (measured: 13 tests in 18 s of wall time); the emissive dragon (about
870 k lights, 480 x 270) is a few seconds of scene build.

  * Default mask: light-sampled frames of D_tri and of an emissive placed copy stay bit-identical to lighting off.
  * D_tri with "all", 1080p x 64 spp: a triangulated rectangle with uniform emission is sampled uniformly over the rectangle
    (pmf_i pdf_i = d2 / (A_rect |n.w|)), so the frame follows the float64 law of kind D (tests/lighting_laws.py), which
    knows nothing of triangles; rays_per_depth equal lighting off's; one shadow ray per scattering ground vertex, none
    occluded; variance against lighting off better than 10x.
  * prt_sample_light against the float64 restatement (tests/mesh_light_replay.py) for triangles of a world-space mesh and of a
    rotated, scaled placed copy.
  * Every sample of the replayed cases within its tolerance; other routes bit-identical to the first.
  * Emissive bunny: off, mis and nee agree in mean.  Emissive dragon: renders, no error flag, agrees with lighting off.
  * Refit and the group (which need a device): the light set after Refit equals a fresh scene's; a group reports one set."""
import time

import numpy as np
import pytest

import closed_form as cf
import lighting_laws as ll
import mesh_light_replay as mr
from parallelraytracing_amd import scenes
from util import orc, prt

pytestmark = pytest.mark.gpu

SEED = 11


def _render(scene, cam, W, H, spp, max_depth, mode="off", sources=None, sif=16, params=(), sampling=None, seed=SEED):
    film = prt.Film(W, H)
    r = prt.HipWavefrontRenderer(device=0, max_depth=max_depth, seed=seed)
    for k, v in params:
        r.set_param(k, v)
    if sources is not None:
        r.set_light_sources(sources)
    r.Init(film, scene, cam)
    r.set_samples_in_flight(sif)
    r.set_lighting(mode)
    if sampling is not None:
        r.set_sampling(*sampling)
    r.reset_stats()
    r.ProgressiveRender(spp)
    r.download()
    r.synchronize()
    rays = np.array(r.stats().rays_per_depth[:max_depth], np.uint64)
    return r, film.accum.copy(), film.weights.copy(), rays, r.light_stats()


def _placed_copy_scene():
    sc = prt.Scene(preset=None, sky=cf.SKY)
    g = sc.AddLambertian(cf.GROUND_ALBEDO)
    e = sc.AddEmissive(cf.EMISSION)
    sc.AddQuad(20.0, 20.0, g, translation=(0.0, -1.0, 0.0))
    sc.AddInstance(prt.Mesh(scenes.asset("icosahedron.ply")), e, translation=(0.0, 5.0, 0.0))
    return sc


@pytest.mark.parametrize("case", ["D_tri", "placed"])
def test_default_mask_is_still_bit_identical_to_lighting_off(case):
    W, H, S, D = 320, 240, 16, 5
    if case == "D_tri":
        sc = scenes.triangulate_quads(cf.ground_scene(prt)[0])
        cam = cf.camera(prt, "ground", W, H)
    else:
        sc = _placed_copy_scene()
        cam = prt.Camera((0.0, 3.0, 8.0), front=prt.glm_normalize(np.array([0.0, 0.0, -1.0], np.float32)), width=W, height=H)
    _, a0, w0, r0, _ = _render(sc, cam, W, H, S, D, "off")
    for sources in (None, "analytic"):
        _, a1, w1, r1, ls = _render(sc, cam, W, H, S, D, "mis", sources=sources)
        assert ls.n_lights == 0 and ls.shadow_rays == 0
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(w0, w1) and np.array_equal(r0, r1)
    # and the new mask does sample them
    _, a2, _, r2, ls = _render(sc, cam, W, H, S, D, "mis", sources="all")
    assert ls.n_lights in (8, 20) and ls.shadow_rays > 0 and np.array_equal(r0, r2)
    assert not np.array_equal(a0, a2)


@pytest.mark.parametrize("sampling", [(0, 0, 0.0), (0, 1, 1.0)])
def test_d_tri_frames_follow_the_float64_law_of_kind_d(record_property, sampling):
    W, H, S, D = 1920, 1080, 64, 5
    cam = cf.camera(prt, "ground", W, H)
    base, ground, emitter = cf.ground_scene(prt)
    sc = scenes.triangulate_quads(base)
    light = ("quad", emitter[0], emitter[1], emitter[2])
    sub = (np.arange(H)[::4, None] * W + np.arange(W)[None, ::4]).ravel()
    r, a_off, _, r_off, _ = _render(sc, cam, W, H, S, D, "off", sampling=sampling)
    o, d = cf.pixel_rays(r.camera_rays, W, H)
    del r
    for mode in ("mis", "nee"):
        law = ll.frame_law(o[sub], d[sub], ground, light, mode, cf.GROUND_ALBEDO, cf.EMISSION, cf.SKY, rr=sampling[1],
                           clamp=sampling[2], max_depth=D)
        _, a, w, rays, ls = _render(sc, cam, W, H, S, D, mode, sources="all", sampling=sampling)
        st = ll.frame_stats(a.reshape(-1, 3)[sub], w.reshape(-1)[sub], S, law, W // 4, H // 4)
        # noise against lighting off, on the law's ground pixels
        g = law["on_g"] & ~law["excluded"]
        X1 = a.reshape(-1, 3)[sub].astype(np.float64).sum(1) / S
        X0 = a_off.reshape(-1, 3)[sub].astype(np.float64).sum(1) / S
        var_ratio = float(((X0[g] - law["mu"][g]) ** 2).mean() / ((X1[g] - law["mu"][g]) ** 2).mean())
        rec = {f"D_tri_{mode}_rr{sampling[1]}_c{sampling[2]}": st, "var_ratio": round(var_ratio, 1), "shadow": int(ls.shadow_rays)}
        record_property("mesh_light_law", rec)
        print(rec, flush=True)
        assert ls.n_lights == 8 and ls.n_emitters_unsampled == 0
        assert np.array_equal(r_off, rays), (mode, r_off, rays)          # the scattered path is draw for draw lighting off's
        if sampling[1] == 0:
            assert ls.shadow_rays == rays[1], (ls.shadow_rays, rays)     # one shadow ray per scattering ground vertex
        assert ls.shadow_rays > 0 and ls.shadow_occluded == 0, (ls.shadow_rays, ls.shadow_occluded)
        assert st["excluded"] <= cf.MAX_EXCLUDED * len(sub), st
        assert ll.passes(st), st
        if sampling == (0, 0, 0.0):
            assert var_ratio > 10.0, rec


def _sample_scene():
    sc = prt.Scene(preset=None, sky=cf.SKY)
    g = sc.AddLambertian(cf.GROUND_ALBEDO)
    e = sc.AddEmissive(cf.EMISSION)
    e2 = sc.AddEmissive((2.0, 3.0, 4.0))
    sc.AddQuad(20.0, 20.0, g, translation=(0.0, -1.0, 0.0))
    sc.AddCircle(0.5, e2, scale=(2.0, 2.0, 2.0), translation=(3.0, 3.0, 1.0))
    ico = prt.Mesh(scenes.asset("icosahedron.ply"))
    up = ico.copy()
    mat, inv = scenes.make_transform((1, 1, 1), (0, 0, 0), (-2.0, 4.0, 0.5))
    up.transform(mat, inv)
    sc.AddMesh(up, e)                                                                                  # world-space mesh
    sc.AddInstance(ico, e2, scale=1.7, euler_deg=(25.0, 40.0, 10.0), translation=(1.0, 5.0, -1.0))   # rotated, scaled copy
    return sc


def test_sample_light_matches_float64_for_triangles():
    sc = _sample_scene()
    W, H = 64, 48
    r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=SEED)
    r.set_light_sources("all")
    r.Init(prt.Film(W, H), sc, cf.camera(prt, "ground", W, H))
    lights = mr.MeshLightSet(sc, "all")
    prim, pmf = r.light_info()
    assert np.array_equal(prim.astype(np.int64), lights.prim) and lights.n == 41
    assert np.all(np.abs(r.light_intervals().astype(np.float64) - lights.width) <= 2.0)
    rng = np.random.default_rng(5)
    n = 20000
    o = np.column_stack([rng.uniform(-8, 8, n), np.full(n, 1.5), rng.uniform(-8, 8, n)]).astype(np.float32)
    d = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (n, 1))
    hits = r.closest_hit(o, d)
    assert np.all(hits["prim"] == 0)
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for mode in ("mis", "nee"):
        r.set_lighting(mode)
        out = r.sample_light(d, hits, keys)
        x = hits["position"].astype(np.float64)
        nrm = hits["normal"].astype(np.float64)
        s = mr.sample_lights(lights, x, nrm, keys, mode)
        ok = ~s["sel_band"] & s["valid"]
        assert ok.sum() > 0.99 * n
        assert np.array_equal(out["light"][ok], s["light"][ok].astype(np.uint32))
        kind = lights.kind[s["light"]]
        world = ok & (kind == 2) & (lights.prim[s["light"]] < 2 + 20)
        placed = ok & (kind == 2) & (lights.prim[s["light"]] >= 2 + 20)
        assert world.sum() > 1000 and placed.sum() > 1000 and (ok & (kind == 0)).sum() > 100
        alb = np.asarray(cf.GROUND_ALBEDO, np.float32).astype(np.float64)
        contrib = alb * lights.Le[s["light"]] * s["f"][:, None]
        tri = ok & (kind == 2)
        np.testing.assert_allclose(out["dir"][ok], s["w"][ok], atol=2e-6)
        np.testing.assert_allclose(out["tmax"][tri], s["tmax"][tri], rtol=2e-6)
        np.testing.assert_allclose(out["tmax"][ok], s["tmax"][ok], rtol=1e-5)
        # test_sample_light_matches_float64's tolerances, plus the replay's conditioning term where a quantity divides by the
        # light's cosine: that test's quad faces the ground (|n_l.w| of order 1); an icosahedron's faces are also seen edge-on,
        # and fp32 carries |n_g.w| to about 8 * 2^-24 absolute (lighting_replay: c = 8 U / min cos; below COS_MIN the sample
        # is left out there, and here)
        ok = ok & (s["cos_l"] >= mr.COS_MIN)
        c = 8.0 * mr.U / np.maximum(s["cos_l"], mr.COS_MIN)

        def close(got, want, rtol, atol=0.0, sel=ok):
            err = np.abs(got[sel].astype(np.float64) - want[sel])
            lim = atol + (rtol + c[sel]).reshape((-1,) + (1,) * (want.ndim - 1)) * np.abs(want[sel])
            assert np.all(err <= lim), float((err / np.maximum(lim, 1e-300)).max())

        close(out["pdf_light"], s["pdf_l"], 1e-5)
        np.testing.assert_allclose(out["pdf_bsdf"][ok], s["pb"][ok], rtol=1e-5, atol=1e-7)
        close(out["w_light"], s["wl"], 1e-5, 1e-6)
        close(out["contrib"], contrib, 1e-5, 1e-6)
        pb, pl = s["pb"], s["pdf_l"]
        both = ok & (pb > 0) & (pl > 0)
        wb = mr.hit_weight(lights, lights.prim[s["light"]], x, s["w"], s["t_light"] ** 2, pb, mode)[0]
        if mode == "mis":
            np.testing.assert_allclose(out["w_light"][both] + out["w_bsdf"][both], 1.0, atol=2e-6)
            close(out["w_bsdf"], wb, 1e-4, 1e-6, sel=both)
        else:
            assert np.all(out["w_bsdf"][both] == 0.0) and np.all(out["w_light"][both] == 1.0)
            assert np.all(wb[both] == 0.0)


def _renderer(c, mode, sif=16, group=False, params=()):
    film = prt.Film(c["W"], c["H"])
    if group:
        r = prt.HipWavefrontGroupRenderer([0, 0, 0], max_depth=c["depth"], seed=mr.SEED)
    else:
        r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=mr.SEED)
    for k, v in params:
        r.set_param(k, v)
    r.set_light_sources("all")
    r.Init(film, c["scene"], c["cam"])
    r.set_samples_in_flight(sif)
    r.set_lighting(mode)
    return r, film


@pytest.mark.parametrize("name", mr.CASES)
def test_every_sample_matches_the_float64_replay(record_property, name):
    c = mr.case(name)
    osc = orc.OracleScene(c["scene"].desc())
    for mode in ("mis", "nee"):
        t0 = time.time()
        rep = mr.replay_case(c, mode, osc=osc)
        t1 = time.time()
        r, film = _renderer(c, mode)
        r.reset_stats()
        frames = mr.render_samples(r, film, mr.SAMPLES)
        r.synchronize()
        t2 = time.time()
        rec = mr.check_gpu(rep, frames, r.light_stats(), r.light_info(), r.light_intervals())
        rec.update(case=name, mode=mode, cpu_s=round(t1 - t0, 2), gpu_s=round(t2 - t1, 2))
        record_property("mesh_light_replay", rec)
        assert rec["compared"] >= 0.995 * len(rep.pix)
        assert rec["triangle_samples"] > 1000
        del r


def test_other_routes_are_bit_identical():
    """placed (two-level tree, the INST instances): device-built trees, 1 and 64 samples in flight, plain binary search, three
    ranks of a group; balls + an emissive mesh (the primitive-BVH instances): with and without the primitive BVH."""
    c = mr.case("placed")
    r, film = _renderer(c, "mis")
    ref = mr.render_samples(r, film, mr.SAMPLES)
    info = r.light_info()
    del r
    for kw in (dict(params=(("gpu_build", 1),)), dict(sif=1), dict(sif=64), dict(params=(("light_buckets", 0),))):
        r, film = _renderer(c, "mis", **kw)
        got = mr.render_samples(r, film, mr.SAMPLES)
        for s in mr.SAMPLES:
            assert np.array_equal(got[s].view(np.uint32), ref[s].view(np.uint32)), (kw, s)
        del r
    g, film = _renderer(c, "mis", group=True)
    got = mr.render_samples(g, film, mr.SAMPLES, clear=g.Clear)
    for s in mr.SAMPLES:
        assert np.array_equal(got[s].view(np.uint32), ref[s].view(np.uint32)), ("group", s)
    ginfo = g.light_info()
    assert np.array_equal(ginfo[0], info[0]) and np.array_equal(ginfo[1], info[1]) and g.light_stats().n_lights == len(info[0])
    del g
    sc = prt.Scene("RANDOM_BALLS_SMALL")
    e = sc.AddEmissive((3.0, 2.0, 1.0))
    ico = prt.Mesh(scenes.asset("icosahedron.ply")).copy()
    mat, inv = scenes.make_transform((1, 1, 1), (0, 0, 0), (0.0, 3.0, 0.0))
    ico.transform(mat, inv)
    sc.AddMesh(ico, e)
    cb = dict(scene=sc, cam=prt.Camera(width=320, height=240), W=320, H=240, depth=5)
    frames = []
    for pb in (1, 0):
        r, film = _renderer(cb, "mis", params=(("prim_bvh", pb),))
        frames.append(mr.render_samples(r, film, (0, 1)))
        assert r.light_stats().n_lights == 8 + 20 and r.light_stats().shadow_rays > 0
        del r
    for s in (0, 1):
        assert np.array_equal(frames[0][s].view(np.uint32), frames[1][s].view(np.uint32)), s


def _agree(X, W, pairs=(("mis", "nee"), ("mis", "off"), ("nee", "off")), label=""):
    """The statistic of test_gpu_lighting.test_several_lights_mis_nee_and_off_agree (same bounds): frame Z of the per-pixel
    differences with variances from a second seed, and 8x8-tile Z with the two modes taken from different seeds."""
    for m1, m2 in pairs:
        d1, d2 = X[m1, 0] - X[m2, 0], X[m1, 1] - X[m2, 1]
        var = (d1 - d2) ** 2 / 2.0
        keep = var > 0
        Z = d1[keep].sum() / np.sqrt(var[keep].sum())
        e1 = X[m1, 0] - X[m2, 1]
        ve = ((X[m1, 0] - X[m1, 1]) ** 2 + (X[m2, 0] - X[m2, 1]) ** 2) / 2.0
        kt = ve > 0
        pix = np.nonzero(kt)[0]
        tile = (pix // W // 8) * ((W + 7) // 8) + (pix % W) // 8
        num, den, cnt = np.bincount(tile, e1[kt]), np.bincount(tile, ve[kt]), np.bincount(tile)
        ok = cnt >= 32
        tileZ = float(np.abs(num[ok] / np.sqrt(den[ok])).max()) if ok.any() else 0.0
        print(dict(case=label, pair=(m1, m2), Z=round(float(Z), 2), tileZ=round(tileZ, 2), tiles=int(ok.sum())), flush=True)
        assert abs(Z) <= 6.0, (label, m1, m2, Z)
        assert tileZ <= 6.0, (label, m1, m2, tileZ)


def test_emissive_bunny_mis_nee_and_off_agree():
    W, H, S, D = 320, 240, 64, 5
    c = mr.case("bunny_light", W, H)
    X = {}
    for mode in ("off", "mis", "nee"):
        for k, seed in enumerate((SEED, SEED + 500)):
            _, a, _, _, ls = _render(c["scene"], c["cam"], W, H, S, D, mode, sources="all", sif=64, seed=seed)
            X[mode, k] = a.reshape(-1, 3).astype(np.float64).sum(1) / S
            if mode != "off":
                assert ls.n_lights > 9000 and ls.shadow_rays > 0 and ls.shadow_occluded > 0
    _agree(X, W, label="bunny_light")


def test_emissive_dragon_renders_and_agrees_with_lighting_off():
    """C3's dragon made emissive (about 870 k triangle lights beside the quad), 480 x 270."""
    W, H, S, D = 480, 270, 16, 5
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.5, 0.5, 0.5))
    light = sc.AddEmissive((15.0, 15.0, 15.0))
    glow = sc.AddEmissive((1.0, 0.8, 0.6))
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    mesh = scenes.refined("dragon.ply", 870_000)
    sc.AddMesh(mesh, glow)
    cam = prt.Camera(scenes.MESH_CAMERA, width=W, height=H)
    want = mr.MeshLightSet(sc, "all")
    X = {}
    for mode in ("off", "mis"):
        for k, seed in enumerate((SEED, SEED + 500)):
            r, a, w, rays, ls = _render(sc, cam, W, H, S, D, mode, sources="all", sif=16, seed=seed)
            r.synchronize()                                       # raises on the kernels' error flag
            assert np.all(np.isfinite(a)) and np.all(w == S)
            X[mode, k] = a.reshape(-1, 3).astype(np.float64).sum(1) / S
            if mode == "mis" and k == 0:
                print(dict(n_lights=int(ls.n_lights), triangles=mesh.n_triangles, unsampled=int(ls.n_emitters_unsampled),
                           shadow=int(ls.shadow_rays), occluded=int(ls.shadow_occluded)), flush=True)
                assert ls.n_lights == want.n and ls.n_lights > 0.9 * mesh.n_triangles
                assert ls.n_emitters_unsampled == want.n_unsampled_power
                assert ls.shadow_rays > 0 and 0 < ls.shadow_occluded < ls.shadow_rays
                prim, _ = r.light_info()
                assert np.array_equal(prim.astype(np.int64), want.prim)
            del r
    _agree(X, W, pairs=(("mis", "off"),), label="dragon_light")


def test_refit_rebuilds_the_light_set():
    base = scenes.refined("bunny.ply", 12_000)
    v = base.GetVertices().copy()
    v[:, 0] += 0.03 * np.sin(3.0 * v[:, 1])
    v *= np.float32(1.1)
    moved = prt.Mesh(vertices=v, normals=base.GetNormals(), indices=base.GetIndices())

    def scene(mesh):
        sc = prt.Scene(preset=None, sky=cf.SKY)
        g = sc.AddLambertian(cf.GROUND_ALBEDO)
        e = sc.AddEmissive((4.0, 3.0, 2.0))
        e2 = sc.AddEmissive((6.0, 8.0, 12.0))
        sc.AddQuad(20.0, 20.0, g, translation=(0.0, -1.0, 0.0))
        sc.AddCircle(0.25, e2, scale=(2.0, 2.0, 2.0), translation=(-2.0, 0.2, 1.0))
        sc.AddMesh(mesh, e)
        return sc
    W, H, D = 96, 54, 5
    cam = prt.Camera(position=(2.0, 1.5, 3.0), width=W, height=H)
    out = []
    for refit in (True, False):
        film = prt.Film(W, H)
        r = prt.HipWavefrontRenderer(device=0, max_depth=D, seed=3)
        r.set_light_sources("all")
        r.Init(film, scene(base if refit else moved), cam)
        r.set_lighting("mis")
        if refit:
            r.ProgressiveRender(1)
            before = r.light_intervals()
            r.Refit(scene(moved))
            assert not np.array_equal(before, r.light_intervals())
            film.Clear()
            r.frame_index = 0
        r.ProgressiveRender(2)
        r.download()
        out.append((r.light_info(), r.light_intervals(), r.light_stats().n_emitters_unsampled, film.accum.copy()))
        del r
    (i0, w0, u0, a0), (i1, w1, u1, a1) = out
    assert np.array_equal(i0[0], i1[0]) and np.array_equal(i0[1], i1[1]) and np.array_equal(w0, w1) and u0 == u1
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
    # a context that switches the mask on after the refit gets the refitted table too
    film = prt.Film(W, H)
    r = prt.HipWavefrontRenderer(device=0, max_depth=D, seed=3)
    r.Init(film, scene(base), cam)
    r.Refit(scene(moved))
    r.set_light_sources("all")
    r.set_lighting("mis")
    r.ProgressiveRender(2)
    r.download()
    assert np.array_equal(r.light_intervals(), w1) and np.array_equal(film.accum.view(np.uint32), a1.view(np.uint32))
