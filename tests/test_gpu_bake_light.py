"""The texel's light sample of surface baking (include/prt.h "Surface baking"; bake_light_samples, bake_irradiance(texel_light=))
on the GPU.

1. Samples: bake_light_samples equals sample_light over hits built from bake_surface on a white Lambertian (in_dirs = -n,
   keys = path_seed(t, s, seed)) bit for bit: dir, light, tmax (0 where n.w <= 0 or there is no sample), contrib clamped,
   and ray_pb equals the fp32 expression of the header over bake_rays' directions.
2. Composition: the sums of bake_irradiance(texel_light=True) equal the fp32 sum, in ascending sample order, of
   fl(q + e): q = radiance(o, d, rng_state, lighting=True, pb=ray_pb), e = contrib where tmax > 0 and not occluded; bit for
   bit, in every chunking, numpy and torch outputs, and the shadow rays add up.
3. Nothing else moves: without the option (or with lighting off, either way) the _opt entry equals prt_bake_irradiance
   bit for bit; film, statistics and the next render are untouched.
4. Closed form: the form factor of an emissive quad under nee + texel light, mis + texel light and mis alone, held per
   texel and over the map with the standard error estimated from the sample values themselves."""
import ctypes as C

import numpy as np
import pytest

import bake_replay as br
import closed_form as cf
from util import prt
from parallelraytracing_amd import capi
from test_gpu_bake import SEED, bits, cornell_with_cube, env_textured, renderer, textured

pytestmark = pytest.mark.gpu

F = np.float32
INV_PI = F(0.318309886183790672)
NONE = 0xFFFFFFFF


def emissive_square():
    """A 0.6 x 0.6 emissive square facing down: a mesh emitter for set_light_sources("all")"""
    m = br.square_mesh(0.6)
    mat, inv = prt.make_transform((1.0, 1.0, 1.0), (180.0, 0.0, 0.0), (-0.3, 1.6, 0.2))
    return m.transform(mat, inv)


def target_scene(case):
    """-> (scene, target keywords with UVs, the white Lambertian's material id).  Every scene holds one extra Lambertian of
    albedo (1, 1, 1) that no primitive uses: the material of the hits prt_sample_light stands in with."""
    if case == "env_textures":
        sc, mesh = env_textured()
        kw = dict(mesh=0)
    elif case == "copy":
        sc = prt.Scene(preset=None, sky=(0.4, 0.3, 0.6))
        ground, light, body = sc.AddLambertian((0.5, 0.5, 0.5)), sc.AddEmissive((15.0, 15.0, 15.0)), sc.AddLambertian((0.8, 0.8, 0.8))
        sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -2.0, 0.0))
        sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 7.0, 0.0))
        sc.AddMesh(br.square_mesh(3.0, -1.5), ground)
        mesh = br.cube_mesh()
        sc.AddInstance(mesh, body, scale=br.COPY_SRT[0], euler_deg=br.COPY_SRT[1], translation=br.COPY_SRT[2])
        textured(sc, (body,))
        kw = dict(instance=0, uvs=br.cube_atlas_uvs(mesh))
    else:
        sc, mesh = cornell_with_cube()
        sc.AddMesh(emissive_square(), sc.AddEmissive((300.0, 250.0, 200.0)))      # (bright: the power rule picks its triangles too)
        kw = dict(mesh=0, uvs=br.cube_atlas_uvs(mesh))
    white = sc.AddLambertian((1.0, 1.0, 1.0))
    return sc, kw, white


def configure(r, case, mode):
    r.set_lighting(mode)
    if case == "env_textures":
        r.set_environment(np.random.default_rng(6).uniform(0.1, 2.0, (8, 16, 3)).astype(F), 0.5)
        r.set_light_sources("all")
    elif case == "all_power":
        r.set_light_sources("all")
    elif case == "clustered":
        r.set_light_sources("all")
        r.set_light_selection("clustered", 4)
        r.set_sampling(clamp=0.75)
    elif case == "rr_clamp":
        r.set_sampling(rr_depth=2, clamp=1.5)


def ray_pb_of(normal, d):
    n, d = normal.astype(F), d.astype(F)
    c = ((n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]).astype(F) + (n[..., 2] * d[..., 2]).astype(F)).astype(F)
    return (np.where(c > 0, c, F(0)).astype(F) * INV_PI).astype(F)


# ---- 1. samples -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", [("cornell", "mis"), ("all_power", "nee"), ("clustered", "mis"), ("env_textures", "mis"),
                                       ("copy", "mis"), ("cornell", "off")])
def test_samples_equal_sample_light_on_a_white_vertex(case, mode):
    sc, kw, white = target_scene(case)
    r, _ = renderer(sc)
    configure(r, case, mode)
    H, W = (17, 33) if case != "env_textures" else (16, 16)      # (the binding's UVs cover the whole 16 x 16 map)
    surf = r.bake_surface(size=(H, W), **kw)
    cov = surf["coverage"].ravel() != 0
    assert cov.sum() > 100 and (case == "env_textures") == bool(cov.all())
    t = np.nonzero(cov)[0]
    p, n = surf["position"].reshape(-1, 3)[cov], surf["normal"].reshape(-1, 3)[cov]
    hits = np.zeros(len(t), dtype=capi.HIT_DTYPE)
    hits["front_face"], hits["material_id"], hits["position"], hits["normal"] = 1, white, p, n
    clamp = F(0.75) if case == "clustered" else None
    lights = set()
    for s in (0, 3):
        keys = br.path_seed(t, s, SEED).astype(np.uint32)
        want = r.sample_light((-n).astype(F), hits, keys)
        got = r.bake_light_samples(size=(H, W), sample=s, **kw)
        flat = {k: v.reshape(H * W, -1) if v.ndim == 3 else v.ravel() for k, v in got.items()}
        cast = want["pdf_bsdf"] > 0
        assert np.array_equal(bits(flat["dir"][cov]), bits(want["dir"])), (case, s)
        assert np.array_equal(flat["light"][cov], want["light"]), (case, s)
        assert np.array_equal(bits(flat["tmax"][cov]), bits(np.where(cast, want["tmax"], F(0)).astype(F))), (case, s)
        wc = want["contrib"] if clamp is None else np.minimum(clamp, want["contrib"]).astype(F)
        assert np.array_equal(bits(flat["contrib"][cov]), bits(wc)), (case, s)
        assert not wc[~cast].any()
        d = r.bake_rays(size=(H, W), sample=s, **kw)["d"]
        assert np.array_equal(bits(got["ray_pb"]), bits(ray_pb_of(surf["normal"], d)))
        # uncovered texels: zero / none
        assert not flat["dir"][~cov].any() and not flat["tmax"][~cov].any() and not flat["contrib"][~cov].any()
        assert (flat["light"][~cov] == NONE).all() and not got["ray_pb"].ravel()[~cov].any()
        # the case does what its name says
        assert cast.sum() > 20 and (flat["tmax"][cov] == 0).any() and flat["contrib"][cov].any()
        if clamp is not None:
            assert (want["contrib"] > clamp).any()
        lights |= set(np.unique(want["light"]).tolist())
    if case == "env_textures":
        assert capi.LIGHT_ENVIRONMENT in lights and len(lights - {NONE}) >= 2
    elif case in ("all_power", "clustered"):
        assert len(lights - {NONE}) >= 3       # the quad and both triangles of the emissive square


# ---- 2. composition -------------------------------------------------------------------------------------------------------
def _composition(r, kw, H, W, samples, first):
    surf = r.bake_surface(size=(H, W), **kw)
    cov = surf["coverage"].ravel() != 0
    p = surf["position"].reshape(-1, 3)[cov]
    total = np.zeros((int(cov.sum()), 3), F)
    seg = shadow = texel_rays = 0
    for s in range(first, first + samples):
        ray = r.bake_rays(size=(H, W), sample=s, **kw)
        ls = r.bake_light_samples(size=(H, W), sample=s, **kw)
        tmax, w, contrib = ls["tmax"].ravel()[cov], ls["dir"].reshape(-1, 3)[cov], ls["contrib"].reshape(-1, 3)[cov]
        occ = r.occluded(p, w, tmax)
        e = np.where(((tmax > 0) & ~occ)[:, None], contrib, F(0)).astype(F)
        _, q = r.radiance(ray["o"].reshape(-1, 3)[cov], ray["d"].reshape(-1, 3)[cov], rng_state=ray["rng_state"].ravel()[cov], samples=1,
                          return_info=True, lighting=True, pb=ls["ray_pb"].ravel()[cov])
        total = (total + (q["sum"] + e).astype(F)).astype(F)
        seg += int(q["segments"].sum(dtype=np.uint64))
        shadow += q["shadow_rays"] + int((tmax > 0).sum())
        texel_rays += int((tmax > 0).sum())
    return cov, total, seg, shadow, texel_rays


@pytest.mark.parametrize("mode", ["mis", "nee"])
@pytest.mark.parametrize("case", ["cornell", "env_textures", "rr_clamp", "clustered"])
def test_bake_is_the_composition_of_the_public_functions_bit_for_bit(case, mode):
    sc, kw, _ = target_scene(case)
    r, _ = renderer(sc)
    configure(r, case, mode)
    H, W = (16, 16) if case == "env_textures" else (17, 33)
    cov, want, seg, shadow, texel_rays = _composition(r, kw, H, W, 3, 2)
    assert cov.sum() > 100 and want.any() and texel_rays > cov.sum() // 2 and len(np.unique(want, axis=0)) > 4
    plain = r.bake_irradiance(size=(H, W), samples=3, first_sample=2, lighting=True, return_info=True, **kw)[1]
    assert not np.array_equal(bits(plain["sum"].reshape(-1, 3)[cov]), bits(want))      # the option does something
    for chunk in (0, 1, 2):
        r.set_param("bake_chunk", chunk)
        irr, got = r.bake_irradiance(size=(H, W), samples=3, first_sample=2, lighting=True, texel_light=True, return_info=True, **kw)
        total = got["sum"].reshape(-1, 3)
        bad = np.nonzero((bits(total[cov]) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (case, mode, chunk, bad[:8], total[cov][bad[:3]], want[bad[:3]])
        assert not total[~cov].any() and np.array_equal(got["coverage"].ravel() != 0, cov)
        assert got["info"]["segments"] == seg == plain["info"]["segments"]
        assert got["info"]["rays"] == 3 * cov.sum() == plain["info"]["rays"] and got["info"]["n_covered"] == cov.sum()
        assert got["info"]["shadow_rays"] == shadow
        assert 0 < got["info"]["shadow_occluded"] < shadow
        assert np.array_equal(bits(irr), bits(got["sum"] * F(np.pi) / F(3)))
    r.set_param("bake_chunk", 0)
    irr_t, got_t = r.bake_irradiance(size=(H, W), samples=3, first_sample=2, lighting=True, texel_light=True, out="torch", return_info=True, **kw)
    assert irr_t.is_cuda and np.array_equal(bits(got_t["sum"].cpu().numpy().reshape(-1, 3)[cov]), bits(want))
    assert got_t["info"]["shadow_rays"] == shadow and np.array_equal(bits(irr_t.cpu().numpy()), bits(irr))


def test_depth_zero_is_zero_and_takes_no_sample():
    sc, kw, _ = target_scene("cornell")
    r, _ = renderer(sc)
    r.set_lighting("mis")
    _, got = r.bake_irradiance(size=(16, 16), samples=2, max_depth=0, lighting=True, texel_light=True, return_info=True, **kw)
    assert not got["sum"].any() and got["info"]["shadow_rays"] == 0 and got["info"]["segments"] == 0 and got["coverage"].any()


# ---- 3. nothing else moves ------------------------------------------------------------------------------------------------
def _opt_entry(r, kw, H, W, samples, opt, depth=5):
    """prt_bake_irradiance_opt called directly: every combination of the option words, whatever the Python layer allows"""
    uv = np.ascontiguousarray(kw["uvs"], F)
    t = capi.PrtBakeTarget(capi.BAKE_MESH, kw["mesh"], uv.ctypes.data_as(C.POINTER(C.c_float)), W, H)
    q = capi.PrtRadianceQuery(depth, samples, SEED, 0)
    total, cov, info = np.zeros((H, W, 3), F), np.zeros((H, W), np.uint8), capi.PrtBakeInfo()
    o = capi.PrtBakeOptions(*opt)
    r._check(capi.lib().prt_bake_irradiance_opt(r._ctx, C.byref(t), C.byref(q), C.byref(o), total.ctypes.data_as(C.POINTER(C.c_float)),
                                                cov.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info)))
    return total, cov, {k: v for k, v in r._bake_info(info).items() if k != "device_ms"}


def _old_entry(r, kw, H, W, samples, lighting, dilate, depth=5):
    uv = np.ascontiguousarray(kw["uvs"], F)
    t = capi.PrtBakeTarget(capi.BAKE_MESH, kw["mesh"], uv.ctypes.data_as(C.POINTER(C.c_float)), W, H)
    q = capi.PrtRadianceQuery(depth, samples, SEED, 0)
    total, cov, info = np.zeros((H, W, 3), F), np.zeros((H, W), np.uint8), capi.PrtBakeInfo()
    r._check(capi.lib().prt_bake_irradiance(r._ctx, C.byref(t), C.byref(q), int(lighting), dilate, total.ctypes.data_as(C.POINTER(C.c_float)),
                                            cov.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info)))
    return total, cov, {k: v for k, v in r._bake_info(info).items() if k != "device_ms"}


def test_without_the_option_the_opt_entry_is_the_bake_bit_for_bit():
    sc, kw, _ = target_scene("cornell")
    r, _ = renderer(sc)
    H, W = 17, 33

    def same(a, b):
        return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]

    for mode in ("off", "mis"):
        r.set_lighting(mode)
        r.set_light_sources("all")
        unlit, lit = _old_entry(r, kw, H, W, 3, 0, 1), _old_entry(r, kw, H, W, 3, 1, 1)
        assert same(_opt_entry(r, kw, H, W, 3, (0, 0, 1, 0)), unlit)        # lighting = 0
        assert same(_opt_entry(r, kw, H, W, 3, (0, 1, 1, 0)), unlit)        # lighting = 0: the texel option has no effect
        assert same(_opt_entry(r, kw, H, W, 3, (1, 0, 1, 0)), lit)          # texel_light = 0
        on = _opt_entry(r, kw, H, W, 3, (1, 1, 1, 0))
        assert same(on, lit) == (mode == "off")                             # mode off: no texel sample either
        assert same(unlit, lit) == (mode == "off") and lit[0].any()
        assert (lit[2]["shadow_rays"] > 0) == (mode == "mis") and (on[2]["shadow_rays"] > lit[2]["shadow_rays"]) == (mode == "mis")
    irr = r.bake_irradiance(size=(H, W), samples=3, lighting=True, dilate=1, seed=SEED, **kw)      # the Python layer goes through _opt
    assert np.array_equal(bits(irr), bits(lit[0] * F(np.pi) / F(3)))


def _state(r, film):
    r.download()
    return film.accum.copy(), film.weights.copy(), bytes(r.stats()), dict(r.batch_instances()), bytes(r.light_stats())


def test_texel_light_leaves_film_statistics_and_the_next_render_alone():
    def run(with_bake):
        sc, kw, _ = target_scene("cornell")
        r, film = renderer(sc)
        r.set_lighting("mis")
        r.set_light_sources("all")
        r.set_film_statistics(True)
        r.ProgressiveRender(2)
        before = _state(r, film) + tuple(a.copy() for a in r.film_statistics())
        got = None
        if with_bake:
            got = r.bake_irradiance(size=(16, 16), samples=2, dilate=1, lighting=True, texel_light=True, return_info=True, **kw)[1]
            r.bake_light_samples(size=(16, 16), sample=1, **kw)
        after = _state(r, film) + tuple(a.copy() for a in r.film_statistics())
        r.ProgressiveRender(2)
        r.download()
        return before, after, film.accum.copy(), film.weights.copy(), got

    b0, a0, film0, w0, _ = run(False)
    b1, a1, film1, w1, got = run(True)
    for x, y in zip(b1, a1):          # across the bake itself
        assert (np.array_equal(bits(x), bits(y)) if isinstance(x, np.ndarray) else x == y)
    assert np.array_equal(bits(film0), bits(film1)) and np.array_equal(w0, w1)    # the render after it
    assert got["sum"].any() and got["info"]["shadow_rays"] > 0


# ---- 4. closed form -------------------------------------------------------------------------------------------------------
def test_form_factor_with_the_texel_sample():
    sc, mat = br.ff_scene()
    sc.AddLambertian((1.0, 1.0, 1.0))
    r, _ = renderer(sc)
    H, W = br.FF_MAP
    S = br.FF_SAMPLES
    uv = br.square_mesh().GetUVs()
    surf = r.bake_surface(mesh=0, size=(H, W), uvs=uv)
    Fq = cf.form_factor(surf["position"].reshape(-1, 3).astype(np.float64), surf["normal"].reshape(-1, 3).astype(np.float64),
                        cf.quad_corners(mat, br.FF_QUAD["width"], br.FF_QUAD["height"]))
    assert Fq.min() >= 0.05 and Fq.max() <= 0.95
    Le = np.asarray(br.FF_EMISSION, np.float64)
    variances = {}
    for name, mode, texel in (("nee + texel light", "nee", True), ("mis + texel light", "mis", True), ("mis", "mis", False)):
        r.set_lighting(mode)
        _, got = r.bake_irradiance(mesh=0, size=(H, W), uvs=uv, samples=S, max_depth=1, lighting=True, texel_light=texel, return_info=True)
        assert (got["coverage"] == 1).all()
        m = (got["sum"].reshape(-1, 3).astype(np.float64) / (S * Le)).mean(axis=1)
        # the S sample values themselves: S one-sample bakes (the map's sum is their fp32 sum in this order)
        vals = np.stack([r.bake_irradiance(mesh=0, size=(H, W), uvs=uv, samples=1, first_sample=s, max_depth=1, lighting=True, texel_light=texel,
                                           return_info=True)[1]["sum"].reshape(-1, 3) for s in range(S)])
        if name == "nee + texel light":      # no occluders: the values are bake_light_samples' contribs
            for s in (0, 7):
                assert np.array_equal(bits(vals[s]), bits(r.bake_light_samples(mesh=0, size=(H, W), uvs=uv, sample=s)["contrib"].reshape(-1, 3)))
        x = (vals.astype(np.float64) / Le).mean(axis=2)                    # [S, texels]
        assert np.allclose(x.mean(axis=0), m, rtol=1e-5, atol=1e-7)
        var = x.var(axis=0, ddof=1)
        assert (var > 0).all()
        se = np.sqrt(var / S)
        z = (m - Fq) / se
        Z = (m.sum() - Fq.sum()) / np.sqrt((se ** 2).sum())
        variances[name] = var.mean()
        print(f"form factor, {name}: max |z| = {np.abs(z).max():.3f}, map |Z| = {abs(Z):.3f}, mean per-texel sample variance = {var.mean():.6f}")
        assert np.abs(z).max() <= 6.5 and abs(Z) <= 6.0, (name, np.abs(z).max(), Z)
    print("variances:", variances)
