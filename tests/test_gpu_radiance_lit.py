"""The light-sampled radiance query (include/prt.h "Radiance query", prt_radiance_lit; radiance(lighting=True)) on the GPU.

1. The lit render is the lit query over its own rays, bit for bit: on a 9 x 7 film, depth 5, seed 11, the sum of the query
   over the pixel-centre rays (samples = 3, first_sample = 2) equals the fp32 sum, in ascending sample order, of three
   one-sample lit renders each read from a cleared film; the segments equal those renders' ray counts and the query's
   shadow-ray counts equal the renders' light statistics.  Both modes, on cases that reach every instance of the step
   kernel and every branch of the estimator (CASES).  The renders are held to float64 replays by the lighting tests.
2. Off means off: with the lighting off the lit entry point is the unlit one bit for bit; in every lighting mode the segments
   and the final RNG states are the unlit query's.
3. Rays that are not camera rays: at max_depth 2 under "nee" the lit sum is the unlit sum plus the light sample composed from
   closest_hit, sample_light and occluded, bit for bit.
4. Same expectation, less noise: 256 probe rays toward the ground under a small light, 16 batches of 256 samples.
   The measured figures are in test_probe_rays_same_expectation_less_noise's docstring.
5. Nothing else moves; sizes and forms; probes and the command line."""
import os
import subprocess

import numpy as np
import pytest

import lens_replay as lp
import lighting_replay as lr
import mesh_light_replay as mlr
import util
from util import prt

pytestmark = pytest.mark.gpu

F = np.float32
W, H, DEPTH, SEED = 9, 7, 5, 11
MODES = ("mis", "nee")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def renderer(scene, cam=None, depth=DEPTH):
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=SEED)
    film = prt.Film(W, H)
    r.Init(film, scene, cam or prt.Camera(width=W, height=H))
    return r, film


def _one_sample_renders(r, film, samples):
    """[accum of a one-sample render from a cleared film for each sample index], the rays and the shadow rays (cast,
    occluded) those renders traced."""
    out, rays, cast, occluded = [], 0, 0, 0
    for s in samples:
        film.Clear()
        r.reset_stats()
        l0 = r.light_stats()          # (whether or not reset_stats clears them: the render's own delta)
        r.frame_index = s
        r.ProgressiveRender()
        r.download()
        assert (film.weights == 1).all()
        out.append(film.accum.reshape(-1, 3).copy())
        rays += r.stats().rays_total
        l1 = r.light_stats()
        cast += l1.shadow_rays - l0.shadow_rays
        occluded += l1.shadow_occluded - l0.shadow_occluded
    return out, rays, (cast, occluded)


def _pixel_centres():
    y, x = np.mgrid[0:H, 0:W]
    return (x.ravel() + 0.5).astype(F), (y.ravel() + 0.5).astype(F)


def _textured_scene():
    """tests/test_gpu_radiance.py's: a textured ground and a textured mesh (restated: that module is not imported)."""
    sc = prt.scenes.mesh_scene(prt.Mesh(prt.scenes.asset("cube_uv.ply")))
    img = np.random.default_rng(5).uniform(0.05, 0.95, (6, 5, 3)).astype(F)
    t = sc.AddTexture(img, "bilinear", "repeat")
    sc.SetMaterialTexture(0, t)      # the ground
    sc.SetMaterialTexture(2, t)      # the mesh
    return sc


# name -> (what builds the case, light sources, light selection, does the case have blockers)
CASES = {
    "penumbra": (lambda: lr.case("penumbra", W, H), "analytic", "power", True),
    "bunny": (lambda: lr.case("bunny", W, H), "analytic", "power", True),
    "resting": (lambda: lr.case("resting", W, H), "analytic", "power", False),
    "specular": (lambda: lr.case("specular", W, H), "analytic", "power", True),
    "placed_all": (lambda: mlr.case("placed", W, H), "all", "power", True),
    "placed_clustered": (lambda: mlr.case("placed", W, H), "all", "clustered", True),
    "bunny_light_all": (lambda: mlr.case("bunny_light", W, H), "all", "power", True),
    "env_textures_analytic": (None, "analytic", "power", True),
    "env_textures_clustered": (None, "all", "clustered", True),
    "penumbra_rr_clamp": (lambda: lr.case("penumbra", W, H), "analytic", "power", True),
    "penumbra_aperture": (lambda: lr.case("penumbra", W, H), "analytic", "power", True),
}


def _case_renderer(name, mode):
    build, sources, selection, _ = CASES[name]
    if build is None:
        scene = _textured_scene()
        cam = prt.Camera((2.5, 2.0, 4.0), front=(-2.5, -2.0, -4.0), width=W, height=H)
    else:
        c = build()
        scene, cam = c["scene"], c["cam"]
    r, film = renderer(scene, cam)
    r.set_lighting(mode)
    if sources != "analytic":
        r.set_light_sources(sources)
    if selection != "power":
        r.set_light_selection(selection)
    if build is None:
        r.set_environment(np.random.default_rng(6).uniform(0.1, 2.0, (8, 16, 3)).astype(F), light_share=0.5)
        assert r.texture_info().n_textured_materials == 2 and r.environment_info().is_set
    if name == "penumbra_rr_clamp":
        r.set_sampling(rr_depth=2, clamp=1.5)
    if name == "penumbra_aperture":
        r.set_lens(0.0, 0.3, 9.0)
    return r, film


# ---- 1. the lit render is the lit query over its own rays -------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_lit_render_equals_the_lit_query_over_its_own_rays(case, mode):
    r, film = _case_renderer(case, mode)
    px, py = _pixel_centres()
    before = bytes(r.light_stats())
    if case == "penumbra_aperture":
        samples = (2,)
        keys = lp.path_seeds(np.arange(W * H), 2, SEED)
        o, d, after = r.camera_rays_lens(px, py, keys)
        assert (after != keys).all()
        _, info = r.radiance(o, d, rng_state=after, return_info=True, lighting=True)
    else:
        samples = (2, 3, 4)
        o, d = r.camera_rays(px, py)
        mean, info = r.radiance(o, d, samples=3, first_sample=2, return_info=True, lighting=True)
        assert np.array_equal(bits(mean), bits(info["sum"] / F(3)))
    assert bytes(r.light_stats()) == before          # the query's shadow rays are counted in its info alone
    frames, rays, (cast, occluded) = _one_sample_renders(r, film, samples)
    want = frames[0]
    for f in frames[1:]:
        want = (want + f).astype(F)
    print(f"\n{case} {mode}: rays {rays}, shadow rays {cast}, occluded {occluded}; the query: {info['shadow_rays']}, "
          f"{info['shadow_occluded']}; distinct pixels {len(np.unique(want, axis=0))}")
    # the reference side alone: the renders cast shadow rays, met blockers where there are some, and drew a picture
    assert cast > 0 and (occluded > 0 or not CASES[case][3]) and occluded <= cast
    assert (want > 0).any() and len(np.unique(want, axis=0)) > 4
    bad = np.nonzero((bits(info["sum"]) != bits(want)).any(axis=1))[0]
    assert bad.size == 0, (case, mode, bad[:8], info["sum"][bad[:3]], want[bad[:3]])
    assert int(info["segments"].sum(dtype=np.uint64)) == rays, (case, mode, int(info["segments"].sum()), rays)
    assert (info["shadow_rays"], info["shadow_occluded"]) == (cast, occluded), (case, mode)
    if case == "penumbra_rr_clamp":
        assert (info["segments"] < 3 * DEPTH).any()


# ---- 2. off means off -------------------------------------------------------------------------------------------------------
def test_off_means_off_and_the_path_is_the_unlit_path_in_every_mode():
    n = 4099
    rng = np.random.default_rng(21)
    o, d = util.random_rays(rng, n, center=(0.0, 1.0, 0.0), radius=12.0, spread=3.0)
    state = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    r, _ = renderer(prt.Scene("CORNELL"))
    base = r.radiance(o, d, rng_state=state, return_info=True)[1]
    off = r.radiance(o, d, rng_state=state, return_info=True, lighting=True)[1]
    assert np.array_equal(bits(off["sum"]), bits(base["sum"])) and np.array_equal(off["segments"], base["segments"])
    assert np.array_equal(off["rng_state"], base["rng_state"]) and off["shadow_rays"] == 0 and off["shadow_occluded"] == 0
    many = r.radiance(o, d, samples=3, first_sample=5, return_info=True)[1]
    off = r.radiance(o, d, samples=3, first_sample=5, return_info=True, lighting=True)[1]
    assert np.array_equal(bits(off["sum"]), bits(many["sum"])) and np.array_equal(off["segments"], many["segments"])
    differs = 0
    for mode, sources, selection in (("mis", "analytic", "power"), ("nee", "analytic", "power"), ("mis", "all", "clustered")):
        r.set_lighting(mode)
        r.set_light_sources(sources)
        r.set_light_selection(selection)
        lit = r.radiance(o, d, rng_state=state, return_info=True, lighting=True)[1]
        assert np.array_equal(lit["segments"], base["segments"]) and np.array_equal(lit["rng_state"], base["rng_state"]), mode
        assert lit["shadow_rays"] > 0
        differs += int((bits(lit["sum"]) != bits(base["sum"])).any())
        unlit = r.radiance(o, d, rng_state=state, return_info=True)[1]        # the unlit entry point does not follow the mode
        assert np.array_equal(bits(unlit["sum"]), bits(base["sum"]))
    assert differs == 3                                                        # another estimator: other sample values


# ---- 3. rays that are not camera rays ---------------------------------------------------------------------------------------
def test_light_term_composed_from_the_public_pieces():
    n = 1025
    c = lr.case("penumbra", W, H)
    r, _ = renderer(c["scene"], c["cam"])
    r.set_lighting("nee")
    rng = np.random.default_rng(33)
    o, d = util.random_rays(rng, n, center=(0.0, 0.5, 0.0), radius=7.0, spread=2.5)
    state = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    unlit = r.radiance(o, d, rng_state=state, max_depth=2, return_info=True)[1]
    lit = r.radiance(o, d, rng_state=state, max_depth=2, return_info=True, lighting=True)[1]
    assert np.array_equal(lit["segments"], unlit["segments"]) and np.array_equal(lit["rng_state"], unlit["rng_state"])
    # the composition: the first vertex, its light sample at throughput 1 (the first vertex's), the shadow ray
    hits = r.closest_hit(o, d)
    idx = np.nonzero(hits["prim"] >= 0)[0]
    sc, _, em, so, sd, _ = r.scatter(d[idx], hits[idx], state[idx])
    assert not em[sc].any()
    lam = idx[sc]                               # (the case's materials are Lambertian and Emissive: what scatters is Lambertian)
    lambertian = np.zeros(n, bool)
    lambertian[lam] = True
    ls = r.sample_light(d, hits, state)
    cast = lambertian & (ls["light"] != 0xFFFFFFFF) & (ls["pdf_bsdf"] > 0)
    assert not ls["contrib"][~cast].any()
    occ = np.zeros(n, bool)
    occ[cast] = r.occluded(hits["position"][cast], ls["dir"][cast], ls["tmax"][cast])
    # the second segment, as the unlit path is composed: from the scattered origin along the normalised direction
    second = r.closest_hit(so[sc], np.stack([prt.glm_normalize(v) for v in sd[sc]]))
    hit2 = np.nonzero(second["prim"] >= 0)[0]
    # Emissive = what emits: the case's one emitter is its light, and a segment that meets it has pdf_L > 0
    em2 = r.scatter(np.zeros((hit2.size, 3), F) + F(1), second[hit2], np.zeros(hit2.size, np.uint32))[2].any(axis=1)
    ends_on_light = np.zeros(n, bool)
    ends_on_light[lam[hit2[em2]]] = True
    keep = ~ends_on_light
    share = 1.0 - keep.mean()
    add = np.where((cast & ~occ)[:, None], ls["contrib"], F(0)).astype(F)
    want = (unlit["sum"] + add).astype(F)
    print(f"\nrays {n}: Lambertian first hits {int(lambertian.sum())}, shadow rays {int(cast.sum())}, occluded {int(occ.sum())}, "
          f"left out {int(ends_on_light.sum())} ({share:.3f})")
    assert share <= 0.25
    assert lambertian.sum() > n // 4 and (cast & ~occ).sum() > n // 16 and occ.sum() > 8
    bad = np.nonzero(keep & (bits(lit["sum"]) != bits(want)).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], lit["sum"][bad[:3]], want[bad[:3]], unlit["sum"][bad[:3]])
    other = ~lambertian
    assert np.array_equal(bits(lit["sum"][other]), bits(unlit["sum"][other]))
    # left out: under "nee" the emitter met by the second segment weighs 0, so the sample value is the light term alone
    assert np.array_equal(bits(lit["sum"][ends_on_light]), bits(add[ends_on_light]))
    assert (lit["shadow_rays"], lit["shadow_occluded"]) == (int(cast.sum()), int(occ.sum()))


# ---- 4. same expectation, less noise ----------------------------------------------------------------------------------------
def test_probe_rays_same_expectation_less_noise():
    """Measured on an MI355X (penumbra, 256 rays, 16 batches of 256 samples): unidirectional mean 1.513545, sd of the batch
    means 0.016738, 6 SE / mean = 0.0166 (below the 0.05 asked at 256 samples per batch); MIS mean 1.508395, sd 0.003236,
    variance ratio 26.8, |difference| = 1.23 SE; NEE mean 1.508324, sd 0.003294, variance ratio 25.8, |difference| = 1.25 SE."""
    c = lr.case("penumbra", W, H)
    r, _ = renderer(c["scene"], c["cam"])
    gx, gz = np.meshgrid(np.linspace(-3.0, 3.0, 16), np.linspace(-3.0, 3.0, 16))
    target = np.stack([gx.ravel(), np.full(256, -1.0), gz.ravel()], axis=1)
    origin = np.array([0.2, 1.0, 1.5])          # 2 above the ground, outside both blockers
    d = np.stack([prt.glm_normalize(v) for v in (target - origin).astype(F)])
    o = np.broadcast_to(origin.astype(F), d.shape).copy()
    S, B = 256, 16

    def batch_means(lighting):
        m = np.empty(B)
        for b in range(B):
            info = r.radiance(o, d, samples=S, first_sample=S * b, return_info=True, lighting=lighting)[1]
            m[b] = info["sum"].astype(np.float64).sum() / (S * d.shape[0])
        return m

    uni = batch_means(False)
    se = uni.std(ddof=1) / 4.0
    print(f"\nunidirectional: mean {uni.mean():.6f}, sd of batch means {uni.std(ddof=1):.6f}, 6 SE / mean {6 * se / uni.mean():.4f}")
    assert 6.0 * se < 0.05 * uni.mean()          # the yardstick can tell a wrong estimator
    for mode in MODES:
        r.set_lighting(mode)
        lit = batch_means(True)
        print(f"{mode}: mean {lit.mean():.6f}, sd of batch means {lit.std(ddof=1):.6f}, variance ratio "
              f"{(uni.std(ddof=1) / lit.std(ddof=1)) ** 2:.1f}, |difference| / SE {abs(lit.mean() - uni.mean()) / se:.2f}")
        assert abs(lit.mean() - uni.mean()) <= 6.0 * se, mode
        assert lit.std(ddof=1) < uni.std(ddof=1), mode
    r.set_lighting("off")
    assert np.array_equal(batch_means(True), uni)


# ---- 5. nothing else moves, sizes and forms ---------------------------------------------------------------------------------
def _state(r, film):
    r.download()
    return film.accum.copy(), film.weights.copy(), bytes(r.stats()), dict(r.batch_instances()), bytes(r.light_stats())


def _cloud(n, seed=44):
    rng = np.random.default_rng(seed)
    o, d = util.random_rays(rng, n, center=(0.0, 0.5, 0.0), radius=7.0, spread=2.5)
    return o, d, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def test_lit_query_leaves_film_statistics_and_the_next_render_alone():
    o, d, _ = _cloud(257)

    def run(with_query):
        c = lr.case("penumbra", W, H)
        r, film = renderer(c["scene"], c["cam"])
        r.set_lighting("mis")
        r.set_film_statistics(True)
        r.ProgressiveRender(2)
        before = _state(r, film) + tuple(a.copy() for a in r.film_statistics())
        got = r.radiance(o, d, samples=2, return_info=True, lighting=True)[1] if with_query else None
        after = _state(r, film) + tuple(a.copy() for a in r.film_statistics())
        r.ProgressiveRender(2)
        r.download()
        return before, after, film.accum.copy(), film.weights.copy(), bytes(r.light_stats()), got

    b0, a0, film0, w0, ls0, _ = run(False)
    b1, a1, film1, w1, ls1, got = run(True)
    for x, y in zip(b1, a1):          # across the query itself
        assert (np.array_equal(bits(x), bits(y)) if isinstance(x, np.ndarray) else x == y)
    assert np.array_equal(bits(film0), bits(film1)) and np.array_equal(w0, w1) and ls0 == ls1    # the render after it
    assert got["shadow_rays"] > got["shadow_occluded"] > 0 and got["sum"].any()


def test_counts_share_one_context_and_depths_zero_and_one():
    N = 4099
    o, d, state = _cloud(N)
    c = lr.case("penumbra", W, H)
    r, _ = renderer(c["scene"], c["cam"])
    r.set_lighting("mis")
    full = r.radiance(o, d, rng_state=state, return_info=True, lighting=True)[1]
    assert full["shadow_rays"] > full["shadow_occluded"] > 0
    for n in (65, 1, 3, N, 3):        # a ray's path depends on nothing but the ray and its state: every count is a prefix
        info = r.radiance(o[:n], d[:n], rng_state=state[:n], return_info=True, lighting=True)[1]
        assert np.array_equal(bits(info["sum"]), bits(full["sum"][:n])) and np.array_equal(info["segments"], full["segments"][:n]), n
        assert np.array_equal(info["rng_state"], full["rng_state"][:n]), n
    mean, info = r.radiance(np.zeros((0, 3), F), np.zeros((0, 3), F), return_info=True, lighting=True)
    assert mean.shape == (0, 3) and info["segments"].shape == (0,) and info["shadow_rays"] == 0
    # max_depth = 0: every output is zero, the states are left alone; max_depth = 1: no light sample, lit equals unlit
    mean, info = r.radiance(o[:65], d[:65], rng_state=state[:65], max_depth=0, return_info=True, lighting=True)
    assert not bits(info["sum"]).any() and not info["segments"].any() and np.array_equal(info["rng_state"], state[:65])
    assert info["shadow_rays"] == 0 and not bits(r.radiance(o[:65], d[:65], samples=3, max_depth=0, lighting=True)).any()
    one = r.radiance(o, d, rng_state=state, max_depth=1, return_info=True, lighting=True)[1]
    unlit = r.radiance(o, d, rng_state=state, max_depth=1, return_info=True)[1]
    assert one["shadow_rays"] == 0 and np.array_equal(bits(one["sum"]), bits(unlit["sum"])) and one["sum"].any()
    assert np.array_equal(one["segments"], unlit["segments"]) and np.array_equal(one["rng_state"], unlit["rng_state"])


def test_torch_device_tensors_give_the_bits_of_the_host_form():
    import torch
    n = 1500
    o, d, state = _cloud(n)
    c = lr.case("penumbra", W, H)
    r, _ = renderer(c["scene"], c["cam"])
    r.set_lighting("mis")
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    st = torch.from_numpy(state.view(np.int32).copy()).to(dev)
    host = r.radiance(o, d, rng_state=state, return_info=True, lighting=True)
    devi = r.radiance(to, td, rng_state=st, return_info=True, lighting=True)
    assert devi[0].device == dev and np.array_equal(bits(host[1]["sum"]), bits(devi[1]["sum"].cpu().numpy()))
    assert np.array_equal(host[1]["segments"], devi[1]["segments"].cpu().numpy().view(np.uint32))
    assert np.array_equal(host[1]["rng_state"], devi[1]["rng_state"].cpu().numpy().view(np.uint32))
    assert (host[1]["shadow_rays"], host[1]["shadow_occluded"]) == (devi[1]["shadow_rays"], devi[1]["shadow_occluded"])
    assert host[1]["shadow_rays"] > 0 and np.array_equal(st.cpu().numpy().view(np.uint32), state)
    host3 = r.radiance(o, d, samples=3, first_sample=1, lighting=True)
    dev3 = r.radiance(to, td, samples=3, first_sample=1, lighting=True)        # without info: no final wait for it
    assert np.array_equal(bits(host3), bits(dev3.cpu().numpy()))
    assert r.radiance(to[:0], td[:0], lighting=True).shape == (0, 3)


def test_forced_chunks_do_not_change_a_bit():
    n = 515
    o, d, _ = _cloud(n)
    c = lr.case("penumbra", W, H)
    r, _ = renderer(c["scene"], c["cam"])
    r.set_lighting("mis")
    whole = r.radiance(o, d, samples=5, first_sample=7, return_info=True, lighting=True)[1]
    acc = np.zeros((n, 3), F)         # sample s of ray i is the path of path_seed(i, first_sample + s, seed)
    for s in range(5):
        one = r.radiance(o, d, rng_state=lp.path_seeds(np.arange(n), 7 + s, SEED), return_info=True, lighting=True)[1]
        acc = (acc + one["sum"]).astype(F)
    assert np.array_equal(bits(whole["sum"]), bits(acc)) and whole["shadow_rays"] > 0
    for chunk in (1, 2):              # 5 samples as 1 + 1 + 1 + 1 + 1 and as 2 + 2 + 1
        r.set_param("radiance_chunk", chunk)
        got = r.radiance(o, d, samples=5, first_sample=7, return_info=True, lighting=True)[1]
        assert np.array_equal(bits(got["sum"]), bits(whole["sum"])) and np.array_equal(got["segments"], whole["segments"]), chunk
        assert (got["shadow_rays"], got["shadow_occluded"]) == (whole["shadow_rays"], whole["shadow_occluded"]), chunk
    r.set_param("radiance_chunk", 0)


def test_lit_probe_of_an_empty_scene_is_its_environment():
    r, _ = renderer(prt.Scene(preset=None))
    E = np.random.default_rng(9).uniform(0.05, 4.0, (8, 16, 3)).astype(F)
    r.set_environment(E)
    for mode in MODES:
        r.set_lighting(mode)
        assert np.array_equal(bits(r.render_probe((1, 2, 3), 8, 16, samples=1, lighting=True)), bits(E)), mode
        assert np.array_equal(bits(r.render_probe((1, 2, 3), 8, 16, samples=4, lighting=True)), bits(E)), mode


def test_command_line_lit_probe_equals_render_probe(tmp_path):
    exe = os.path.join(util.ROOT, "parallelraytracing_amd", "csrc", "prt_render")
    args = [exe, "--preset", "CORNELL", "--probe", "0.5,1.5,0.25", "--probe-size", "12x6", "--spp", "3", "--depth", "4",
            "--seed", str(SEED), "--lighting", "mis"]
    out = [str(tmp_path / "lit"), str(tmp_path / "unlit")]
    for path, extra in zip(out, (["--probe-lighting"], [])):
        p = subprocess.run(args + extra + ["--out", path], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
    r, _ = renderer(prt.Scene("CORNELL"), depth=4)
    r.set_lighting("mis")
    want = r.render_probe((0.5, 1.5, 0.25), 6, 12, samples=3, lighting=True)
    unlit = r.render_probe((0.5, 1.5, 0.25), 6, 12, samples=3)
    got = prt.read_pfm(out[0] + ".pfm")
    assert got.shape == (6, 12, 3) and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(prt.read_pfm(out[1] + ".pfm")), bits(unlit))     # without the flag a probe is what it was
    assert not np.array_equal(bits(want), bits(unlit)) and len(np.unique(want.reshape(-1, 3), axis=0)) > 12
