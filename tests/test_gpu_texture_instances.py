"""Every texture instance of the shade kernels on one MI355X, against the replays (tests/texture_replay.py, whose gate and
undecidable shares tests/test_texture_replay.py checks on the CPU), and three routes of a batch that no other test takes.

prt_plan_route (csrc/prt_route.h) chooses one of 24 texture instances from four facts: INST (placed copies), ABVH (the
primitive BVH: more than 16 analytic primitives and prim_bvh = 1), MESHL (triangle lights), ENV (an environment image).
Renderer.shade_instance() names the instance a batch launched, in the instance list's own words; every test here asserts it.
Scenes: C (22 primitives, no copies), D (C + placed copies), Q_small / Q_big (8 / 20 quads, no triangle at all), E (scene B's
bunny alone, 3 primitives), A and B of tests/test_gpu_textures.py.  "pb0": the same case with prim_bvh = 0, asserted
bit-identical to the frames of the case beside it.

  instance                                       held to the replay by                            also run by
  k_shade_tex<false, false, false>               frames Q_small                                   Q_big pb0, C pb0
  k_shade_tex<false, false, true>                frames Q_small + env                             Q_big pb0, C pb0 (+ env)
  k_shade_tex<false, true, false>                frames C, Q_big; lens C
  k_shade_tex<false, true, true>                 frames C + env, Q_big + env
  k_shade_tex<true, false, false>                lens A (and test_gpu_textures.py, frames A, B)   D pb0
  k_shade_tex<true, false, true>                 D + env pb0 (bit-equal to frames D + env)
  k_shade_tex<true, true, false>                 frames D
  k_shade_tex<true, true, true>                  frames D + env
  k_shade_nee_tex<false, false, false, false>    E_mis_analytic                                   C_mis_analytic pb0, variants, sort_rays
  k_shade_nee_tex<false, false, false, true>     E_mis_env                                        C_mis_env pb0
  k_shade_nee_tex<false, false, true, false>     E_nee_mesh                                       C_nee_mesh pb0
  k_shade_nee_tex<false, false, true, true>      E_nee_mesh_env                                   C_nee_mesh_env pb0
  k_shade_nee_tex<false, true, false, false>     C_mis_analytic
  k_shade_nee_tex<false, true, false, true>      C_mis_env
  k_shade_nee_tex<false, true, true, false>      C_nee_mesh
  k_shade_nee_tex<false, true, true, true>       C_nee_mesh_env
  k_shade_nee_tex<true, false, false, false>     test_gpu_textures.py A_mis_analytic, B_nee_analytic; lens A_mis_analytic    D_nee_analytic pb0
  k_shade_nee_tex<true, false, false, true>      test_gpu_textures.py A_mis_env                   D_nee_analytic_env pb0
  k_shade_nee_tex<true, false, true, false>      test_gpu_textures.py B_mis_mesh                  D_mis_mesh pb0
  k_shade_nee_tex<true, false, true, true>       test_gpu_textures.py B_nee_mesh_env              D_mis_mesh_env pb0
  k_shade_nee_tex<true, true, false, false>      D_nee_analytic
  k_shade_nee_tex<true, true, false, true>       D_nee_analytic_env
  k_shade_nee_tex<true, true, true, false>       D_mis_mesh
  k_shade_nee_tex<true, true, true, true>        D_mis_mesh_env
The last test of the module asserts that the names seen through shade_instance() in the tests above are exactly these 24.

  1. prt_hit_uv on C, D and Q: hits equal prt_closest_hit and the oracle, UVs and albedo equal the restatement bit for bit, and
     prim_bvh = 0 gives identical arrays.
  2. Frames, lighting off (C, D, Q_small, Q_big; without and with an environment image; 4 samples, once plain and once with
     jitter, roulette and clamp in calls of 1 + 3): the film equals texture_replay.frame's fp32 sums bit for bit, rays_per_depth
     its segment counts; prim_bvh = 0 gives the same film.  Under an image a miss takes the device's own lookup of its direction
     (prt_environment_eval, held to the float64 mapping by tests/test_gpu_environment.py): a float64 lookup cannot settle a
     direction on a texel edge, and the film is compared whole.
  3. Lighting through the float64 replays (lighting_replay, mesh_light_replay, environment_replay with the textured walker):
     tolerances, checks and the compared share are the replays' own.
  4. Textures under a thin lens (A, C; jitter 0 / 1): the replay walks the renderer's own lens rays; one lit case.
  5. Traversal variants 0 / 1 / 2 under lighting (E textured, lighting_replay's bunny untextured): frames and light statistics
     bit-identical, variant 0 held to the replay.
  6. sort_rays 1 / 2 against 0 (B, E with mis, an untextured jittered bunny): films, rays_per_depth and light statistics
     bit-identical.
Every frame is at most 48 x 36 at depth 4, except the untextured bunny's 80 x 60 at depth 5.

Figures of the first run on an MI355X (all 44 cases pass, the file in under 10 s): every bit-for-bit comparison exact, every
instance name as the table has it; the lighting replays (compared / left out as undecidable / worst error over tolerance / shadow
rays GPU = replay / occluded):
  C_mis_analytic      4800 / 0 / 0.051 / 5009 = 5009 / 727      C_nee_mesh          4800 / 0 / 0.165 / 4981 = 4981 / 843
  C_mis_env           4799 / 1 / 0.176 / 5213 = 5213 / 781      C_nee_mesh_env      4799 / 1 / 0.195 / 5180 = 5180 / 836
  D_nee_analytic      4800 / 0 / 0.044 / 4823 = 4823 / 767      D_mis_mesh          4800 / 0 / 0.165 / 4797 = 4797 / 887
  D_nee_analytic_env  4799 / 1 / 0.178 / 5078 = 5078 / 816      D_mis_mesh_env      4799 / 1 / 0.178 / 5047 = 5047 / 870
  E_mis_analytic      4800 / 0 / 0.043 / 3036 = 3036 / 183      E_nee_mesh          4800 / 0 / 0.050 / 3042 = 3042 / 283
  E_mis_env           4800 / 0 / 0.213 / 3118 = 3118 / 119      E_nee_mesh_env      4800 / 0 / 0.221 / 3121 = 3121 / 175
  A_mis_analytic under the lens  6912 / 0 / 0.043 / 4008 = 4008 / 172
  bunny, 80 x 60, variant 0      19198 / 2 / 0.047 / 12113 = 12113 / 1166     (E_mis_analytic, variant 0: the figures above)
The triangle lights took 230 (C), 228 (D) and 202 (E) of the light samples.  No test exposed a defect."""
import numpy as np
import pytest

import environment_replay as er
import lens_replay as lp
import lighting_replay as lr
import mesh_light_replay as mr
import texture_replay as tr
import util
from util import orc, prt

pytestmark = pytest.mark.gpu
F = np.float32
B = ("false", "true")
ALL = {f"k_shade_tex<{i}, {a}, {e}>" for i in B for a in B for e in B} | \
      {f"k_shade_nee_tex<{i}, {a}, {m}, {e}>" for i in B for a in B for m in B for e in B}
SEEN = set()      # what shade_instance() answered after the renders of this module
ENV_OFF = "5x3"   # the image of the frames without light sampling (environment_replay.named_map)
LENS = (0.9, 0.15, 5.0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _name(lit, inst, abvh, mesh=False, env=False):
    if lit:
        return f"k_shade_nee_tex<{B[inst]}, {B[abvh]}, {B[mesh]}, {B[env]}>"
    return f"k_shade_tex<{B[inst]}, {B[abvh]}, {B[env]}>"


def _ran(r, want):
    got = r.shade_instance()
    SEEN.add(got)
    assert got == want


def _scene(name):
    return {"A": tr.scene_a, "B": tr.scene_b, "C": tr.scene_c, "D": tr.scene_d, "Q_small": tr.scene_q, "Q_big": lambda: tr.scene_q(big=True)}[name]()


def _facts(name):
    """(INST, ABVH with prim_bvh = 1) of a scene"""
    return name[0] in "ABD", name[0] in "CD" or name == "Q_big"


def _renderer(c, sif=4, sampling=None, lighting=None, sources=None, env=None, params=(), seed=tr.SEED, lens=None, variant=None):
    film = prt.Film(c["W"], c["H"])
    r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=seed)
    for k, v in params:
        r.set_param(k, v)
    if sources:
        r.set_light_sources(sources)
    if env is not None:
        r.set_environment(env[0], env[1])
    if lens:
        r.set_lens(*lens)
    r.Init(film, c["scene"], c["cam"])
    r.set_samples_in_flight(sif)
    if sampling and tuple(sampling) != (0, 0, 0.0):
        r.set_sampling(*sampling)
    if lighting:
        r.set_lighting(lighting)
    if variant:
        r.set_variant(variant)
    return r, film


def _render(r, film, calls):
    for k in calls:
        r.ProgressiveRender(k)
    r.download()
    return film.accum.copy(), film.weights.copy(), [int(v) for v in r.stats().rays_per_depth]


# ---- 0. the query itself ------------------------------------------------------------------------------------------------------
def test_shade_instance_names_the_untextured_launches_too():
    c = tr.scene_a("none")
    r, film = _renderer(c)
    assert r.shade_instance() == ""                       # nothing launched yet
    r.ProgressiveRender(1)
    assert r.shade_instance() == "k_shade<0, true, true, false, false>"
    r.set_lighting("mis")
    r.ProgressiveRender(1)
    assert r.shade_instance() == "k_shade_nee<true, false>"
    r.set_lighting("off")
    r.set_environment(er.named_map("1x1"), 0.5)
    r.ProgressiveRender(1)
    assert r.shade_instance() == "k_shade_env<true, false>"
    r.synchronize()


# ---- 1. UV and albedo of hits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C", "D", "Q_small", "Q_big"])
def test_hit_uv_equals_the_restatement_bit_for_bit(name):
    c = _scene(name)
    ts = tr.TexScene(c["scene"])
    o, d = tr.primary_and_random_rays(c)
    r, _ = _renderer(c)
    hits, uv, alb = r.hit_uv(o, d)
    assert util.hits_equal(hits, r.closest_hit(o, d)) == []
    want_hits = orc.OracleScene(c["scene"].desc()).closest_hit(o, d, use_bvh=True, n_threads=lr.n_threads_default())
    assert util.hits_equal(hits, want_hits) == []
    want_uv, _ = ts.hit_uv(o, d, hits)
    want_alb = ts.albedo(hits, want_uv)
    bad = np.nonzero((uv != want_uv).any(1))[0]
    assert len(bad) == 0, (len(bad), hits["prim"][bad[:8]], uv[bad[:4]], want_uv[bad[:4]])
    assert np.array_equal(_bits(alb), _bits(want_alb))
    hit = hits["prim"] >= 0
    assert ts.textured(hits).sum() > 500 and (~hit).sum() > 100
    assert np.all(uv[~hit] == 0) and np.all(alb[~hit] == 0)
    rotated = np.isin(hits["prim"], c["rotated_quads"]) & hit
    assert rotated.sum() > 20 and (rotated & (hits["front_face"] == 0)).sum() > 20
    if name in "CD":          # the bunny's UVs leave [0, 1] on both sides under a clamped image
        world = (hits["prim"] >= ts.n_prims) & (hits["prim"] < ts.n_prims + ts.n_world)
        assert uv[world].min() < -0.2 and uv[world].max() > 1.2
    # the linear scan over the primitives in the primitive BVH's place
    r0, _ = _renderer(c, params=(("prim_bvh", 0),))
    hits0, uv0, alb0 = r0.hit_uv(o, d)
    assert util.hits_equal(hits0, hits) == []
    assert np.array_equal(_bits(uv0), _bits(uv)) and np.array_equal(_bits(alb0), _bits(alb))


# ---- 2. frames, lighting off --------------------------------------------------------------------------------------------------
def _env_off(on):
    return (er.named_map(ENV_OFF), 0.5) if on else None


def _device_lookup(r):
    return lambda d: r.environment_eval(d)["rgb"]


def _check_frame(monkeypatch, c, sampling, calls, want_name, with_env=False, lens=None, pb0_name=None):
    spp = sum(calls)
    r, film = _renderer(c, sampling=sampling, env=_env_off(with_env), lens=lens)
    if with_env:
        monkeypatch.setattr(tr, "MISS_RGB", _device_lookup(r))
    if lens:
        monkeypatch.setattr(lr, "primary_rays", lambda cam_desc, W, pix, rng, jitter: r.camera_rays_lens(*lp.jittered_points(pix, W, rng, jitter)))
    osc = orc.OracleScene(c["scene"].desc())
    want, wwts, per_depth = tr.frame(c["scene"], osc, c["cam"], c["W"], c["H"], c["depth"], tr.SEED, 0, spp, sampling)
    got, wts, rays = _render(r, film, calls)
    _ran(r, want_name)
    bad = np.nonzero((_bits(got) != _bits(want)).any(2))
    assert len(bad[0]) == 0, (c["name"], sampling, len(bad[0]), got[bad][:3], want[bad][:3])
    assert np.array_equal(wts, wwts)
    assert rays[:c["depth"]] == per_depth.tolist() and r.stats().rays_total == per_depth.sum()
    assert per_depth[-1] > 0                          # paths reach the last bounce
    if pb0_name:
        r0, film0 = _renderer(c, sampling=sampling, env=_env_off(with_env), lens=lens, params=(("prim_bvh", 0),))
        got0, wts0, rays0 = _render(r0, film0, calls)
        _ran(r0, pb0_name)
        assert np.array_equal(_bits(got0), _bits(got)) and np.array_equal(wts0, wts) and rays0 == rays


@pytest.mark.parametrize("sampling", [(0, 0, 0.0), (1, 1, 0.75)], ids=["plain", "jitter_rr_clamp"])
@pytest.mark.parametrize("with_env", [False, True], ids=["sky", "env"])
@pytest.mark.parametrize("name", ["C", "D", "Q_small", "Q_big"])
def test_film_equals_the_replay_bit_for_bit(monkeypatch, name, with_env, sampling):
    c = _scene(name)
    inst, abvh = _facts(name)
    _check_frame(monkeypatch, c, sampling, [4] if sampling == (0, 0, 0.0) else [1, 3], _name(False, inst, abvh, env=with_env), with_env,
                 pb0_name=_name(False, inst, False, env=with_env))


# ---- 3. lighting modes through the existing replays ---------------------------------------------------------------------------
def _lit_renderer(c, mode, name, **kw):
    with_env = name.endswith("_env")
    return _renderer(c, lighting=mode, sources="all" if c["sources"] == "all" else None,
                     env=(er.named_map(c["env"]), c["light_share"]) if with_env else None, seed=lr.SEED, **kw)


def _lit_frames(r, film):
    r.reset_stats()
    frames = lr.render_samples(r, film, lr.SAMPLES)
    r.synchronize()
    ls = r.light_stats()
    return frames, (int(ls.shadow_rays), int(ls.shadow_occluded)), [int(v) for v in r.stats().rays_per_depth]


def _check_lit(rep, name, c, r, frames):
    if name.endswith("_env"):
        rec = er.check_against_gpu(rep, frames, r.light_stats())
    elif c["sources"] == "all":
        rec = mr.check_gpu(rep, frames, r.light_stats(), r.light_info(), r.light_intervals())
        assert rec["triangle_samples"] >= 20
    else:
        rec = lr.check_against_gpu(rep, frames, r.light_stats(), r.light_info())
    assert rec["compared"] >= 0.995 * len(rep.pix)
    return rec


def _same_frames(a, b):
    for s in a[0]:
        assert np.array_equal(_bits(a[0][s]), _bits(b[0][s])), s
    assert a[1] == b[1] and a[2] == b[2]


@pytest.mark.parametrize("name", tr.INSTANCE_LIGHTING_CASES)
def test_lighting_modes_match_the_float64_replays(monkeypatch, name):
    tr.patch_walk(monkeypatch)
    c, mode, fn = tr.lighting_case(name)
    rep = fn(c, orc.OracleScene(c["scene"].desc()))
    inst, abvh = _facts(name)
    mesh, env = c["sources"] == "all", name.endswith("_env")
    r, film = _lit_renderer(c, mode, name)
    got = _lit_frames(r, film)
    _ran(r, _name(True, inst, abvh, mesh, env))
    _check_lit(rep, name, c, r, got[0])
    if abvh:      # the same case over the linear scan: another instance, the same frames
        r0, film0 = _lit_renderer(c, mode, name, params=(("prim_bvh", 0),))
        got0 = _lit_frames(r0, film0)
        _ran(r0, _name(True, inst, False, mesh, env))
        _same_frames(got0, got)


# ---- 4. textures under a thin lens --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("name", ["A", "C"])
def test_textured_film_under_a_lens_equals_the_replay_bit_for_bit(monkeypatch, name, jitter):
    c = _scene(name)
    inst, abvh = _facts(name)
    _check_frame(monkeypatch, c, (jitter, 0, 0.0), [1, 3], _name(False, inst, abvh), lens=LENS)


def test_lit_textured_frame_under_a_lens_matches_the_replay(monkeypatch):
    tr.patch_walk(monkeypatch)
    c, mode, fn = tr.lighting_case("A_mis_analytic")
    r, film = _lit_renderer(c, mode, "A_mis_analytic", lens=LENS)
    monkeypatch.setattr(lr, "primary_rays", lambda cam_desc, W, pix, rng, jitter: r.camera_rays_lens(*lp.jittered_points(pix, W, rng, jitter)))
    rep = fn(c, orc.OracleScene(c["scene"].desc()))
    got = _lit_frames(r, film)
    _ran(r, _name(True, True, False))
    _check_lit(rep, "A_mis_analytic", c, r, got[0])


# ---- 5. traversal variants under lighting -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E_mis_analytic", "bunny"])
def test_traversal_variants_under_lighting_are_bit_identical(monkeypatch, name):
    """variant 1 / 2: the paths' rays and the shadow rays of every bounce go through the closest-hit kernels of the binary tree
    and k_light_accum compares the hit with the bound (no placed copies, a host-built tree: the variant takes effect)."""
    if name == "bunny":
        c, mode = dict(lr.case("bunny", 80, 60), sources="analytic"), "mis"
        rep = lr.replay_case(c, mode)
    else:
        tr.patch_walk(monkeypatch)
        c, mode, fn = tr.lighting_case(name)
        rep = fn(c, orc.OracleScene(c["scene"].desc()))
    ref = None
    for variant in (0, 1, 2):
        r, film = _lit_renderer(c, mode, name, variant=variant)
        assert r.bvh_info().built_on_device == 0 and not c["scene"].instances
        got = _lit_frames(r, film)
        if name == "bunny":
            assert r.shade_instance() == "k_shade_nee<false, false>"
        else:
            _ran(r, _name(True, False, False))
        assert got[1][0] > 1000 and got[1][1] > 50
        if variant == 0:
            _check_lit(rep, name, c, r, got[0])
            ref = got
        else:
            _same_frames(got, ref)


# ---- 6. sorted rays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "E_mis_analytic", "bunny_jitter"])
def test_sorted_rays_give_the_same_frames(name):
    """sort_rays 1 / 2: bounces >= 1 (and a jittered bounce 0) walk their rays through a permutation (prt_sort_rays, tune.perm)."""
    ref = None
    for sort in (0, 1, 2):
        if name == "B":
            c = tr.scene_b()
            r, film = _renderer(c, params=(("sort_rays", sort),))
            got = _render(r, film, [4])
            _ran(r, _name(False, True, False))
        elif name == "bunny_jitter":
            c = lr.case("bunny", 80, 60)
            r, film = _renderer(c, sampling=(1, 0, 0.0), params=(("sort_rays", sort),))
            got = _render(r, film, [2])
            assert r.shade_instance().startswith("k_shade<")
        else:
            c, mode, _ = tr.lighting_case(name)
            r, film = _lit_renderer(c, mode, name, params=(("sort_rays", sort),))
            got = _lit_frames(r, film)
            _ran(r, _name(True, False, False))
        if ref is None:
            ref = got
            assert got[2][1] > 100        # there are rays beyond the primary ones to sort
        elif name == "E_mis_analytic":
            _same_frames(got, ref)
        else:
            assert np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]


# ---- 7. coverage --------------------------------------------------------------------------------------------------------------
def test_every_texture_instance_ran():
    """The names shade_instance() gave in the tests above (this test is the module's last and needs them all to have run)."""
    assert SEEN == ALL, (sorted(ALL - SEEN), sorted(SEEN - ALL))
