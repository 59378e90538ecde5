"""Every raygen, shade and accumulate instance of a batch on one MI355X, named and held to the reference of its family.

prt_plan_route (csrc/prt_route.h) picks one instance per stage from the facts of a batch.  Renderer.batch_instances() says what
the last batch launched, stage by stage ("raygen", "shade0": bounce 0 where it differs, "shade", "accumulate"; "" for a stage
that launched nothing), recorded where run_batch launches; instance_names(stage) walks the lists of prt_route.h.  Every test here
asserts all four names after its renders; the last test holds what was seen, together with the 24 texture instances that
tests/test_gpu_texture_instances.py proves, to the whole lists: 35 raygen, 68 shade, 6 accumulate instances.

Scenes (tests/texture_replay.py with textured = False: the same geometry with no material bound to a texture): E (bunny, 3
primitives; INST false, ABVH false), B (placed copies, 2 primitives; INST true, ABVH false), C (22 primitives; ABVH true), D
(C + placed copies; both true).  "pb0": the same case with prim_bvh = 0, which takes the ABVH-false instance and is asserted
bit-identical to the frames beside it.  Frames are 40 x 30 at depth 4, four samples in calls of 1 + 3.

  instance                                   held to what                                     by which case
  k_raygen<false, false, false, true>        the oracle's film, bit for bit                   plain E_compact (and C pb0)
  k_raygen<false, false, false, false>         "                                              plain E_full_records, E_fuse, D pb0
  k_raygen<true, false, false, false>          "                                              plain E_jitter
  k_raygen<false, true, false, false>          "                                              plain E_rr_clamp, E_fuse_rr_clamp
  k_raygen<true, true, false, false>           "                                              plain E_jitter_rr_clamp, C / D jitter pb0
  k_raygen<false, true, true, false>           "                                              plain C, D
  k_raygen<true, true, true, false>            "                                              plain C / D jitter_rr_clamp
  k_shade<0, false, false, false, true>        "   (bounce 0 of the compact route)            plain E_compact
  k_shade<0, false, false, false, false>       "                                              plain E_compact, E_full_records, E_jitter
  k_shade<0, true, false, false, false>        "                                              plain E_rr_clamp, E_jitter_rr_clamp
  k_shade<1, false, false, false, false>       "   (film and ray total: fused paths advance   plain E_fuse
  k_shade<1, true, false, false, false>        "    at their own rate, no count per depth)    plain E_fuse_rr_clamp
  k_shade<0, true, false, true, false>         "                                              plain C
  k_shade<0, true, true, true, false>          "                                              plain D
  k_shade<0, true, true, false, false>         "                                              plain D pb0
  k_raygen_env<J, ABVH>, k_shade_env<INST, ABVH>   texture_replay.frame under an image, misses  env E, C (pb0), B, D (pb0), plain and
                                               from prt_environment_eval; whole film, bit for bit   jitter_rr_clamp
  k_shade_nee / _env / _mesh / _mesh_env <INST, ABVH>   lighting_replay / environment_replay / mesh_light_replay, their own   lit C_* (<false, true>; pb0 <false, false>), D_*
                                               tolerances, both modes in every family           (<true, true>; pb0 <true, false>), E_* (<false, false>)
  k_shade_nee_clus / _clus_env <INST, ABVH>,   light_cluster_replay over the device's tables    clustered E_* / C_* / B_* / D_*, untextured and
  k_shade_nee_clus_tex<INST, ABVH, ENV>                                                         textured; pb0 on C and D
  k_raygen_lens / _lens_env <J, ABVH>          texture_replay.frame over prt_camera_rays_lens   lens E, C (pb0), jitter 0 / 1, without / with an image
  k_raygen_list<J, ABVH, ENV, LENS> (16)       per pixel the fp32 ordered sum of the reference's first n(p) one-sample frames, n(p)
                                               the film weight; the reference is texture_replay.walk (= the oracle bit for bit, which
                                               the rows without image and lens also assert; with an image the frame replay of "env";
                                               with a lens the lens replay); weights, moments and info equal adaptive_replay's loop
  k_accumulate_stat<false, false>              moments = adaptive_replay.moments of the oracle's frames        statistics E
  k_accumulate_stat<false, true>               moments = adaptive_replay's loop over the reference's frames    every listed case
  k_accumulate_stat<true, false>               moments = adaptive_replay.moments of the context's own frames   statistics lit
  k_accumulate_stat<true, true>                film, weights, moments = adaptive_replay's loop over the context's own one-sample
                                               frames (only a float64 replay exists for a lit frame: the rule of
                                               test_every_pixel_equals_the_uniform_render_of_its_count); these two lit rows alone use it
  k_accumulate, k_accumulate_lit               named in every plain / env / lens and every lit case
One film per family at 37 x 29 (no multiple of a tile, a wave or a producer block), once on one context and once through a group
of three ranks on one device, both against the same reference.  UNREACHABLE is empty: every instance ran.

Figures of the first run on an MI355X (all 88 cases pass, the file in under 5 s; every bit-for-bit comparison exact, every name as
the table has it, no test exposed a defect); the lit cases (compared / left out as undecidable / worst error over tolerance / shadow
rays GPU = replay / occluded; the group's frames equal the single context's bit for bit):
  C_mis_analytic                    4800 / 0 / 0.047 / 5009 = 5009 / 727          D_mis_mesh clustered              4798 / 2 / 0.107 / 4836 = 4836 / 978
  C_nee_mesh                        4800 / 0 / 0.159 / 4981 = 4981 / 843          D_mis_mesh clustered textured     4798 / 2 / 0.109 / 4836 = 4836 / 978
  C_mis_env                         4799 / 1 / 0.177 / 5213 = 5213 / 781          E_nee_mesh_env clustered          4799 / 1 / 0.211 / 3137 = 3137 / 245
  C_nee_mesh_env                    4799 / 1 / 0.195 / 5180 = 5180 / 836          E_nee_mesh_env clustered textured 4799 / 1 / 0.214 / 3137 = 3137 / 245
  D_nee_analytic                    4800 / 0 / 0.048 / 4823 = 4823 / 767          C_nee_mesh_env clustered          4799 / 1 / 0.195 / 5195 = 5195 / 901
  D_mis_mesh                        4800 / 0 / 0.160 / 4797 = 4797 / 887          C_nee_mesh_env clustered textured 4799 / 1 / 0.195 / 5195 = 5195 / 901
  D_nee_analytic_env                4799 / 1 / 0.183 / 5078 = 5078 / 816          B_nee_mesh_env clustered          4799 / 1 / 0.220 / 3209 = 3209 / 281
  D_mis_mesh_env                    4799 / 1 / 0.183 / 5047 = 5047 / 870          B_nee_mesh_env clustered textured 4799 / 1 / 0.220 / 3209 = 3209 / 281
  E_mis_analytic                    4800 / 0 / 0.043 / 3036 = 3036 / 183          D_mis_mesh_env clustered          4799 / 1 / 0.183 / 5063 = 5063 / 935
  E_nee_mesh                        4800 / 0 / 0.050 / 3042 = 3042 / 283          D_mis_mesh_env clustered textured 4799 / 1 / 0.178 / 5063 = 5063 / 935
  E_mis_env                         4800 / 0 / 0.209 / 3118 = 3118 / 119          C_mis_analytic 37x29              4292 / 0 / 0.054 / 4592 = 4592 / 663
  E_nee_mesh_env                    4800 / 0 / 0.218 / 3121 = 3121 / 175          D_nee_analytic_env 37x29          4292 / 0 / 0.065 / 4663 = 4663 / 715
  E_nee_mesh clustered              4799 / 1 / 0.057 / 3078 = 3078 / 450          E_nee_mesh 37x29                  4292 / 0 / 0.049 / 2706 = 2706 / 268
  E_nee_mesh clustered textured     4799 / 1 / 0.052 / 3078 = 3078 / 450          D_mis_mesh_env 37x29              4292 / 0 / 0.098 / 4647 = 4647 / 768
  C_nee_mesh clustered              4798 / 2 / 0.096 / 5018 = 5018 / 956          D_mis_mesh clustered 37x29        4291 / 1 / 0.079 / 4450 = 4450 / 901
  C_nee_mesh clustered textured     4798 / 2 / 0.105 / 5018 = 5018 / 956          C_nee_mesh_env clustered 37x29    4290 / 2 / 0.097 / 4785 = 4785 / 775
  B_mis_mesh clustered              4798 / 2 / 0.046 / 3051 = 3051 / 437          D_mis_mesh_env clus. textured 37x29 4291 / 1 / 0.098 / 4658 = 4658 / 809
  B_mis_mesh clustered textured     4798 / 2 / 0.046 / 3051 = 3051 / 437"""
import numpy as np
import pytest

import adaptive_replay as ar
import batch_instance_cases as bc
import environment_replay as er
import lens_replay as lp
import light_cluster_replay as lcr
import lighting_replay as lr
import mesh_light_replay as mr
import texture_replay as tr
from test_gpu_texture_instances import ALL as TEXTURED
from util import orc, prt

pytestmark = pytest.mark.gpu
F = np.float32
B = ("false", "true")
STAGES = ("raygen", "shade0", "shade", "accumulate")
SEEN = {st: set() for st in STAGES}   # what batch_instances() answered after the renders of this module
UNREACHABLE = {}                      # instance -> why no legal state of the API launches it (none)
ENV_OFF = "5x3"                       # the image of the frames without light sampling (environment_replay.named_map)
LENS = (0.9, 0.15, 5.0)
PLAIN, JRC = (0, 0, 0.0), (1, 1, 0.75)
ADAPT = (4, 4, 12, 0.01)              # min, step, max samples and the noise floor of the listed cases
K = 8                                 # clusters


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _ran(r, raygen, shade, accumulate, shade0=""):
    got = r.batch_instances()
    for st in STAGES:
        SEEN[st].add(got[st])
    assert got == dict(raygen=raygen, shade0=shade0, shade=shade, accumulate=accumulate), got
    return got


def _renderer(c, sif=4, sampling=None, lighting=None, sources=None, env=None, params=(), seed=tr.SEED, lens=None, selection=None,
              group=False, stats=False):
    film = prt.Film(c["W"], c["H"])
    if group:
        r = prt.HipWavefrontGroupRenderer([0, 0, 0], max_depth=c["depth"], seed=seed)
    else:
        r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=seed)
    for k, v in params:
        r.set_param(k, v)
    if sources:
        r.set_light_sources(sources)
    if selection:
        r.set_light_selection(selection, K)
    if env is not None:
        r.set_environment(env[0], env[1])
    if lens:
        r.set_lens(*lens)
    r.Init(film, c["scene"], c["cam"])
    r.set_samples_in_flight(sif)
    if sampling and tuple(sampling) != PLAIN:
        r.set_sampling(*sampling)
    if lighting:
        r.set_lighting(lighting)
    if stats:
        r.set_film_statistics(True)
    return r, film


def _render(r, film, calls):
    for k in calls:
        r.ProgressiveRender(k)
    r.download()
    return film.accum.copy(), film.weights.copy(), [int(v) for v in r.stats().rays_per_depth]


def _env_off(on):
    return (er.named_map(ENV_OFF), 0.5) if on else None


def _patch_reference(monkeypatch, r, with_env, lens):
    """The frame replay takes what only the device can settle from the device's own function-level entry points (each held to
    its float64 contract by a test of its own): the lookup of a missing ray's direction, the lens rays."""
    if with_env:
        monkeypatch.setattr(tr, "MISS_RGB", lambda d: r.environment_eval(d)["rgb"])
    if lens:
        monkeypatch.setattr(lr, "primary_rays", lambda cam_desc, W, pix, rng, jitter: r.camera_rays_lens(*lp.jittered_points(pix, W, rng, jitter)))


def _oracle_film(c, osc, spp, sampling, first=0):
    sp = prt.capi.PrtSampling(int(sampling[0]), int(sampling[1]), float(sampling[2])) if tuple(sampling) != PLAIN else None
    return osc.render(c["cam"].desc(), c["W"], c["H"], spp=spp, first_sample=first, max_depth=c["depth"], seed=tr.SEED, iterative=True,
                      use_bvh=True, n_threads=lr.n_threads_default(), sampling=sp)


# ---- 0. the two queries -------------------------------------------------------------------------------------------------------
def test_the_queries_answer_before_a_batch_past_the_end_and_on_the_path_route():
    names = {st: prt.instance_names(st) for st in STAGES}
    assert [len(names[st]) for st in STAGES] == [35, 68, 68, 6] and names["shade0"] == names["shade"]
    assert all(len(set(v)) == len(v) and "" not in v for v in names.values())
    buf = prt.capi.C.create_string_buffer(96)
    L = prt.capi.lib()
    for st, n in (("raygen", 35), ("shade", 68), ("accumulate", 6)):
        assert L.prt_instance_name(prt.capi.STAGES[st], n - 1, buf, 96) == 0 and buf.value.decode() == names[st][-1]
        assert L.prt_instance_name(prt.capi.STAGES[st], n, buf, 96) != 0
    assert L.prt_instance_name(4, 0, buf, 96) != 0
    c = bc.scene("E")
    r, film = _renderer(c, params=(("path_kernel", 2),))
    assert r.batch_instances() == dict(raygen="", shade0="", shade="", accumulate="") and r.shade_instance() == ""
    assert L.prt_batch_instance(r._ctx, 4, buf, 96) != 0
    path = _render(r, film, [1, 3])
    assert r.batch_instances() == dict(raygen="", shade0="", shade="", accumulate="k_accumulate") and r.shade_instance() == ""
    want = _oracle_film(c, orc.OracleScene(c["scene"].desc()), 4, PLAIN)
    assert np.array_equal(_bits(path[0]), _bits(want[0])) and r.stats().rays_total == want[2]
    r.set_param("path_kernel", 0)      # prt_shade_instance keeps its meaning: the last shade launched
    r.ProgressiveRender(2)
    assert r.shade_instance() == r.batch_instances()["shade"] == "k_shade<0, false, false, false, false>"
    r.synchronize()


# ---- 1. k_shade and k_raygen against the oracle ---------------------------------------------------------------------------------
RG, SH = "k_raygen<%s>", "k_shade<%s>"
PLAIN_CASES = {
    # id: (scene, sampling, params, (raygen, shade0, shade), the same with prim_bvh = 0 or None)
    "E_compact": ("E", PLAIN, (), (RG % "false, false, false, true", SH % "0, false, false, false, true", SH % "0, false, false, false, false"), None),
    "E_full_records": ("E", PLAIN, (("compact_primary", 0),), (RG % "false, false, false, false", "", SH % "0, false, false, false, false"), None),
    "E_jitter": ("E", (1, 0, 0.0), (), (RG % "true, false, false, false", "", SH % "0, false, false, false, false"), None),
    "E_rr_clamp": ("E", (0, 1, 0.75), (), (RG % "false, true, false, false", "", SH % "0, true, false, false, false"), None),
    "E_jitter_rr_clamp": ("E", JRC, (), (RG % "true, true, false, false", "", SH % "0, true, false, false, false"), None),
    "E_fuse": ("E", PLAIN, (("fuse", 1),), (RG % "false, false, false, false", "", SH % "1, false, false, false, false"), None),
    "E_fuse_rr_clamp": ("E", (0, 1, 0.75), (("fuse", 1),), (RG % "false, true, false, false", "", SH % "1, true, false, false, false"), None),
    "C": ("C", PLAIN, (), (RG % "false, true, true, false", "", SH % "0, true, false, true, false"),
          (RG % "false, false, false, true", SH % "0, false, false, false, true", SH % "0, false, false, false, false")),
    "C_jitter_rr_clamp": ("C", JRC, (), (RG % "true, true, true, false", "", SH % "0, true, false, true, false"),
                          (RG % "true, true, false, false", "", SH % "0, true, false, false, false")),
    "D": ("D", PLAIN, (), (RG % "false, true, true, false", "", SH % "0, true, true, true, false"),
          (RG % "false, false, false, false", "", SH % "0, true, true, false, false")),
    "D_jitter_rr_clamp": ("D", JRC, (), (RG % "true, true, true, false", "", SH % "0, true, true, true, false"),
                          (RG % "true, true, false, false", "", SH % "0, true, true, false, false")),
}


def _check_plain(c, sampling, params, names, pb0, group=False):
    osc = orc.OracleScene(c["scene"].desc())
    want = _oracle_film(c, osc, 4, sampling)
    fused = ("fuse", 1) in params
    r, film = _renderer(c, sampling=sampling, params=params, group=group)
    got, wts, rays = _render(r, film, [1, 3])
    _ran(r, names[0], names[2], "k_accumulate", shade0=names[1])
    bad = np.nonzero((_bits(got) != _bits(want[0])).any(2))
    assert len(bad[0]) == 0, (c["name"], sampling, len(bad[0]), got[bad][:3], want[0][bad][:3])
    assert np.array_equal(wts, want[1]) and r.stats().rays_total == want[2] and rays[0] == 4 * c["W"] * c["H"]
    if not fused:      # the segments per depth: the walker's, whose film is the oracle's
        acc, _, per_depth = tr.frame(c["scene"], osc, c["cam"], c["W"], c["H"], c["depth"], tr.SEED, 0, 4, sampling)
        assert np.array_equal(_bits(acc), _bits(want[0]))
        assert rays[:c["depth"]] == per_depth.tolist() and per_depth[-1] > 0
    if pb0:
        r0, film0 = _renderer(c, sampling=sampling, params=tuple(params) + (("prim_bvh", 0),), group=group)
        got0, wts0, rays0 = _render(r0, film0, [1, 3])
        _ran(r0, pb0[0], pb0[2], "k_accumulate", shade0=pb0[1])
        assert np.array_equal(_bits(got0), _bits(got)) and np.array_equal(wts0, wts) and rays0 == rays


@pytest.mark.parametrize("case", sorted(PLAIN_CASES))
def test_plain_film_equals_the_oracle_bit_for_bit(case):
    name, sampling, params, names, pb0 = PLAIN_CASES[case]
    _check_plain(bc.scene(name), sampling, params, names, pb0)


# ---- 2. frames under an image, under a lens, and both -----------------------------------------------------------------------------
def _frame_names(name, sampling, with_env, lens, abvh):
    """(raygen, shade) of a lighting-off frame under an image and / or a lens"""
    inst = bc.facts(name)[0]
    j, sa = B[sampling[0] != 0], sampling[1] != 0 or sampling[2] > 0
    if lens:
        raygen = f"k_raygen_lens{'_env' if with_env else ''}<{j}, {B[abvh]}>"
    else:
        raygen = f"k_raygen_env<{j}, {B[abvh]}>"
    if with_env:
        return raygen, f"k_shade_env<{B[inst]}, {B[abvh]}>"
    assert not inst
    return raygen, SH % ("0, true, false, true, false" if abvh else f"0, {B[sa]}, false, false, false")


def _check_frame(monkeypatch, c, name, sampling, with_env=False, lens=None, group=False, pb0=True):
    abvh = bc.facts(name)[1]
    r, film = _renderer(c, sampling=sampling, env=_env_off(with_env), lens=lens)
    _patch_reference(monkeypatch, r, with_env, lens)
    osc = orc.OracleScene(c["scene"].desc())
    want, wwts, per_depth = tr.frame(c["scene"], osc, c["cam"], c["W"], c["H"], c["depth"], tr.SEED, 0, 4, sampling)
    assert per_depth[-1] > 0                          # paths reach the last bounce
    for pb in ([1, 0] if abvh and pb0 else [1]):
        for grp in ([False, True] if group else [False]):
            if pb == 1 and not grp:
                rr, ff = r, film
            else:
                rr, ff = _renderer(c, sampling=sampling, env=_env_off(with_env), lens=lens, group=grp, params=() if pb else (("prim_bvh", 0),))
            got, wts, rays = _render(rr, ff, [1, 3])
            raygen, shade = _frame_names(name, sampling, with_env, lens, abvh and pb == 1)
            _ran(rr, raygen, shade, "k_accumulate")
            bad = np.nonzero((_bits(got) != _bits(want)).any(2))
            assert len(bad[0]) == 0, (c["name"], pb, grp, sampling, len(bad[0]), got[bad][:3], want[bad][:3])
            assert np.array_equal(wts, wwts)
            assert rays[:c["depth"]] == per_depth.tolist() and rr.stats().rays_total == per_depth.sum()


@pytest.mark.parametrize("sampling", [PLAIN, JRC], ids=["plain", "jitter_rr_clamp"])
@pytest.mark.parametrize("name", ["E", "C", "B", "D"])
def test_film_under_an_image_equals_the_replay_bit_for_bit(monkeypatch, name, sampling):
    _check_frame(monkeypatch, bc.scene(name), name, sampling, with_env=True)


@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("with_env", [False, True], ids=["sky", "env"])
@pytest.mark.parametrize("name", ["E", "C"])
def test_film_under_a_lens_equals_the_replay_bit_for_bit(monkeypatch, name, with_env, jitter):
    _check_frame(monkeypatch, bc.scene(name), name, (jitter, 0, 0.0), with_env=with_env, lens=LENS)


# ---- 3. the lighting modes through the float64 replays ------------------------------------------------------------------------------
def _lit_names(name, abvh, clustered=False, textured=False):
    inst = bc.facts(name)[0]
    mesh, env = "mesh" in name, name.endswith("_env")
    ia = f"{B[inst]}, {B[abvh]}"
    raygen = f"k_raygen_env<false, {B[abvh]}>" if env else RG % ("false, true, true, false" if abvh else "false, false, false, false")
    if clustered and textured:
        return raygen, f"k_shade_nee_clus_tex<{ia}, {B[env]}>"
    if clustered:
        return raygen, f"k_shade_nee_clus{'_env' if env else ''}<{ia}>"
    assert not textured
    return raygen, f"k_shade_nee{'_mesh' if mesh else ''}{'_env' if env else ''}<{ia}>"


def _lit_renderer(c, mode, name, clustered=False, **kw):
    with_env = name.endswith("_env")
    return _renderer(c, lighting=mode, sources="all" if c["sources"] == "all" else None, selection="clustered" if clustered else None,
                     env=(er.named_map(c["env"]), c["light_share"]) if with_env else None, seed=lr.SEED, **kw)


def _lit_frames(r, film, group=False):
    if not group:
        r.reset_stats()
    frames = lr.render_samples(r, film, lr.SAMPLES, clear=r.Clear if group else None)
    ls = r.light_stats()
    return frames, (int(ls.shadow_rays), int(ls.shadow_occluded)), [int(v) for v in r.stats().rays_per_depth]


def _check_lit(rep, name, c, frames, light_stats, light_info, intervals):
    if name.endswith("_env"):
        rec = er.check_against_gpu(rep, frames, light_stats)
    elif c["sources"] == "all":
        rec = mr.check_gpu(rep, frames, light_stats, light_info, intervals)
        assert rec["triangle_samples"] >= 20
    else:
        rec = lr.check_against_gpu(rep, frames, light_stats, light_info)
    assert rec["compared"] >= 0.995 * len(rep.pix) and rep.stable.mean() >= 0.995
    return rec


def _same_frames(a, b):
    for s in a[0]:
        assert np.array_equal(_bits(a[0][s]), _bits(b[0][s])), s
    assert a[1] == b[1] and a[2] == b[2]


def _check_lit_case(monkeypatch, name, clustered=False, textured=False, odd=False, group=False):
    if textured:
        tr.patch_walk(monkeypatch)
    c, mode, fn = bc.lit_case(name, textured=textured, odd=odd)
    assert bool(c["scene"].material_texture) == textured
    abvh = bc.facts(name)[1]
    osc = orc.OracleScene(c["scene"].desc())
    r, film = _lit_renderer(c, mode, name, clustered)
    if clustered:
        assert r.light_cluster_info().active == 1
        tables = lcr.read_tables(r)
        with lcr.clustered(tables):
            rep = fn(c, osc)
    else:
        rep = fn(c, osc)
    got = _lit_frames(r, film)
    _ran(r, *_lit_names(name, abvh, clustered, textured), "k_accumulate_lit")
    if name.endswith("_env") and clustered:
        assert r.environment_info().t_env == int(rep.t_env) and rep.t_env > 0
    info = r.light_info()
    intervals = r.light_intervals() if c["sources"] == "all" else None
    rec = _check_lit(rep, name, c, got[0], r.light_stats(), info, intervals)
    print("FIGURES", name, "clustered" if clustered else "power", "textured" if textured else "plain", (c["W"], c["H"]), rec, flush=True)
    if abvh and not odd:      # the same case over the linear scan: another instance, the same frames
        r0, film0 = _lit_renderer(c, mode, name, clustered, params=(("prim_bvh", 0),))
        got0 = _lit_frames(r0, film0)
        _ran(r0, *_lit_names(name, False, clustered, textured), "k_accumulate_lit")
        _same_frames(got0, got)
    if group:
        g, gfilm = _lit_renderer(c, mode, name, clustered, group=True)
        if clustered:
            gt = lcr.read_tables(g)
            assert all(np.array_equal(tables[k], gt[k]) for k in tables)
        gg = _lit_frames(g, gfilm, group=True)
        _ran(g, *_lit_names(name, abvh, clustered, textured), "k_accumulate_lit")
        _check_lit(rep, name, c, gg[0], g.light_stats(), g.light_info(), intervals)
        _same_frames(gg, got)


@pytest.mark.parametrize("name", bc.LIT_CASES)
def test_lighting_modes_match_the_float64_replays(monkeypatch, name):
    _check_lit_case(monkeypatch, name)


@pytest.mark.parametrize("textured", [False, True], ids=["plain", "textured"])
@pytest.mark.parametrize("name", bc.CLUSTER_CASES)
def test_clustered_selection_matches_the_float64_replay(monkeypatch, name, textured):
    _check_lit_case(monkeypatch, name, clustered=True, textured=textured)


# ---- 4. listed batches and the statistics ---------------------------------------------------------------------------------------------
def _sample_frames(c, osc, n, sampling):
    """The reference's one-sample frames 0 .. n - 1 (texture_replay.walk, whatever _patch_reference put in place)."""
    W, H = c["W"], c["H"]
    pix = np.arange(W * H)
    _, delivered, _, _ = tr.walk(c["scene"], osc, c["cam"], W, H, c["depth"], tr.SEED, np.tile(pix, n), np.repeat(np.arange(n), len(pix)), sampling, True)
    return [delivered[s * len(pix):(s + 1) * len(pix)].reshape(H, W, 3).copy() for s in range(n)]


def _check_adaptive(c, r, film, frames, names, lit=False):
    """One adaptive frame of renderer r against adaptive_replay's loop over `frames`, and per pixel against the fp32 ordered sum
    of its first n(p) frames, n(p) the film weight."""
    W, H = c["W"], c["H"]
    mn, step, mx, floor = ADAPT
    thr, n_stop, n_go = bc.split_threshold(frames, W, H, mn, floor)
    rp = ar.Replay(W, H, lambda s: frames[s])
    want = rp.run(mn, step, mx, thr, floor)
    info = r.render_adaptive(thr, mn, step, mx, floor)
    r.download()
    _ran(r, names[0], names[1], f"k_accumulate_stat<{B[lit]}, true>")
    wts = film.weights
    per_tile = np.array([wts[y0, x0] for x0, y0, x1, y1 in ar.tiles(W, H)])
    assert (per_tile == mn).sum() == n_stop > 0 and (per_tile > mn).sum() == n_go > 0      # a proper, non-empty subset stopped early
    cum, ordered = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
    for s in range(mx):
        cum += frames[s]
        ordered[wts == s + 1] = cum[wts == s + 1]
    assert set(np.unique(wts).tolist()) <= {float(mn + k * step) for k in range((mx - mn) // step + 1)}
    bad = np.nonzero((_bits(film.accum) != _bits(ordered)).any(2))
    assert len(bad[0]) == 0, (c["name"], len(bad[0]), film.accum[bad][:3], ordered[bad][:3], wts[bad][:3])
    assert np.array_equal(wts, rp.count_map(want["counts"])) and np.array_equal(_bits(film.accum), _bits(rp.accum))
    A, Q = r.film_statistics()
    assert np.array_equal(_bits(A), _bits(rp.A)) and np.array_equal(_bits(Q), _bits(rp.Q))
    if isinstance(r, prt.HipWavefrontRenderer):
        assert ar.info_dict(info) == ar.replay_info(want)
        assert r.stats().rays_per_depth[0] == int(wts.sum()) == info.pixel_samples
    return wts


def _check_listed(monkeypatch, c, name, jitter, with_env, lens, group=False):
    abvh = bc.facts(name)[1]
    sampling = (jitter, 0, 0.0)
    r, film = _renderer(c, sampling=sampling, env=_env_off(with_env), lens=LENS if lens else None, stats=True)
    _patch_reference(monkeypatch, r, with_env, lens)
    osc = orc.OracleScene(c["scene"].desc())
    frames = _sample_frames(c, osc, ADAPT[2], sampling)
    if not with_env and not lens:       # the walker's frames are the oracle's
        for s in (0, ADAPT[2] - 1):
            assert np.array_equal(_bits(frames[s]), _bits(_oracle_film(c, osc, 1, sampling, first=s)[0])), s
    shade = f"k_shade_env<false, {B[abvh]}>" if with_env else SH % ("0, true, false, true, false" if abvh else "0, false, false, false, false")
    names = (f"k_raygen_list<{B[jitter]}, {B[abvh]}, {B[with_env]}, {B[lens]}>", shade)
    wts = _check_adaptive(c, r, film, frames, names)
    if group:
        g, gfilm = _renderer(c, sampling=sampling, env=_env_off(with_env), lens=LENS if lens else None, stats=True, group=True)
        gw = _check_adaptive(c, g, gfilm, frames, names)
        assert np.array_equal(gw, wts)


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("with_env", [False, True], ids=["sky", "env"])
@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("name", ["E", "C"])
def test_listed_batches_add_each_pixel_its_first_samples_in_order(monkeypatch, name, jitter, with_env, lens):
    _check_listed(monkeypatch, bc.scene(name), name, jitter, with_env, lens)


def _own_frames(r, film, n):
    """The context's own one-sample frames 0 .. n - 1 (a cleared film plus one sample is that sample, exactly)."""
    frames = lr.render_samples(r, film, range(n))
    film.Clear()
    r.frame_index = 0
    r.reset_stats()
    return [frames[s] for s in range(n)]


def test_statistics_of_a_uniform_render_equal_the_restatement():
    """k_accumulate_stat<false, false> against the moments of the oracle's frames, <true, false> against those of the context's
    own one-sample frames (each held to the float64 replay by test_lighting_modes_match_the_float64_replays)."""
    c = bc.scene("E")
    osc = orc.OracleScene(c["scene"].desc())
    r, film = _renderer(c, stats=True)
    got, wts, _ = _render(r, film, [1, 3])
    _ran(r, RG % "false, false, false, true", SH % "0, false, false, false, false", "k_accumulate_stat<false, false>",
         shade0=SH % "0, false, false, false, true")
    oframes = [_oracle_film(c, osc, 1, PLAIN, first=s)[0] for s in range(4)]
    A, Q = ar.moments(oframes)
    gA, gQ = r.film_statistics()
    assert np.array_equal(_bits(gA), _bits(A)) and np.array_equal(_bits(gQ), _bits(Q)) and (Q > 0).any()
    assert np.array_equal(_bits(got), _bits(_oracle_film(c, osc, 4, PLAIN)[0]))
    c, mode, _ = bc.lit_case("E_mis_analytic")
    r, film = _lit_renderer(c, mode, "E_mis_analytic", stats=True)
    frames = _own_frames(r, film, 4)
    got, wts, _ = _render(r, film, [1, 3])
    _ran(r, RG % "false, false, false, false", "k_shade_nee<false, false>", "k_accumulate_stat<true, false>")
    A, Q = ar.moments(frames)
    gA, gQ = r.film_statistics()
    assert np.array_equal(_bits(gA), _bits(A)) and np.array_equal(_bits(gQ), _bits(Q)) and (Q > 0).any()
    assert (wts == 4).all() and np.array_equal(_bits(got), _bits(frames[0] + frames[1] + frames[2] + frames[3]))


@pytest.mark.parametrize("name", ["E_mis_analytic", "D_mis_mesh_env"])
def test_listed_lit_batches_equal_the_loop_over_the_contexts_own_frames(name):
    """k_accumulate_stat<true, true>: only a float64 replay exists for a lit frame, so every pixel is held to the fp32 ordered sum
    of the context's own one-sample frames (the uniform render of its count), as
    test_gpu_adaptive.test_every_pixel_equals_the_uniform_render_of_its_count does."""
    c, mode, _ = bc.lit_case(name)
    abvh = bc.facts(name)[1]
    r, film = _lit_renderer(c, mode, name, stats=True)
    frames = _own_frames(r, film, ADAPT[2])
    raygen = f"k_raygen_list<false, {B[abvh]}, {B[name.endswith('_env')]}, false>"
    _check_adaptive(c, r, film, frames, (raygen, _lit_names(name, abvh)[1]), lit=True)
    assert r.light_stats().shadow_rays > 0


# ---- 5. one film per family at 37 x 29, on one context and through a group of three ranks ------------------------------------------------
def _odd(name):
    return bc.resized(bc.scene(name), bc.ODD)


def test_odd_film_plain_and_group():
    name, sampling, params, names, pb0 = PLAIN_CASES["E_compact"]
    for group in (False, True):
        _check_plain(_odd(name), sampling, params, names, None, group=group)
    name, sampling, params, names, pb0 = PLAIN_CASES["D_jitter_rr_clamp"]
    for group in (False, True):
        _check_plain(_odd(name), sampling, params, names, None, group=group)


@pytest.mark.parametrize("name,with_env,lens,jitter", [("C", True, None, 0), ("C", False, LENS, 1), ("D", True, LENS, 1)], ids=["env", "lens", "lens_env"])
def test_odd_film_under_an_image_and_a_lens_and_group(monkeypatch, name, with_env, lens, jitter):
    _check_frame(monkeypatch, _odd(name), name, (jitter, 0, 0.0), with_env=with_env, lens=lens, group=True, pb0=False)


def test_odd_film_listed_and_group(monkeypatch):
    _check_listed(monkeypatch, _odd("C"), "C", 1, False, False, group=True)


@pytest.mark.parametrize("name", bc.ODD_LIT_CASES)
def test_odd_film_lighting_modes_and_group(monkeypatch, name):
    _check_lit_case(monkeypatch, name, odd=True, group=True)


@pytest.mark.parametrize("name,textured", bc.ODD_CLUSTER_CASES, ids=[n + ("_textured" if t else "") for n, t in bc.ODD_CLUSTER_CASES])
def test_odd_film_clustered_selection_and_group(monkeypatch, name, textured):
    _check_lit_case(monkeypatch, name, clustered=True, textured=textured, odd=True, group=True)


# ---- 6. the census ------------------------------------------------------------------------------------------------------------------
def test_every_instance_ran():
    """Per stage, the names batch_instances() gave in the tests above, with the 24 texture instances that
    tests/test_gpu_texture_instances.py proves, are the library's whole list (this test is the module's last and needs them all
    to have run).  Bounce 0's own instance is reported as "shade0" and counts for the shade list."""
    assert UNREACHABLE == {}
    seen = {"raygen": SEEN["raygen"], "shade": SEEN["shade"] | SEEN["shade0"] | TEXTURED, "accumulate": SEEN["accumulate"]}
    for st, got in seen.items():
        every = set(prt.instance_names(st))
        got = got - {""}
        assert got == every, (st, sorted(every - got), sorted(got - every))
    assert TEXTURED <= set(prt.instance_names("shade")) and len(TEXTURED) == 24
    assert SEEN["shade0"] == {"", SH % "0, false, false, false, true"}
