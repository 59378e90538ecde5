"""Moving placed copies on the device (prt_set_instance_transforms): one long-lived renderer follows a sequence of motion
steps (a small jiggle, the copies exchanging places, all of them on one spot, random similarity transforms, back to the
start) by a refit or a rebuild of its top level only, and after every step its closest hits, its occlusion answers and a
jittered frame equal the oracle's linear scan of the moved description in every ray, field and pixel, and equal a fresh
renderer that got the moved description through prt_set_scene.  Scenes: tests/instance_motion.py (A: world mesh, two
instanced meshes, analytic primitives; B: 40 copies, no world mesh, coinciding boxes, three top-level levels; C: instance
scales 2^-10 / 1 / 2^10 with translations up to 1e4).  The oracle's side is computed once per (scene, step)."""
import functools

import numpy as np
import pytest

import instance_motion as im
import scale_cases as sc
import util
from util import prt
from parallelraytracing_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, DEPTH, SEED = 96, 64, 4, 5, 6
CAMS = {"A": (6.0, 5.0, 12.0), "B": (7.0, 6.0, 14.0), "C": (6.0, 5.0, 12.0)}
JITTERED = "random"   # the step whose frame runs with jitter + roulette
PRT_ERR_INVALID = 1


def _cam(name):
    return prt.Camera(position=CAMS[name], width=W, height=H)


def _sampling(step):
    return dict(jitter=1, rr_depth=2, clamp=0.0) if step == JITTERED else dict(jitter=0, rr_depth=0, clamp=0.0)


@functools.lru_cache(maxsize=None)
def _reference(name, step):
    """The oracle's side of (scene, step): the rays of the six families built on the moved scene, their closest hits by
    linear scan, and the frame.  Shared by every configuration; nothing in it is written afterwards."""
    scene = im.SCENES[name]()
    im.move(scene, im.motion(scene, step))
    fam = sc.ray_families(scene, np.random.default_rng([19, "ABC".index(name), im.STEPS.index(step)]), n=512)
    o, d = sc.all_rays(fam)
    lo, hi = sc.world_box(scene)
    osc = util.oracle_scene(scene)
    want = osc.closest_hit(o, d, use_bvh=False, n_threads=8)
    sp = capi.PrtSampling(**{k: (float(v) if k == "clamp" else int(v)) for k, v in _sampling(step).items()})
    acc, wts, rays = osc.render(_cam(name).desc(), W, H, spp=SPP, max_depth=DEPTH, seed=SEED, iterative=True, use_bvh=False, n_threads=8,
                                sampling=sp)
    for a in (o, d, want, acc, wts):
        a.setflags(write=False)
    return dict(o=o, d=d, want=want, diam=float(np.linalg.norm(hi - lo)), acc=acc, wts=wts, rays=rays, shares=sc.hit_shares(fam, want))


def _renderer(scene, name, builder=0, stride=0, depth=DEPTH, seed=SEED, sources=None):
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=seed)
    r.set_param("gpu_build", builder)
    if stride:
        r.set_param("node_stride", stride)
    if sources:
        r.set_light_sources(sources)
    film = prt.Film(W, H)
    r.Init(film, scene, _cam(name))
    return r, film


def _tmax_variants(want, diam):
    with np.errstate(all="ignore"):
        base = np.where(want["prim"] >= 0, np.sqrt(want["d2"].astype(F)), F(diam)).astype(F)
        return [(base * F(1 - 2.0 ** -10)).astype(F), base, (base * F(1 + 2.0 ** -10)).astype(F),
                np.full(len(base), np.inf, F), np.full(len(base), np.finfo(F).max, F)]


def _queries(r, ref, label):
    """Closest hits of all rays in every field, and occlusion at five tmax values by the rule of include/prt.h (occluded iff
    the closest hit lies at d2 < fl32(tmax * tmax)), against the oracle."""
    o, d, want = ref["o"], ref["d"], ref["want"]
    got = r.closest_hit(o, d)
    bad = util.hits_equal(got, want)
    for i in np.nonzero((got["prim"] != want["prim"]) | (got["d2"] != want["d2"]))[0][:6]:
        print(f"   {label} ray {i} ({sc.FAMILIES[i // 512]}): o {o[i].tolist()} d {d[i].tolist()} got {got['prim'][i]} {got['d2'][i]!r} "
              f"want {want['prim'][i]} {want['d2'][i]!r}", flush=True)
    assert bad == [], (label, bad)
    occ = []
    for tmax in _tmax_variants(want, ref["diam"]):
        with np.errstate(all="ignore"):
            exp = (want["prim"] >= 0) & (want["d2"] < (tmax * tmax).astype(F))
        occ.append(r.occluded(o, d, tmax))
        assert np.array_equal(occ[-1], exp), (label, int((occ[-1] != exp).sum()))
    return got, occ


def _frame(r, film, step):
    film.Clear()
    r.frame_index = 0
    r.set_sampling(**_sampling(step))
    r.reset_stats()
    r.ProgressiveRender(SPP)
    r.download()
    return film.accum.copy(), film.weights.copy(), int(r.stats().rays_total)


def _follow(name, mode, builder, stride):
    scene = im.SCENES[name]()
    r, film = _renderer(scene, name, builder, stride)
    tops = [r.instance_update_info().top_nodes]
    for k, step in enumerate(im.STEPS):
        ref = _reference(name, step)
        assert min(ref["shares"].values()) >= sc.MIN_HIT_SHARE, ref["shares"]
        im.move(scene, im.motion(scene, step))
        r.UpdateInstances(scene, mode)
        label = f"{name} {step} {mode} builder {builder} stride {stride}"
        info = r.instance_update_info()
        assert info.updates == k + 1 and info.last_mode == capi.INSTANCE_MODES[mode], label
        if mode == "refit":
            assert info.top_nodes == tops[0]
        tops.append(info.top_nodes)
        im.check_top_level(r, scene)   # (the host copy was read back from the device after a refit)
        got, occ = _queries(r, ref, label)
        acc, wts, rays = _frame(r, film, step)
        nbad = int((acc != ref["acc"]).any(axis=-1).sum())
        assert nbad == 0 and np.array_equal(wts, ref["wts"]) and rays == ref["rays"], (label, nbad, rays, ref["rays"])
        # a fresh renderer that got the moved description through prt_set_scene
        fr, ffilm = _renderer(scene, name, builder, stride)
        fgot, focc = _queries(fr, ref, label + " (fresh)")
        assert util.hits_equal(got, fgot) == [] and all(np.array_equal(a, b) for a, b in zip(occ, focc))
        facc, fwts, frays = _frame(fr, ffilm, step)
        assert np.array_equal(acc, facc) and np.array_equal(wts, fwts) and rays == frays, label
        if mode == "rebuild" and builder == 0:   # (the host builder is deterministic: the rebuilt scene IS the fresh one)
            assert r.kernel_instance() == fr.kernel_instance(), (label, r.kernel_instance(), fr.kernel_instance())
            assert r.bvh_info().depth8 == fr.bvh_info().depth8 and r.bvh_info().n_nodes8 == fr.bvh_info().n_nodes8, label
        del fr
    print(f"{name} {mode} builder {builder} stride {stride}: {len(ref['o'])} rays and a {W}x{H}x{SPP} frame per step, top-level nodes {tops}", flush=True)
    return tops


@pytest.mark.parametrize("stride", [0, 8])
@pytest.mark.parametrize("builder", [0, 1, 2])
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_scene_a_follows_every_motion_step(mode, builder, stride):
    _follow("A", mode, builder, stride)


@pytest.mark.parametrize("builder", [0, 1, 2])
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_scene_b_follows_every_motion_step(mode, builder):
    tops = _follow("B", mode, builder, 0)
    if mode == "rebuild" and builder == 0:   # (the rebase pass ran: the host builder's node count follows the layout)
        assert len(set(tops)) > 1, tops


@pytest.mark.parametrize("builder", [0, 1, 2])
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_scene_c_follows_every_motion_step(mode, builder):
    _follow("C", mode, builder, 0)


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_progressive_accumulation_across_an_update(mode):
    """2 samples, an update, 2 more samples: the film is not cleared, and holds the oracle's sum of both halves."""
    scene = im.scene_a()
    r, film = _renderer(scene, "A")
    r.ProgressiveRender(2)
    acc, wts, rays = util.oracle_scene(scene).render(_cam("A").desc(), W, H, spp=2, max_depth=DEPTH, seed=SEED, iterative=True, use_bvh=False,
                                                     n_threads=8)
    im.move(scene, im.motion(scene, "random"))
    r.UpdateInstances(scene, mode)
    r.ProgressiveRender(2)
    r.download()
    acc, wts, rays2 = util.oracle_scene(scene).render(_cam("A").desc(), W, H, spp=2, first_sample=2, max_depth=DEPTH, seed=SEED, iterative=True,
                                                      use_bvh=False, n_threads=8, accum=acc, weights=wts)
    assert np.array_equal(film.accum, acc) and np.array_equal(film.weights, wts) and (wts == 4).all()
    assert r.stats().rays_total == rays + rays2


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_light_sampling_follows_an_emissive_copy(mode):
    """Lighting "mis" over all sources with two emissive copies: frame, shadow-ray and occluded counts after the update are
    bit-identical to a fresh renderer's, and the light set is the fresh one's as integers."""
    scene = im.scene_a(emissive=True)
    r, film = _renderer(scene, "A", sources="all")
    r.set_lighting("mis")
    r.ProgressiveRender(1)
    im.move(scene, im.motion(scene, "random"))
    r.UpdateInstances(scene, mode)
    acc, wts, rays = _frame(r, film, "jiggle")
    fr, ffilm = _renderer(scene, "A", sources="all")
    fr.set_lighting("mis")
    facc, fwts, frays = _frame(fr, ffilm, "jiggle")
    assert np.array_equal(acc, facc) and np.array_equal(wts, fwts) and rays == frays and acc.any()
    ls, fls = r.light_stats(), fr.light_stats()
    assert (ls.shadow_rays, ls.shadow_occluded, ls.n_lights) == (fls.shadow_rays, fls.shadow_occluded, fls.n_lights) and ls.shadow_rays > 0
    assert np.array_equal(r.light_intervals(), fr.light_intervals())
    assert all(np.array_equal(a, b) for a, b in zip(r.light_info(), fr.light_info()))


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_two_rank_group_equals_the_single_context(mode):
    scene = im.scene_a()
    ref = _reference("A", "random")
    g = prt.HipWavefrontGroupRenderer([0, 0], max_depth=DEPTH, seed=SEED)
    film = prt.Film(W, H)
    g.Init(film, scene, _cam("A"))
    g.ProgressiveRender(1)
    im.move(scene, im.motion(scene, "random"))
    g.UpdateInstances(scene, mode)
    g.Clear()
    g.set_sampling(**_sampling("random"))
    g.ProgressiveRender(SPP)
    g.download()
    assert np.array_equal(film.accum, ref["acc"]) and np.array_equal(film.weights, ref["wts"]) and g.stats().rays_total >= ref["rays"]
    for rank in (0, 1):
        info = g.instance_update_info(rank)
        assert info.updates == 1 and info.last_mode == capi.INSTANCE_MODES[mode]


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_sixteen_samples_in_flight(mode):
    scene = im.scene_a()
    ref = _reference("A", "permute")
    r, film = _renderer(scene, "A", builder=1)
    r.set_samples_in_flight(16)
    r.ProgressiveRender(16)
    im.move(scene, im.motion(scene, "permute"))
    r.UpdateInstances(scene, mode)
    acc, wts, rays = _frame(r, film, "permute")
    assert np.array_equal(acc, ref["acc"]) and np.array_equal(wts, ref["wts"]) and rays == ref["rays"]


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_refusals_on_a_device_context_leave_the_frame_as_it_was(mode):
    scene = im.scene_a()
    r, film = _renderer(scene, "A", builder=1)
    im.move(scene, im.motion(scene, "jiggle"))
    r.UpdateInstances(scene, mode)
    ref = _reference("A", "jiggle")
    before = _frame(r, film, "jiggle")
    assert np.array_equal(before[0], ref["acc"])
    n8 = r.bvh_read8()
    L = capi.lib()
    n = len(scene.instances)

    def arr(edit=None):
        a = (capi.PrtInstance * n)(*scene.instances)
        if edit:
            edit(a)
        return a

    def other_mesh(a):
        a[0].mesh = 1 - a[0].mesh

    def other_material(a):
        a[3].material_id += 1

    def stretched(a):
        mat, inv = prt.make_transform((1.0, 2.0, 1.0), (0, 0, 0), (0, 0, 0))
        a[2].mat[:], a[2].inv[:] = mat.tolist(), inv.tolist()

    def wrong_inverse(a):
        a[4].inv[12] += 0.5

    for what, (a, k) in {"count": (arr(), n - 1), "mesh": (arr(other_mesh), n), "material": (arr(other_material), n),
                         "stretched": (arr(stretched), n), "inverse": (arr(wrong_inverse), n), "null": (None, n)}.items():
        assert L.prt_set_instance_transforms(r._ctx, a, k, capi.INSTANCE_MODES[mode]) == PRT_ERR_INVALID, what
    assert L.prt_set_instance_transforms(r._ctx, arr(), n, 7) == PRT_ERR_INVALID
    assert np.array_equal(r.bvh_read8(), n8) and r.instance_update_info().updates == 1
    after = _frame(r, film, "jiggle")
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    util_hits = r.closest_hit(ref["o"], ref["d"])
    assert util.hits_equal(util_hits, ref["want"]) == []


def test_update_info_reports_what_ran():
    scene = im.scene_b()
    r, _ = _renderer(scene, "B")
    i0 = r.instance_update_info()
    assert (i0.updates, i0.last_ms) == (0, 0.0) and i0.top_nodes > 1 and i0.top_depth == 3
    im.move(scene, im.motion(scene, "collapse"))
    r.UpdateInstances(scene, "refit")
    i1 = r.instance_update_info()
    assert (i1.updates, i1.last_mode, i1.top_nodes, i1.top_depth) == (1, 0, i0.top_nodes, i0.top_depth) and i1.last_ms > 0
    _, _, levels = im.check_top_level(r, scene)
    assert levels == i1.top_depth
    depth_refit = r.bvh_info().depth8
    r.UpdateInstances(scene, "rebuild")
    i2 = r.instance_update_info()
    assert (i2.updates, i2.last_mode) == (2, 1) and i2.top_nodes < i0.top_nodes and i2.top_depth < i0.top_depth
    _, _, levels = im.check_top_level(r, scene)
    assert levels == i2.top_depth and r.bvh_info().depth8 == depth_refit - (i0.top_depth - i2.top_depth)
    assert r.bvh_info().n_nodes8 == len(r.bvh_read8())
    # PrtBvhInfo's own counters are not this call's
    assert r.bvh_info().refits == 0
