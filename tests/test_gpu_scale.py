"""Coordinate scale / offset on the GPU (-m gpu): every traversal path against the oracle's LINEAR SCAN, bit for bit, at
every case of tests/scale_cases.py (scales 2^-20 .. 2^20, offsets up to 1e5, a half-degenerate mesh, eleven orders of
magnitude in one scene, and the extreme group 2^-40 / 2^30 / 2^40).

  * closest hit and occlusion: every case x builder (host, both device builders) x node layout, six ray families
    (random, axis-parallel with exactly zero components, one component tiny, 10^3 diameters away, origins on vertices,
    origins on the lattice points next to the root's box planes); the device-built trees validate structurally;
  * frames per case (plain, jitter + roulette + clamp, the one-launch path instance), one light-sampled frame of a scaled
    emissive mesh against tests/mesh_light_replay.py;
  * placed copies at instance scales 2^-10 / 1 / 2^10 with translations up to 1e4, next to a world mesh and more than 16
    analytic primitives;
  * refits far beyond a small deformation (translate by 10^3 extents, scale by 2^8, squash onto a plane, and back).

The oracle's own BVH is not used here: it carries absolute pads and is itself untested off unit scale."""

import numpy as np
import pytest

import mesh_light_replay as mr
import scale_cases as sc
import util
from util import prt

pytestmark = pytest.mark.gpu

CONFIGS = [(b, st) for b in (0, 1, 2) for st in (None, 8)]
F = np.float32


def _renderer(scene, cam=None, W=16, H=16, depth=5, seed=5, params=()):
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=seed)
    for k, v in params:
        r.set_param(k, v)
    film = prt.Film(W, H)
    r.Init(film, scene, cam or prt.Camera(width=W, height=H))
    return r, film


def _params(builder, stride):
    return (("gpu_build", builder),) + ((("node_stride", stride),) if stride else ())


def _tmax_variants(want, diam):
    """sqrt(d2) x {1 - 2^-10, 1, 1 + 2^-10}, +inf and FLT_MAX (d2: the oracle's; for a miss the scene's diameter)."""
    with np.errstate(all="ignore"):
        base = np.where(want["prim"] >= 0, np.sqrt(want["d2"].astype(F)), F(diam)).astype(F)
        return [(base * F(1 - 2.0 ** -10)).astype(F), base, (base * F(1 + 2.0 ** -10)).astype(F),
                np.full(len(base), np.inf, F), np.full(len(base), np.finfo(F).max, F)]


def _expect_occluded(want, tmax):
    """include/prt.h: occluded iff the closest hit lies at d2 < fl32(tmax * tmax) (the product may overflow to +inf)."""
    with np.errstate(all="ignore"):
        return (want["prim"] >= 0) & (want["d2"] < (tmax * tmax).astype(F))


def _check_queries(r, o, d, want, diam, label, keep=None):
    """Closest hits and occlusion of the rays `keep` (default: all) against the oracle's `want`."""
    keep = np.ones(len(o), bool) if keep is None else keep
    got = r.closest_hit(o, d)
    bad = util.hits_equal(got[keep], want[keep])
    if bad:
        idx = np.nonzero(keep & ((got["prim"] != want["prim"]) | (got["d2"] != want["d2"])))[0]
        for i in idx[:6]:
            print(f"   {label} ray {i}: o {o[i].tolist()} d {d[i].tolist()} got {got['prim'][i]} {got['d2'][i]!r} "
                  f"want {want['prim'][i]} {want['d2'][i]!r}", flush=True)
    assert bad == [], (label, bad)
    n_occ = []
    for tmax in _tmax_variants(want, diam):
        exp = _expect_occluded(want, tmax)
        occ = r.occluded(o, d, tmax)
        for i in np.nonzero(keep & (occ != exp))[0][:6]:
            print(f"   {label} occlusion of ray {i}: o {o[i].tolist()} d {d[i].tolist()} tmax {tmax[i]!r} got {occ[i]} want {exp[i]} "
                  f"(closest hit: prim {want['prim'][i]} d2 {want['d2'][i]!r})", flush=True)
        assert np.array_equal(occ[keep], exp[keep]), (label, int((occ != exp)[keep].sum()))
        n_occ.append(int(exp.sum()))
    return n_occ, got


@pytest.mark.parametrize("name", sc.NAMES)
def test_closest_hit_and_occlusion_equal_the_linear_scan(name):
    c = sc.case(name)
    scene = sc.case_scene(c)
    fam = sc.ray_families(scene, np.random.default_rng([11, sc.NAMES.index(name)]), n=512)
    o, d = sc.all_rays(fam)
    lo, hi = sc.world_box(scene)
    diam = float(np.linalg.norm(hi - lo))
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
    shares = sc.hit_shares(fam, want)
    assert min(shares.values()) >= sc.MIN_HIT_SHARE, shares
    for builder, stride in CONFIGS:
        r, _ = _renderer(scene, params=_params(builder, stride))
        if builder and not stride:
            n8 = r.bvh_read8()
            _, tris = r.bvh_read()
            _, levels = util.check_bvh8(n8, tris)
            assert levels == r.bvh_info().depth8
        n_occ, _ = _check_queries(r, o, d, want, diam, f"{name} builder {builder} stride {stride}")
        if not builder and not stride:
            _other_kernels(r, o, d, want, name)
        del r
    print(f"{name}: {len(o)} rays x {len(CONFIGS)} configurations, hit share per family "
          + ", ".join(f"{f} {shares[f]:.2f}" for f in sc.FAMILIES) + f", occluded per tmax variant {n_occ}", flush=True)


def _other_kernels(r, o, d, want, label):
    """The walks that share the slab expressions with the 8-wide kernel, on a host-built tree: the one-thread-per-ray
    kernels over the binary tree (variants 1 and 2), the 4-wide tree's instances (wide = 1), the binary tree's persistent
    kernel (wide = 0), and the 8-wide kernel with its stack capped (most rays go through the overflow list to the 4-wide
    instance)."""
    for v in (1, 2):
        r.set_variant(v)
        assert util.hits_equal(r.closest_hit(o, d), want) == [], (label, "variant", v)
    r.set_variant(0)
    for wide, lds in ((1, 0), (1, 2), (0, 0)):
        r.set_param("wide", wide)
        r.set_param("stack_lds", lds)
        assert util.hits_equal(r.closest_hit(o, d), want) == [], (label, "wide", wide, lds)
    r.set_param("wide", 2)
    r.set_param("stack_lds", 0)
    r.set_param("stack_cap", 3)
    assert util.hits_equal(r.closest_hit(o, d), want) == [], (label, "stack_cap")
    r.set_param("stack_cap", 0)


@pytest.mark.parametrize("name", sc.NAMES)
def test_many_spheres_equal_the_linear_scan_at_every_scale(name):
    """RANDOM_BALLS_MEDIUM (409 analytic primitives: the walk over their world boxes, scan_analytic<ABVH>, with its pad
    quadratic in |o|_1) moved by every case, the extreme group included: closest hit and occlusion of rays aimed at the
    spheres (random, axis-parallel with exactly zero components, one component tiny, 10^3 diameters away), with the
    primitive tree and with the linear scan on the device, against the oracle's linear scan."""
    scene = sc.balls_scene(sc.case(name))
    fam = sc.ball_rays(scene, np.random.default_rng([29, sc.NAMES.index(name)]), n=512)
    o, d = sc.all_rays(fam)
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
    shares = sc.hit_shares(fam, want)
    assert min(shares.values()) >= sc.MIN_HIT_SHARE, shares
    for prim_bvh in (1, 0):
        r, _ = _renderer(scene, params=(("prim_bvh", prim_bvh),))
        _check_queries(r, o, d, want, 120.0 * sc.case(name)[1], f"balls {name} prim_bvh {prim_bvh}")
        del r
    print(f"balls {name}: {len(o)} rays x 2, hit share per family " + ", ".join(f"{f} {v:.2f}" for f, v in shares.items()), flush=True)


def _frame(scene, cam, W, H, spp, depth, seed, params=(), sampling=None, one_sample_calls=False):
    r, film = _renderer(scene, cam, W, H, depth, seed, params)
    sp = r.set_sampling(**sampling) if sampling else None
    if one_sample_calls:
        for _ in range(spp):
            r.ProgressiveRender()
    else:
        r.ProgressiveRender(spp)
    r.download()
    return film.accum.copy(), film.weights.copy(), int(r.stats().rays_total), sp


@pytest.mark.parametrize("name", sc.NAMES)
def test_frames_equal_the_linear_scan_oracle(name):
    """64 x 36, 2 spp, 5 segments: the plain pipeline, jitter + roulette from depth 2 + clamp, and the one-launch path
    instance (forced), each against the oracle rendering with its linear scan: accum, weights and the ray count."""
    c = sc.case(name)
    W, H, spp, depth, seed = 64, 36, 2, 5, 9
    if c[4] and c[1] < 1:   # (an analytic primitive at scale 2^-40 is below the documented bound of transforms: sky light only)
        scene = sc.case_scene(c)
        lo, hi = sc.world_box(scene)
        cam = prt.Camera(position=tuple(float(v) for v in (lo + hi) / 2 + np.array([0.0, 0.0, 2 * sc.REACH_MIN])),
                         front=(0.0, 0.0, -1.0), width=W, height=H)
    else:
        scene, cam = sc.lit_scene(c)
    osc = util.oracle_scene(scene)
    n_rays = []
    for params, sampling, one in (((), None, False), ((), dict(jitter=1, rr_depth=2, clamp=4.0), False),
                                  ((("path_kernel", 2),), None, False), ((("path_kernel", 1),), dict(jitter=1), True)):
        acc, wts, rays, sp = _frame(scene, cam, W, H, spp, depth, seed, params, sampling, one)
        a, w, n = osc.render(cam.desc(), W, H, spp=spp, max_depth=depth, seed=seed, iterative=True, use_bvh=False, n_threads=8,
                             sampling=sp)
        nbad = int((acc != a).any(axis=-1).sum())
        assert nbad == 0 and np.array_equal(wts, w) and rays == n, (name, params, sampling, nbad, rays, n)
        n_rays.append(n)
    print(f"{name}: 4 frames {W}x{H}x{spp}, rays {n_rays}", flush=True)


def test_light_sampled_frame_of_a_scaled_emissive_mesh_follows_the_replay(record_property):
    """mesh_light_replay's emissive bunny (9,999 triangle lights + a sphere light over a ground quad) scaled by 2^10: the
    light table's areas and thresholds come from the scaled vertices; every sample within that module's own tolerances."""
    c = mr.case("bunny_light", 160, 120)
    s, T = 2.0 ** 10, (0.0, 0.0, 0.0)
    c = dict(c, scene=sc.move_scene(c["scene"], s, T), cam=sc.move_camera(c["cam"], s, T))
    osc = util.oracle_scene(c["scene"])
    rep = mr.replay_case(c, "mis", osc=osc)
    film = prt.Film(c["W"], c["H"])
    r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=mr.SEED)
    r.set_light_sources("all")
    r.Init(film, c["scene"], c["cam"])
    r.set_samples_in_flight(16)
    r.set_lighting("mis")
    r.reset_stats()
    frames = mr.render_samples(r, film, mr.SAMPLES)
    r.synchronize()
    rec = mr.check_gpu(rep, frames, r.light_stats(), r.light_info(), r.light_intervals())
    record_property("scaled_mesh_light_replay", rec)
    assert rec["compared"] >= 0.995 * len(rep.pix) and rec["triangle_samples"] > 1000


@pytest.mark.parametrize("scale", [2.0 ** -10, 1.0, 2.0 ** 10])
def test_placed_copies_at_scaled_instances_equal_the_linear_scan(scale):
    """The level switch of the two-level walk: world -> local origin and direction, the local culling bound from the world
    distance (inv_scale), candidates keyed by world distance: instance scales 2^-10 / 1 / 2^10 x (0.5 .. 2), rotations,
    translations up to 1e4, beside a world mesh and 22 analytic primitives (their own walk)."""
    scene = sc.placed_scene(scale)
    fam = sc.ray_families(scene, np.random.default_rng([13, int(np.log2(scale)) + 100]), n=512)
    o, d = sc.all_rays(fam)
    lo, hi = sc.world_box(scene)
    diam = float(np.linalg.norm(hi - lo))
    osc = util.oracle_scene(scene)
    want = osc.closest_hit(o, d, use_bvh=False, n_threads=8)
    shares = sc.hit_shares(fam, want)
    assert min(shares.values()) >= sc.MIN_HIT_SHARE, shares
    W, H, spp, depth, seed = 64, 36, 2, 5, 4
    cam = prt.Camera(position=(6.0 * scale, 5.0 * scale, 12.0 * scale), width=W, height=H)
    a, w, n = osc.render(cam.desc(), W, H, spp=spp, max_depth=depth, seed=seed, iterative=True, use_bvh=False, n_threads=8)
    for builder, stride in ((0, None), (1, None), (2, 8)):
        r, film = _renderer(scene, cam, W, H, depth, seed, _params(builder, stride))
        _check_queries(r, o, d, want, diam, f"placed {scale} builder {builder}")  # (all rays)
        r.reset_stats()
        r.ProgressiveRender(spp)
        r.download()
        assert np.array_equal(film.accum, a) and np.array_equal(film.weights, w) and r.stats().rays_total == n, (scale, builder)
        del r
    print(f"placed copies at {scale}: {len(o)} rays x 3 configurations, a frame of {n} rays, hit share per family "
          + ", ".join(f"{f} {shares[f]:.2f}" for f in sc.FAMILIES), flush=True)


def _bunny(vertices):
    m = sc.asset_mesh("bunny.ply")
    scene = prt.Scene(preset=None)
    scene.AddMesh(prt.Mesh(vertices=vertices.astype(np.float32), normals=m.GetNormals(), indices=m.GetIndices()),
                  scene.AddLambertian((0.8, 0.8, 0.8)))
    return scene


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_refit_far_beyond_a_small_deformation(builder):
    """One Init, then prt_refit_meshes to: the mesh translated by 10^3 of its extent, scaled by 2^8, squashed onto the
    plane y = const, and the original again.  After every step the tree read back is valid and its boxes are the tightest
    the format allows (util.check_bvh8_tight: squashing and restoring must shrink them again), closest hits, occlusion and a
    frame equal the oracle's linear scan and a fresh Init of the same geometry, and bvh_info().refits counts the steps.

    The squashed mesh holds slivers (triangles that stood upright: areas down to 1e-7 on edges of 0.15), and from a distance
    the reference reports hits on slivers at positions the ray does not pass (4 of the 1536 rays; for the two of the far
    family the reported position is a sliver's corner 0.1 .. 0.5 units from where the ray crosses the plane, the d2 130 / 305
    below the real hit's 6.29e6): its barycentric numerators are rounding noise there (scale_cases.phantom_winners,
    DESIGN.md section 0).  No box follows those; rays whose ORACLE winner is reported farther from the ray than the per-ray
    pad, in float64, are left out of the comparison by that rule (a rule on the oracle's output alone), they are counted, printed, and may be 1 % at most."""
    v0 = sc.asset_mesh("bunny.ply").GetVertices().astype(np.float64)
    ext = float((v0.max(axis=0) - v0.min(axis=0)).max())
    flat = v0.copy()
    flat[:, 1] = 0.25
    steps = [("translated", v0 + np.array([1e3 * ext, 0.0, -1e3 * ext])), ("scaled", v0 * 2.0 ** 8), ("squashed", flat),
             ("original", v0)]
    W, H, spp, depth, seed = 64, 36, 2, 5, 6
    r, film = _renderer(_bunny(v0), prt.Camera(width=W, height=H), W, H, depth, seed, _params(builder, None))
    r.ProgressiveRender(1)  # (the renderer has worked with the old geometry)
    for k, (what, v) in enumerate(steps):
        scene = _bunny(v)
        r.Refit(scene)
        assert r.bvh_info().refits == k + 1
        n8 = r.bvh_read8()
        _, tris = r.bvh_read()
        _, levels = util.check_bvh8(n8, tris)
        assert levels == r.bvh_info().depth8
        assert util.check_bvh8_tight(n8, tris) == len(n8), what   # a refit shrinks boxes as well as it grows them
        fam = sc.ray_families(scene, np.random.default_rng([17, k]), n=256)
        o, d = sc.all_rays(fam)
        lo, hi = sc.world_box(scene)
        osc = util.oracle_scene(scene)
        want = osc.closest_hit(o, d, use_bvh=False, n_threads=8)
        shares = sc.hit_shares(fam, want)
        # per family, except origins ON the flat mesh aimed along it (the vertex family of the squashed step: every target
        # lies in the plane the ray starts in, Triangle::Intersect's divisor is 0 and the reference reports nothing)
        assert all(v >= sc.MIN_HIT_SHARE for f, v in shares.items() if not (what == "squashed" and f == "vertex")), shares
        assert (want["prim"] >= 0).mean() >= sc.MIN_HIT_SHARE
        phantom = sc.phantom_winners(scene, o, d, want)
        assert phantom.mean() <= 0.01, int(phantom.sum())
        _, got = _check_queries(r, o, d, want, float(np.linalg.norm(hi - lo)), f"refit {what} builder {builder}", keep=~phantom)
        for i in np.nonzero(phantom)[0]:
            print(f"   refit {what}: the oracle's winner of ray {i} ({sc.FAMILIES[i // 256]}) is a phantom: prim {want['prim'][i]} d2 "
                  f"{want['d2'][i]!r}; the walk reports prim {got['prim'][i]} d2 {got['d2'][i]!r}", flush=True)
        ctr = (lo + hi) / 2
        size = float((hi - lo).max())
        cam = prt.Camera(position=tuple(float(x) for x in ctr + size * np.array([1.2, 0.6, 1.9])),
                         front=tuple(float(x) for x in prt.glm_normalize(np.array([-1.2, -0.6, -1.9], np.float32))), width=W, height=H)
        r.SetCamera(cam)
        film.Clear()
        r.frame_index = 0
        r.reset_stats()
        r.ProgressiveRender(spp)
        r.download()
        a, w, n = osc.render(cam.desc(), W, H, spp=spp, max_depth=depth, seed=seed, iterative=True, use_bvh=False, n_threads=8)
        assert np.array_equal(film.accum, a) and np.array_equal(film.weights, w) and r.stats().rays_total == n, (what, builder)
        r2, film2 = _renderer(scene, cam, W, H, depth, seed, _params(builder, None))
        assert util.hits_equal(r2.closest_hit(o, d)[~phantom], want[~phantom]) == []
        r2.ProgressiveRender(spp)
        r2.download()
        assert np.array_equal(film2.accum, film.accum), (what, builder)
        del r2
        print(f"refit {what} (builder {builder}): {len(o)} rays, {(want['prim'] >= 0).mean():.2f} hit, {int(phantom.sum())} phantom winners "
              f"left out, frame of {n} rays", flush=True)
