"""GPU tests of the occlusion query (prt_occluded / prt_occluded_device) and the device closest-hit form.

Expected values: the oracle's closest hit plus the contract
    occluded[i] = tmax[i] > 0 and closest_hit(ray i).prim >= 0 and closest_hit(ray i).d2 < fl32(tmax[i] * tmax[i])
compared with exact equality.  The any-hit walk may stop at any blocker, so this equality is what pins it."""
import numpy as np
import pytest

import util
from util import prt
from test_gpu_parity import INST_PLACEMENTS, _instanced_scene, _mesh_rays, make_renderer  # noqa: F401

pytestmark = pytest.mark.gpu


def contract(want, tmax, dirs):
    t = np.asarray(tmax, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t2 = (t * t).astype(np.float32)
        live = (t > 0) & ~(dirs == 0).all(axis=1)
        return live & (want["prim"] >= 0) & (want["d2"] < t2)


def tmax_mix(rng, want):
    """+inf, 0, negative, NaN, random values, and sqrt(d2) of the closest hit with its two fp32 neighbours."""
    n = want.shape[0]
    t = rng.uniform(0.05, 25.0, n).astype(np.float32)
    kind = rng.integers(0, 9, n)
    with np.errstate(over="ignore"):
        hd = np.sqrt(want["d2"].astype(np.float32)).astype(np.float32)
    t[kind == 0] = np.inf
    t[kind == 1] = 0.0
    t[kind == 2] = -rng.uniform(0.0, 5.0, (kind == 2).sum()).astype(np.float32)
    t[kind == 3] = np.nan
    t[kind == 4] = hd[kind == 4]
    t[kind == 5] = np.nextafter(hd[kind == 5], np.float32(np.inf))
    t[kind == 6] = np.nextafter(hd[kind == 6], np.float32(0))
    return t


def check(r, o, d, t, want, what=""):
    got = r.occluded(o, d, t)
    exp = contract(want, t, d)
    assert got.dtype == bool and got.shape == exp.shape
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (what, bad[:10], got[bad[:10]], exp[bad[:10]], t[bad[:10]], want["d2"][bad[:10]])
    return got


def boundary_rays(want):
    """tmax exactly at and beside every hit's distance: the strict < of the contract."""
    hd = np.sqrt(want["d2"].astype(np.float32)).astype(np.float32)
    return hd, np.nextafter(hd, np.float32(np.inf)), np.nextafter(hd, np.float32(0))


@pytest.mark.parametrize("preset", util.PRESETS + ["RANDOM_BALLS_LARGE"])
def test_occluded_presets_exact(preset):
    scene = prt.Scene(preset)
    r, _, cam = make_renderer(scene, 64, 48)
    rng = np.random.default_rng(abs(hash(preset)) % 997)
    o1, d1 = util.random_rays(rng, 3000, center=(0, 1, 0), radius=14.0, spread=6.0)
    o2 = rng.uniform(-4, 4, size=(2000, 3)).astype(np.float32)  # many of them start inside spheres
    o2[:, 1] = np.abs(o2[:, 1])
    d2 = np.stack([prt.glm_normalize(v) for v in rng.normal(size=o2.shape).astype(np.float32)])
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    d[::97] = 0.0  # zero directions: dead rays
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False)
    assert (want["prim"] >= 0).sum() > 500
    got = check(r, o, d, tmax_mix(rng, want), want, preset)
    assert got.sum() > 100
    for t in boundary_rays(want):
        check(r, o, d, t, want, preset)
    check(r, o, d, np.float32(np.inf) + np.zeros(len(o), np.float32), want, preset)


@pytest.mark.parametrize("gpu_build", [0, 1])
def test_occluded_refined_bunny_host_and_device_built_trees(gpu_build):
    mesh = prt.scenes.refined("bunny.ply", 30_000)
    scene = prt.scenes.mesh_scene(mesh)
    r = prt.HipWavefrontRenderer(device=0)
    r.set_param("gpu_build", gpu_build)
    r.Init(prt.Film(16, 16), scene, prt.Camera(width=16, height=16))
    assert r.bvh_info().built_on_device == gpu_build
    rng = np.random.default_rng(40 + gpu_build)
    o, d = _mesh_rays(rng, 20000)
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=True, n_threads=8)
    assert (want["prim"] >= 2).sum() > 2000
    check(r, o, d, tmax_mix(rng, want), want)
    for t in boundary_rays(want):
        check(r, o, d, t, want)


def _c3():
    scene, cam, W, H, spp, depth = prt.scenes.config("C3")
    r, _, _ = make_renderer(scene, 64, 36, cam=prt.Camera(cam.position, width=64, height=36))
    return scene, r


def _shadow_rays(r, rng, n, light=(2.0, 6.0, 3.0)):
    """Hit points of camera rays on the C3 scene, rays toward a point light, tmax = distance * (1 - 1e-4)."""
    o, d = r.camera_rays(rng.uniform(0, 64, n).astype(np.float32), rng.uniform(0, 36, n).astype(np.float32))
    h = r.closest_hit(o, d)
    m = h["prim"] >= 0
    p = h["position"][m].astype(np.float32)
    v = (np.asarray(light, np.float32) - p).astype(np.float32)
    dist = np.sqrt((v * v).sum(axis=1)).astype(np.float32)
    sd = np.stack([prt.glm_normalize(x) for x in v]).astype(np.float32)
    return p, sd, (dist * np.float32(1 - 1e-4)).astype(np.float32), h[m]


def test_occluded_full_size_mesh_and_shadow_rays_exact():
    scene, r = _c3()
    rng = np.random.default_rng(12)
    o, d = _mesh_rays(rng, 20000)
    osc = util.oracle_scene(scene)
    want = osc.closest_hit(o, d, use_bvh=True, n_threads=8)
    check(r, o, d, tmax_mix(rng, want), want, "C3 random")
    p, sd, tmax, _ = _shadow_rays(r, rng, 12000)
    want = osc.closest_hit(p, sd, use_bvh=True, n_threads=8)
    got = check(r, p, sd, tmax, want, "C3 shadow rays")
    assert 0 < got.sum() < len(got)
    check(r, p, sd, np.full(len(p), np.inf, np.float32), want, "C3 shadow rays, tmax = inf")
    # every walk the scene can select answers the same: the 8-wide instances, the 4-wide and binary trees, other variants
    for name, val in (("stack_lds", 4), ("stack_lds", 5), ("wide", 1), ("wide", 0)):
        r.set_param(name, val)
        check(r, p, sd, tmax, want, (name, val))
        r.set_param("stack_lds", 0)
        r.set_param("wide", 2)
    for v in (1, 2):
        r.set_variant(v)
        check(r, p, sd, tmax, want, ("variant", v))
    r.set_variant(0)


def test_occluded_every_tier_of_the_ray_hand_out_exact():
    """The parameter sets of test_closest_hit_every_tier_of_the_ray_hand_out_bit_exact: each ray answered exactly once."""
    mesh = prt.scenes.refined("bunny.ply", 30_000)
    scene = prt.scenes.mesh_scene(mesh)
    r, _, _ = make_renderer(scene, 16, 16)
    rng = np.random.default_rng(5)
    o, d = util.random_rays(rng, 200_003, center=(0, 0.3, 0), radius=4.0, spread=1.5)
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=True, n_threads=8)
    t = tmax_mix(rng, want)
    for params in ({"grid_blocks": 8, "big": 3, "big_min": 1, "big_keep": 4, "chunk": 128, "static_small": 0},
                   {"grid_blocks": 64, "static_small": 4096},
                   {"grid_blocks": 8, "static_small": 8},
                   {"grid_blocks": 8, "big": 2, "big_min": 1, "big_keep": 0, "chunk": 256, "tail": 3},
                   {"grid_blocks": 24, "big": 5, "big_min": 8, "big_keep": 1, "chunk": 64, "tail": 0},
                   {"grid_blocks": 1024, "big": 2, "big_min": 96, "big_keep": 32, "chunk": 256, "tail": 1}):
        for k, v in params.items():
            r.set_param(k, v)
        for n in (200_003, 65_537):
            check(r, o[:n], d[:n], t[:n], want[:n], (params, n))


def test_occluded_small_launches_with_subtree_stealing_exact():
    scene, r = _c3()
    rng = np.random.default_rng(21)
    o, d = r.camera_rays(rng.uniform(0, 64, 20000).astype(np.float32), rng.uniform(0, 36, 20000).astype(np.float32))
    h = r.closest_hit(o, d)
    on_mesh = h["prim"] >= 2
    pos, nrm = h["position"][on_mesh][:5000], h["normal"][on_mesh][:5000]
    v = rng.normal(size=pos.shape).astype(np.float32)
    dirs = np.stack([prt.glm_normalize(x) for x in (nrm + v / np.linalg.norm(v, axis=1, keepdims=True))])
    want = util.oracle_scene(scene).closest_hit(pos, dirs, use_bvh=True, n_threads=8)
    t = tmax_mix(rng, want)
    t[::3] = np.inf  # the long walks: rays that escape the mesh walk the whole way
    for steal in (1, 8, 0):
        r.set_param("steal", steal)
        for n in (1, 63, 64, 65, 257, 1000, 5000):
            check(r, pos[:n], dirs[:n], t[:n], want[:n], (steal, n))


def test_occluded_stack_overflow_list_exact():
    """A capped stack sends rays through the overflow list to the 4-wide closest-hit walk from their seeded bound."""
    mesh = prt.scenes.refined("bunny.ply", 30_000)
    scene = prt.scenes.mesh_scene(mesh)
    r, _, _ = make_renderer(scene, 16, 16)
    rng = np.random.default_rng(8)
    o, d = _mesh_rays(rng, 12000)
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=True, n_threads=8)
    t = tmax_mix(rng, want)
    for inst in (0, 4):
        r.set_param("stack_lds", inst)
        r.set_param("stack_cap", 3)
        check(r, o, d, t, want, inst)
        r.set_param("stack_cap", 0)
    r.set_param("stack_lds", 0)


def test_occluded_one_node_per_cache_line_layout_exact():
    mesh = prt.scenes.refined("bunny.ply", 12_000)
    for scene in (prt.scenes.mesh_scene(mesh), _instanced_scene(mesh, True)):
        r = prt.HipWavefrontRenderer(device=0)
        r.set_param("node_stride", 8)
        r.Init(prt.Film(16, 16), scene, prt.Camera(width=16, height=16))
        rng = np.random.default_rng(29)
        o, d = util.random_rays(rng, 4000, center=(0, 0.5, 0), radius=9.0, spread=4.0)
        want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
        check(r, o, d, tmax_mix(rng, want), want)


@pytest.mark.parametrize("with_world_mesh", [False, True])
def test_occluded_instanced_scene_exact(with_world_mesh):
    mesh = prt.Mesh(prt.scenes.asset("icosahedron.ply")).refine(1200)
    scene = _instanced_scene(mesh, with_world_mesh)
    r, _, _ = make_renderer(scene, 16, 16)
    rng = np.random.default_rng(22)
    o, d = util.random_rays(rng, 6000, center=(0, 0.5, 0), radius=11.0, spread=4.5)
    o2 = rng.uniform(-4, 4, size=(3000, 3)).astype(np.float32)
    d2 = np.stack([prt.glm_normalize(v) for v in rng.normal(size=o2.shape).astype(np.float32)])
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
    check(r, o, d, tmax_mix(rng, want), want)
    for t in boundary_rays(want):
        check(r, o, d, t, want)


def test_occluded_analytic_primitives_next_to_meshes_exact():
    mesh = prt.scenes.refined("bunny.ply", 8_000)
    scene = prt.Scene("RANDOM_BALLS_LARGE")
    scene.AddMesh(mesh, scene.AddLambertian((0.7, 0.6, 0.5)))
    r, _, _ = make_renderer(scene, 16, 16)
    rng = np.random.default_rng(23)
    o1, d1 = util.random_rays(rng, 4000, center=(0, 1, 0), radius=14.0, spread=6.0)
    o2, d2 = _mesh_rays(rng, 4000)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
    check(r, o, d, tmax_mix(rng, want), want)


def test_occluded_host_form_reports_a_two_level_stack_overflow_and_recovers():
    mesh = prt.scenes.refined("bunny.ply", 12_000)
    scene = _instanced_scene(mesh, with_world_mesh=True)
    r, _, _ = make_renderer(scene, 16, 16)
    rng = np.random.default_rng(24)
    o, d = util.random_rays(rng, 4000, center=(0, 0.5, 0), radius=11.0, spread=4.5)
    t = np.full(len(o), np.inf, np.float32)
    r.set_param("stack_cap", 1)
    with pytest.raises(prt.PrtError, match="overflow"):
        r.occluded(o, d, t)
    r.set_param("stack_cap", 0)
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
    check(r, o, d, t, want)  # no stale flag, same scratch
    assert util.hits_equal(r.closest_hit(o, d), want) == []


def test_occluded_argument_checks():
    r = prt.HipWavefrontRenderer(device=0)
    with pytest.raises(prt.PrtError, match="prt_set_scene"):
        r.occluded(np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32), 1.0)
    r, _, _ = make_renderer(prt.Scene("CORNELL"), 8, 8)
    assert r.occluded(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 1.0).shape == (0,)
    import ctypes as C
    L = prt.capi.lib()
    fp = C.POINTER(C.c_float)
    assert L.prt_occluded(r._ctx, 0, fp(), fp(), fp(), C.POINTER(C.c_uint8)()) == 0
    assert L.prt_occluded(r._ctx, 3, fp(), fp(), fp(), C.POINTER(C.c_uint8)()) == 1
    assert L.prt_occluded_device(r._ctx, 3, None, None, None, None) == 1
    assert L.prt_closest_hit_device(r._ctx, 3, None, None, None) == 1


@pytest.mark.parametrize("own_stream", [False, True])
def test_device_forms_equal_the_host_forms(own_stream):
    import torch
    mesh = prt.scenes.refined("bunny.ply", 12_000)
    scene = prt.scenes.mesh_scene(mesh)
    r, _, _ = make_renderer(scene, 16, 16)
    s = torch.cuda.Stream(device=0)
    if own_stream:
        r.set_stream(s.cuda_stream)
    rng = np.random.default_rng(25)
    o, d = _mesh_rays(rng, 20000)
    want = r.closest_hit(o, d)
    t = tmax_mix(rng, want)
    host = r.occluded(o, d, t)
    with torch.cuda.stream(s):  # the caller's current stream is another one than the context's (or the same, own_stream)
        to, td, tt = (torch.from_numpy(x).to("cuda:0", non_blocking=True) for x in (o, d, t))
        got = r.occluded(to, td, tt)
        hits = r.closest_hit_device(to, td)
        got2 = r.occluded(to, td, 7.5)
        n_occ = int(got.sum().item())  # plain torch use of the result
    assert got.dtype == torch.bool and got.device == torch.device("cuda", 0)
    assert hits.dtype == torch.int32 and tuple(hits.shape) == (len(o), 10)
    assert np.array_equal(got.cpu().numpy(), host) and n_occ == int(host.sum())
    assert np.array_equal(got2.cpu().numpy(), r.occluded(o, d, np.float32(7.5)))
    assert util.hits_equal(prt.hits_to_numpy(hits), want) == []
    assert np.array_equal(host, contract(util.oracle_scene(scene).closest_hit(o, d, use_bvh=True, n_threads=8), t, d))
    with pytest.raises(ValueError, match="device"):
        r.occluded(to.cpu(), td.cpu(), 1.0)
    with pytest.raises(ValueError, match="dtype"):
        r.occluded(to.double(), td.double(), 1.0)
    with pytest.raises(ValueError, match="contiguous"):
        r.occluded(to.t().contiguous().t(), td, 1.0)
    with pytest.raises(ValueError, match="shape"):
        r.occluded(to, td, tt[:-1])
    if own_stream:
        r.set_stream(0)


def test_queries_between_renders_change_nothing():
    mesh = prt.scenes.refined("bunny.ply", 12_000)
    scene = prt.scenes.mesh_scene(mesh)
    W, H = 64, 36
    cam = prt.Camera(position=(1.5, 1.0, 2.5), width=W, height=H)
    a, fa, _ = make_renderer(scene, W, H, max_depth=5, seed=3, cam=cam)
    b, fb, _ = make_renderer(scene, W, H, max_depth=5, seed=3, cam=cam)
    rng = np.random.default_rng(26)
    o, d = _mesh_rays(rng, 30000)
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=True, n_threads=8)
    t = tmax_mix(rng, want)
    a.ProgressiveRender(2)
    check(a, o, d, t, want)
    a.ProgressiveRender(2)
    b.ProgressiveRender(2)
    b.ProgressiveRender(2)
    a.download()
    b.download()
    assert np.array_equal(fa.accum, fb.accum) and np.array_equal(fa.weights, fb.weights)
    check(a, o[:5000], d[:5000], t[:5000], want[:5000])
    assert util.hits_equal(a.closest_hit(o, d), want) == []  # the two share scratch and the ray buffer
