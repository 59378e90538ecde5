"""Refit from device arrays (prt_refit_meshes_device, include/prt.h) on one MI355X: a tree refitted from torch tensors on
the device is the tree prt_refit_meshes makes of the same arrays on the host, to the bit: tree, records, scene state,
closest hits, film and ray count; both equal the oracle on the deformed scene and a fresh Init of it.  Normals the caller
leaves out are computed on the device by compute_normals' rule, bit for bit (tests/refit_device_replay.py).  Refused
calls leave the scene as it was; inputs are read in stream order; what crosses the bus is counted and bounded.

Shapes: the bunny (10 k triangles) for the three builders, the icosahedron refined to 2 k elsewhere; films 32 x 18, 2 spp,
depth 5; 2 000 rays.  The oracle's answers are computed once per scene and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_trees as dt
import refit_device_replay as rr
import util
from util import prt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
capi = prt.capi

W, H, SPP, DEPTH, SEED = 32, 18, 2, 5, 3
CAM = dict(position=(2.0, 1.5, 3.0), width=W, height=H)
INFO_FIELDS = [f for f, _ in capi.PrtBvhInfo._fields_ if f not in ("build_ms", "refit_ms")]


def _deformed(mesh, amp, seed, normals=True):
    """test_gpu_parity._deformed: the same topology with every vertex moved, a smooth bend plus per-vertex noise of `amp`."""
    v = mesh.GetVertices().astype(np.float64)
    rng = np.random.default_rng(seed)
    v[:, 0] += amp * 4.0 * np.sin(3.0 * v[:, 1])
    v[:, 2] += amp * 4.0 * np.cos(2.0 * v[:, 0])
    v += rng.normal(size=v.shape) * amp
    return prt.Mesh(vertices=v.astype(np.float32), normals=mesh.GetNormals() if normals else None, indices=mesh.GetIndices())


def _mesh_rays(rng, n, extent=1.0):
    o1, d1 = util.random_rays(rng, n // 2, center=(0, 0, 0), radius=9.0, spread=extent)
    o2 = rng.uniform(-extent, extent, size=(n - n // 2, 3)).astype(np.float32)
    d2 = np.stack([prt.glm_normalize(v) for v in rng.normal(size=o2.shape).astype(np.float32)])
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def _renderer(scene, builder=0, prepare=None):
    r = prt.HipWavefrontRenderer(device=0, max_depth=DEPTH, seed=SEED)
    r.set_param("gpu_build", builder)
    film = prt.Film(W, H)
    r.Init(film, scene, prt.Camera(**CAM))
    if prepare:
        prepare(r)
    return r, film


def _render(r, film):
    film.Clear()
    r.frame_index = 0
    r.reset_stats()
    r.ProgressiveRender(SPP)
    r.download()
    return film.accum.copy(), film.weights.copy(), r.stats().rays_total


def _same_render(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _same_tree(a, b, refits=True):
    """bvh_read8, bvh_read and bvh_info (but its times; refits=False: the two have been refitted a different number of times)"""
    ia, ib = a.bvh_info(), b.bvh_info()
    fields = [f for f in INFO_FIELDS if refits or f != "refits"]
    assert [getattr(ia, f) for f in fields] == [getattr(ib, f) for f in fields]
    assert np.array_equal(a.bvh_read8(), b.bvh_read8())
    for x, y in zip(a.bvh_read(), b.bvh_read()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def _same_hits(a, b):
    assert util.hits_equal(a, b) == []
    hit = a["prim"] >= 0
    assert np.array_equal(a["normal"][hit].view(np.uint32), b["normal"][hit].view(np.uint32))
    assert np.array_equal(a["position"][hit].view(np.uint32), b["position"][hit].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _case(ply, target, normals=True):
    """Base and deformed scene of a mesh with the oracle's closest hits (linear scan) and film for the deformed one."""
    base = prt.scenes.refined(ply, target)
    moved = _deformed(base, 0.01, 5, normals)
    scene2 = prt.scenes.mesh_scene(moved)
    osc = util.oracle_scene(scene2)
    o, d = _mesh_rays(np.random.default_rng(7), 2000)
    want = osc.closest_hit(o, d, use_bvh=False, n_threads=8)
    acc, wts, rays = osc.render(prt.Camera(**CAM).desc(), W, H, spp=SPP, max_depth=DEPTH, seed=SEED, iterative=True, use_bvh=True, n_threads=8)
    return dict(base=base, moved=moved, scene1=prt.scenes.mesh_scene(base), scene2=scene2, o=o, d=d, hits=want, film=(acc, wts, rays))


def _ico():
    return _case("icosahedron.ply", 2000)


def _refit_both(c, builder=0, normals=True, producer=None):
    """Context A refitted from host arrays, context B from tensors; both have rendered the old geometry first.  A refit
    keeps the topology it finds, and the device builders (gpu_build 1, 2) hand out node and slot numbers through atomic
    counters: two builds of one mesh are the same tree in two numberings (measured on the bunny: 1128 of 1266 and 2104 of
    2180 node rows differ between two contexts BEFORE any refit).  So for those B takes A's tree by prt_clone_scene: what is
    compared is the two refits, not two runs of the builder."""
    a, fa = _renderer(c["scene1"], builder)
    b, fb = _renderer(c["scene1"], builder)
    if builder:
        b._check(capi.lib().prt_clone_scene(b._ctx, a._ctx))
        b.SetCamera(prt.Camera(**CAM))
    for r in (a, b):
        r.ProgressiveRender(1)
    a.Refit(c["scene2"])
    if producer:
        producer(b)
    else:
        b.RefitDevice(_t(c["moved"].GetVertices()), _t(c["moved"].GetNormals()) if normals else None)
    return a, fa, b, fb


def _check_equal_to_host_form_and_oracle(c, a, fa, b, fb):
    _same_tree(a, b)
    ha, hb = a.closest_hit(c["o"], c["d"]), b.closest_hit(c["o"], c["d"])
    _same_hits(ha, hb)
    assert util.hits_equal(hb, c["hits"]) == [] and (hb["prim"] >= 2).sum() > 50
    ra, rb = _render(a, fa), _render(b, fb)
    assert _same_render(ra, rb) and _same_render(rb, c["film"])
    f, ff = _renderer(c["scene2"])
    assert _same_render(_render(f, ff), rb)


# ---- 1. equals the host form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1, 2])
def test_device_form_equals_the_host_form_the_oracle_and_a_fresh_init(builder):
    c = _case("bunny.ply", 0)
    a, fa, b, fb = _refit_both(c, builder)
    ia, ib = a.refit_info(), b.refit_info()
    assert (ia["last_form"], ib["last_form"], ia["refits"], ib["refits"]) == (1, 2, 1, 1)
    assert ib["normals_computed"] == 0 and ib["host_copies_stale"] == 1 and ia["host_copies_stale"] == 0
    _check_equal_to_host_form_and_oracle(c, a, fa, b, fb)
    assert b.refit_info()["host_copies_stale"] == 0 and b.bvh_info().n_nodes4 == 0 and b.bvh_info().n_nodes == 0


# ---- 2. normals computed on the device ---------------------------------------------------------------------------------
def test_without_normals_the_device_computes_the_library_rule_bit_for_bit():
    c = _case("bunny.ply", 0, False)   # (prt.Mesh(vertices, indices): the host form gets compute_normals' normals)
    a, fa, b, fb = _refit_both(c, 0, normals=False)
    assert b.refit_info()["normals_computed"] == 1
    _check_equal_to_host_form_and_oracle(c, a, fa, b, fb)
    v, i = c["moved"].GetVertices(), c["moved"].GetIndices()
    got = b.mesh_normals_device(0, _t(v)).cpu().numpy()
    want = rr.vertex_normals(v, i)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.nonzero((got != want).any(axis=1))[0][:10]
    assert np.array_equal(want.view(np.uint32), c["moved"].GetNormals().view(np.uint32))


def test_normals_of_a_degenerate_mesh():
    v, i = rr.degenerate_mesh()
    r, _ = _renderer(prt.scenes.mesh_scene(prt.Mesh(vertices=v, indices=i)))
    for pos in (v, (v * np.float32(3.7) + np.float32(0.25)).astype(np.float32)):
        got = r.mesh_normals_device(0, _t(pos)).cpu().numpy()
        want = rr.vertex_normals(pos, i)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
        assert got[11].tolist() == [0.0, 1.0, 0.0] and got[8].tolist() == [0.0, 1.0, 0.0]
    with pytest.raises(ValueError):
        r.mesh_normals_device(1, _t(v))
    with pytest.raises(ValueError):
        r.mesh_normals_device(0, _t(v[:5]))


# ---- 3. two world meshes behind analytic primitives --------------------------------------------------------------------
def _two_mesh_scene(m0, m1):
    sc = prt.Scene(preset=None)
    ground, light = sc.AddLambertian((0.5, 0.5, 0.5)), sc.AddEmissive((15.0, 15.0, 15.0))
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    sc.AddCircle(0.7, sc.AddMetal((0.9, 0.8, 0.7), 0.1), euler_deg=(90.0, 0.0, 0.0), translation=(0.0, 0.5, -2.0))
    sc.AddMesh(m0, sc.AddLambertian((0.8, 0.3, 0.3)))
    sc.AddMesh(m1, sc.AddMetal((0.7, 0.7, 0.9), 0.2))
    return sc


def test_two_world_meshes_one_with_normals_one_without():
    base0 = prt.scenes.refined("icosahedron.ply", 2000)
    small = prt.scenes.refined("icosahedron.ply", 300)
    base1 = prt.Mesh(vertices=small.GetVertices() * np.float32(0.5) + np.array([1.4, 0.2, 0.3], np.float32), normals=small.GetNormals(),
                     indices=small.GetIndices())
    m0, m1 = _deformed(base0, 0.01, 5), _deformed(base1, 0.01, 6, normals=False)
    scene1, scene2 = _two_mesh_scene(base0, base1), _two_mesh_scene(m0, m1)
    assert len(scene1.primitives) == 3
    a, fa = _renderer(scene1)
    b, fb = _renderer(scene1)
    a.Refit(scene2)
    b.RefitDevice([_t(m0.GetVertices()), _t(m1.GetVertices())], [_t(m0.GetNormals()), None])
    assert b.refit_info()["normals_computed"] == 1
    _same_tree(a, b)
    o, d = _mesh_rays(np.random.default_rng(11), 2000, extent=1.5)
    hb = b.closest_hit(o, d)
    _same_hits(a.closest_hit(o, d), hb)
    osc = util.oracle_scene(scene2)
    assert util.hits_equal(hb, osc.closest_hit(o, d, use_bvh=False, n_threads=8)) == []
    assert (hb["prim"] >= 3 + m0.n_triangles).sum() > 20 and ((hb["prim"] >= 3) & (hb["prim"] < 3 + m0.n_triangles)).sum() > 100
    rb = _render(b, fb)
    assert _same_render(_render(a, fa), rb)
    assert _same_render(rb, osc.render(prt.Camera(**CAM).desc(), W, H, spp=SPP, max_depth=DEPTH, seed=SEED, iterative=True, use_bvh=True, n_threads=8))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_scene_as_it_was():
    c = _ico()
    r, film = _renderer(c["scene1"])
    before = _render(r, film)
    v, n = c["moved"].GetVertices(), c["moved"].GetNormals()
    bad = v.copy()
    bad[17, 1] = np.nan
    with pytest.raises(prt.PrtError, match="non-finite"):
        r.RefitDevice(_t(bad), _t(n))
    assert r.bvh_info().refits == 0 and r.refit_info()["host_copies_stale"] == 0 and _same_render(_render(r, film), before)
    bad = v.copy()
    bad[3, 0] = np.inf
    with pytest.raises(prt.PrtError, match="non-finite"):
        r.RefitDevice(_t(bad))
    badn = n.copy()
    badn[9, 2] = np.nan
    with pytest.raises(prt.PrtError, match="non-finite"):
        r.RefitDevice(_t(v), _t(badn))
    assert r.bvh_info().refits == 0 and _same_render(_render(r, film), before)
    for args in (([_t(v), _t(v)],), (torch.from_numpy(v),), (_t(v).double(),), (_t(v)[:-1],), (_t(v), [None, None]), (_t(v).t(),), (v,)):
        with pytest.raises(ValueError):
            r.RefitDevice(*args)
    assert r.bvh_info().refits == 0 and _same_render(_render(r, film), before)
    assert util.hits_equal(r.closest_hit(c["o"], c["d"]), util.oracle_scene(c["scene1"]).closest_hit(c["o"], c["d"], use_bvh=False, n_threads=8)) == []


def test_placed_copies_and_deep_trees_are_refused():
    c = _ico()
    sc = prt.scenes.mesh_scene(c["base"])
    sc.AddInstance(prt.scenes.refined("icosahedron.ply", 80), 2, scale=0.5, translation=(1.5, 0.0, 0.0))
    r, film = _renderer(sc)
    before = _render(r, film)
    with pytest.raises(prt.PrtError, match="placed copies"):
        r.RefitDevice(_t(c["moved"].GetVertices()))
    assert _same_render(_render(r, film), before)
    deep = dt.case_scene("d17")
    r, film = _renderer(deep)
    before = _render(r, film)
    mesh = deep.meshes[0][0]
    with pytest.raises(prt.PrtError, match=r"17 levels.*depth8 > 16"):
        r.RefitDevice(_t(mesh.GetVertices()), _t(mesh.GetNormals()))
    info = r.bvh_info()
    assert info.refits == 0 and info.n_nodes4 > 0 and _same_render(_render(r, film), before)


# ---- 5. stream order ---------------------------------------------------------------------------------------------------
def test_positions_produced_on_the_context_stream_need_no_synchronisation():
    c = _ico()
    src_v, src_n = _t(c["moved"].GetVertices()), _t(c["moved"].GetNormals())
    torch.cuda.synchronize()

    def producer(b):
        h = C.c_void_p()
        b._check(capi.lib().prt_get_stream(b._ctx, C.byref(h)))
        ext = torch.cuda.ExternalStream(h.value, device=torch.device("cuda", 0))
        with torch.cuda.stream(ext):   # torch's current stream IS the context's: RefitDevice inserts no event and no wait
            tmp = src_v
            for _ in range(64):        # a chain of permutations the refit has to wait for: the arrays come out as they went in
                tmp = tmp.roll(1, 0)
            pos = tmp.roll(-64, 0).contiguous()
            b.RefitDevice(pos, src_n)
        assert torch.equal(pos, src_v)

    a, fa, b, fb = _refit_both(c, 0, producer=producer)
    _check_equal_to_host_form_and_oracle(c, a, fa, b, fb)


# ---- 6. traffic --------------------------------------------------------------------------------------------------------
def test_traffic_host_copies_and_clone():
    c = _ico()
    nt = c["moved"].n_triangles
    a, fa, b, fb = _refit_both(c)
    first = b.refit_info()
    assert first["h2d_bytes"] >= 24 * nt and first["d2h_bytes"] <= 256   # (the tables go up once)
    b.RefitDevice(_t(c["base"].GetVertices()), _t(c["base"].GetNormals()))
    b.RefitDevice(_t(c["moved"].GetVertices()), _t(c["moved"].GetNormals()))
    info = b.refit_info()
    print(f"device form: {info}\nhost form:   {a.refit_info()}")
    assert info["h2d_bytes"] == 0 and info["d2h_bytes"] <= 256 and info["refits"] == 3 and info["host_copies_stale"] == 1
    ia = a.refit_info()
    assert ia["h2d_bytes"] >= 72 * nt and ia["d2h_bytes"] >= 96 * nt and ia["host_copies_stale"] == 0
    # a clone takes the refitted scene although the host copies were behind
    twin = prt.HipWavefrontRenderer(device=0, max_depth=DEPTH, seed=SEED)
    L = capi.lib()
    twin._check(L.prt_clone_scene(twin._ctx, b._ctx))
    assert b.refit_info()["host_copies_stale"] == 0
    ft = prt.Film(W, H)
    twin._check(L.prt_set_film(twin._ctx, W, H, 0, 1))
    twin.film, ft._renderer = ft, twin
    twin.SetCamera(prt.Camera(**CAM))
    assert _same_render(_render(twin, ft), c["film"]) and _same_render(_render(b, fb), c["film"])
    # the read-backs bring the host copies up to date on their own, too
    b.RefitDevice(_t(c["base"].GetVertices()), _t(c["base"].GetNormals()))
    assert b.refit_info()["host_copies_stale"] == 1
    n8 = b.bvh_read8()
    assert b.refit_info()["host_copies_stale"] == 0
    a.Refit(c["scene1"])
    assert np.array_equal(n8, a.bvh_read8())
    # and the host form after the device form starts from them
    b.RefitDevice(_t(c["moved"].GetVertices()), _t(c["moved"].GetNormals()))
    b.Refit(c["scene2"])
    a.Refit(c["scene2"])
    _same_tree(a, b, refits=False)


# ---- 7. triangle lights ------------------------------------------------------------------------------------------------
def _lit_scene(mesh):
    sc = prt.Scene(preset=None)
    sc.AddQuad(20.0, 20.0, sc.AddLambertian((0.5, 0.5, 0.5)), translation=(0.0, -1.0, 0.0))
    sc.AddQuad(2.0, 2.0, sc.AddEmissive((5.0, 5.0, 5.0)), euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    sc.AddMesh(mesh, sc.AddEmissive((4.0, 3.0, 2.0)))
    return sc


@pytest.mark.parametrize("selection", ["power", "clustered"])
def test_emissive_mesh_lights_follow_like_the_host_form(selection):
    base = prt.scenes.refined("icosahedron.ply", 300)
    moved = _deformed(base, 0.02, 5)
    scene1, scene2 = _lit_scene(base), _lit_scene(moved)

    def prepare(r):
        r.set_light_sources("all")
        r.set_light_selection(selection, 8)
        r.set_lighting("mis")

    a, fa = _renderer(scene1, prepare=prepare)
    b, fb = _renderer(scene1, prepare=prepare)
    a.Refit(scene2)
    b.RefitDevice(_t(moved.GetVertices()), _t(moved.GetNormals()))
    info = b.refit_info()
    assert info["d2h_bytes"] <= 256 + 36 * moved.n_triangles and info["d2h_bytes"] >= 36 * moved.n_triangles
    for x, y in zip(a.light_info(), b.light_info()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.light_intervals(), b.light_intervals())
    ca, cb = a.light_clusters(), b.light_clusters()
    assert sorted(ca) == sorted(cb) and all(np.array_equal(np.asarray(ca[k]), np.asarray(cb[k])) for k in ca)
    rb = _render(b, fb)
    assert _same_render(_render(a, fa), rb)
    f, ff = _renderer(scene2, prepare=prepare)
    assert _same_render(_render(f, ff), rb)


# ---- 8. sequences ------------------------------------------------------------------------------------------------------
def test_three_deformations_alternating_the_forms_equal_fresh_inits():
    c = _ico()
    r, film = _renderer(c["scene1"])
    r.ProgressiveRender(1)
    for step, (amp, seed) in enumerate([(0.01, 5), (0.03, 6), (0.005, 7)]):
        m = _deformed(c["base"], amp, seed)
        sc = prt.scenes.mesh_scene(m)
        if step % 2 == 0:
            r.RefitDevice(_t(m.GetVertices()), _t(m.GetNormals()))
        else:
            r.Refit(sc)
        assert r.bvh_info().refits == step + 1 and r.refit_info()["last_form"] == (2 if step % 2 == 0 else 1)
        r.ProgressiveRender(1)
        assert r.primary_reuse()[0] == 0     # (the batch after the call rebuilt its primary stage)
        got = _render(r, film)
        f, ff = _renderer(sc)
        assert _same_render(_render(f, ff), got), step
        fill, levels = util.check_bvh8(r.bvh_read8(), r.bvh_read()[1])
        assert levels == r.bvh_info().depth8


def test_textures_stay_and_the_temporal_history_goes():
    base = prt.scenes.refined("icosahedron.ply", 2000)
    base.SetUVs(prt.scenes.planar_uvs(base))
    moved = _deformed(base, 0.01, 5)
    moved.SetUVs(base.GetUVs())

    def textured(mesh):
        sc = prt.scenes.mesh_scene(mesh)
        sc.SetMaterialTexture(2, sc.AddTexture(prt.scenes.checker(8), filter="bilinear"))
        return sc

    scene1, scene2 = textured(base), textured(moved)
    r, film = _renderer(scene1, prepare=lambda r: r.set_film_statistics(True))
    plain, _ = _renderer(prt.scenes.mesh_scene(moved), prepare=lambda r: r.set_film_statistics(True))
    r.ProgressiveRender(SPP)
    r.temporal_step()
    t0 = r.temporal_info()
    assert t0.steps == 1
    tex0 = r.texture_info()
    r.RefitDevice(_t(moved.GetVertices()), _t(moved.GetNormals()))
    t1 = r.temporal_info()
    assert t1.steps == 0 and t1.resets == t0.resets + 1
    tex1 = r.texture_info()
    assert [getattr(tex1, f) for f, _ in tex1._fields_] == [getattr(tex0, f) for f, _ in tex0._fields_] and tex1.n_textures == 1
    got = _render(r, film)
    f, ff = _renderer(scene2, prepare=lambda r: r.set_film_statistics(True))
    assert _same_render(_render(f, ff), got)
    assert not np.array_equal(got[0], _render(plain, plain.film)[0])   # (the checker is in the picture)


def test_group_renderer_refits_from_tensors_rank_by_rank():
    """The group has no C entry point for device arrays; its Python renderer calls the single form on every rank's context."""
    c = _ico()
    g = prt.HipWavefrontGroupRenderer([0], max_depth=DEPTH, seed=SEED)
    film = prt.Film(W, H)
    g.Init(film, c["scene1"], prt.Camera(**CAM))
    g.ProgressiveRender(1)
    g.RefitDevice(_t(c["moved"].GetVertices()), _t(c["moved"].GetNormals()))
    info = g.refit_info()
    assert info["last_form"] == 2 and info["refits"] == 1
    with pytest.raises(ValueError):
        g.RefitDevice([_t(c["moved"].GetVertices())] * 2)
    g.Clear()
    rays0 = g.stats().rays_total   # (the group has no reset of the counters: the batch before the refit is in them)
    g.ProgressiveRender(SPP)
    g.download()
    assert np.array_equal(film.accum.view(np.uint32), c["film"][0].view(np.uint32)) and np.array_equal(film.weights, c["film"][1])
    assert g.stats().rays_total - rays0 == c["film"][2]
