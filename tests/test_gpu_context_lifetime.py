"""What a context owns on the device, counted (prt_device_memory_info; csrc/prt_devmem.h) on one MI355X, one process, small shapes.

The scene: the icosahedron as one placed copy (a mirror, so the guide features follow chains), one emissive mesh (two
triangles), two analytic quads (ground and lamp), one checker texture on the ground and the copy, a 4 x 2 environment image,
mesh lights with clustered selection, light-sampled paths; a 16 x 12 film.  `flat`: the same scene with the icosahedron as a
world-space mesh, because the interface refits only scenes without placed copies.

1. Full lifecycle, three create - destroy cycles: set scene / camera / film, film statistics, a 2-sample lit render, one adaptive
   pass, render_features (max_specular 2, 2 feature samples), two temporal steps, closest_hit / occluded / radiance (lit) on 65
   rays, an 8 x 8 bake with the texel light, set_instance_transforms in both modes, [set_scene to the flat scene, which the two
   refits need,] refit_meshes and refit_meshes_device, measure_shade_divergence, a smaller and a larger film, a second set_scene.
   live_bytes is above the baseline while the context lives and exactly the baseline after prt_destroy, every cycle.
2. Five calls the interface refuses, on either scene: live_bytes after each equals its value before, and the context still
   renders the frame of check 3 bit for bit.
3. Steady state: after one 2-sample render, alloc_calls stands still across two more identical renders, and across two more
   identical closest_hit calls of 65 rays.
4. The film of cycle 1's render equals the film of cycle 3's bit for bit."""
import ctypes as C
import gc

import numpy as np
import pytest

import parallelraytracing_amd as prt
from parallelraytracing_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
W, H, DEPTH, SEED, SPP, RAYS = 16, 12, 4, 11, 2, 65
CAM = dict(position=(2.0, 1.5, 3.0), width=W, height=H)


def _ico(target=0):
    m = prt.Mesh(prt.scenes.asset("icosahedron.ply"))
    if target:
        m.refine(target)
    return m.SetUVs(prt.scenes.planar_uvs(m))


def _square(y=2.5, dx=0.0):
    v = np.array([[-0.5 + dx, y, -0.5], [0.5 + dx, y, -0.5], [0.5 + dx, y, 0.5], [-0.5 + dx, y, 0.5]], F)
    n = np.tile(np.array([[0.0, -1.0, 0.0]], F), (4, 1))
    return prt.Mesh(vertices=v, normals=n, indices=np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
                    uvs=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F))


def _scene(flat=False, dx=0.0, ico=None, copies=1):
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.5, 0.5, 0.5))
    lamp = sc.AddEmissive((15.0, 15.0, 15.0))
    body = sc.AddMetal((0.9, 0.9, 0.9), 0.0)
    glow = sc.AddEmissive((40.0, 30.0, 20.0))
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, lamp, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    sc.AddMesh(_square(dx=dx), glow)
    ico = ico if ico is not None else _ico()
    if flat:
        sc.AddMesh(ico, body)
    for k in range(0 if flat else copies):
        sc.AddInstance(ico, body, scale=0.8, translation=(dx + 1.5 * k, 0.0, 0.0))
    t = sc.AddTexture(prt.scenes.checker(4), "bilinear", "repeat")
    sc.SetMaterialTexture(ground, t)
    sc.SetMaterialTexture(body, t)
    return sc


def _rays():
    rng = np.random.default_rng(65)
    o = rng.normal(size=(RAYS, 3))
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * 6.0).astype(F)
    o[:, 1] = np.abs(o[:, 1]) + F(0.2)
    d = np.stack([prt.glm_normalize(v) for v in (rng.uniform(-1.0, 1.0, size=(RAYS, 3)).astype(F) - o)])
    return np.ascontiguousarray(o), np.ascontiguousarray(d.astype(F))


def _create(scene):
    r = prt.HipWavefrontRenderer(device=0, max_depth=DEPTH, seed=SEED)
    r.set_environment(np.random.default_rng(3).uniform(0.1, 1.0, size=(2, 4, 3)).astype(F))
    r.set_lighting("mis")
    r.set_light_sources("all")
    r.set_light_selection("clustered", 4)
    film = prt.Film(W, H)
    r.Init(film, scene, prt.Camera(**CAM))
    r.set_film_statistics(True)
    return r, film


def _frame(r, film):
    film.Clear()
    r.frame_index = 0
    r.ProgressiveRender(SPP)
    r.download()
    return film.accum.view(np.uint32).copy(), film.weights.copy()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _destroy(r):
    capi.lib().prt_destroy(r._ctx)
    r._ctx = None


def _baseline():
    """live_bytes before a check begins.  Contexts that earlier tests of the process left in reference cycles (a refused call's
    traceback holds its frame, and the frame its renderer) are destroyed by whichever collection comes next; collected here,
    so that none of them is destroyed between two readings of a check and counted as this context's bytes."""
    gc.collect()
    return prt.device_memory_info()[0]


def _lifecycle():
    """One context through the whole interface; returns the frame of its first render.  Asserts check 1 for this cycle."""
    import torch
    base = _baseline()
    scene = _scene()
    r, film = _create(scene)
    frame = _frame(r, film)
    assert frame[1].min() == SPP
    r.render_adaptive(threshold=0.05, min_spp=2, step_spp=2, max_spp=4)
    r.set_feature_trace(max_specular=2)
    r.set_feature_sampling(samples=2)
    feats = r.render_features()
    assert "guide" in feats and "sampled" in feats
    r.temporal_step()
    r.temporal_step()
    o, d = _rays()
    hits = r.closest_hit(o, d)
    assert (hits["prim"] >= 0).any()
    r.occluded(o, d, np.full(RAYS, 4.0, F))
    r.radiance(o, d, samples=2, lighting=True)
    irr, info = r.bake_irradiance(instance=0, size=(8, 8), samples=2, lighting=True, texel_light=True, return_info=True)
    assert (info["coverage"] == 1).any()
    for k, mode in enumerate(("refit", "rebuild")):
        scene.SetInstanceTransform(0, scale=0.8, translation=(0.2 + 0.3 * k, 0.1, -0.2))
        r.UpdateInstances(scene, mode)
    assert r.instance_update_info().updates == 2
    # (the refits: the interface rebuilds scenes with placed copies, so the same scene with the copy as a world-space mesh)
    r.Init(film, _scene(flat=True), prt.Camera(**CAM))
    moved = _scene(flat=True, dx=0.25)
    r.Refit(moved)
    r.RefitDevice([torch.from_numpy(m.GetVertices().copy()).to("cuda:0") for m, _ in moved.meshes])
    assert r.refit_info()["refits"] == 2
    r.measure_shade_divergence()
    r.set_film(prt.Film(8, 8))
    r.ProgressiveRender(1)
    r.set_film(prt.Film(40, 24))
    r.ProgressiveRender(1)
    r.Init(film, scene, prt.Camera(**CAM))
    r.ProgressiveRender(1)
    assert prt.device_memory_info()[0] > base
    _destroy(r)
    assert prt.device_memory_info()[0] == base
    return frame


def test_three_lifecycles_return_every_byte_and_render_the_same_frame():
    frames = [_lifecycle() for _ in range(3)]
    assert _same(frames[0], frames[2])


def _refusals(r, scene, flat):
    o, d = _rays()

    def wrong_instance_count():
        r.UpdateInstances(_scene(copies=2), "refit")

    def wrong_triangle_count():  # (with the placed copy the interface refuses before it counts: such scenes are rebuilt)
        r.Refit(_scene(flat=flat, ico=_ico(80)))

    def bake_reserved():
        uv = np.ascontiguousarray(prt.scenes.planar_uvs(_ico()))
        t = capi.PrtBakeTarget(capi.BAKE_MESH if flat else capi.BAKE_INSTANCE, 1 if flat else 0, uv.ctypes.data_as(C.POINTER(C.c_float)), 8, 8)
        q = capi.PrtRadianceQuery(DEPTH, 2, SEED, 0)
        opt = capi.PrtBakeOptions(1, 1, 0, 1)
        total, cov = np.zeros((8, 8, 3), F), np.zeros((8, 8), np.uint8)
        r._check(capi.lib().prt_bake_irradiance_opt(r._ctx, C.byref(t), C.byref(q), C.byref(opt), total.ctypes.data_as(C.POINTER(C.c_float)),
                                                    cov.ctypes.data_as(C.POINTER(C.c_uint8)), None))

    def radiance_no_samples():
        r.radiance(o, d, samples=0)

    def texture_material_out_of_range():
        bad = _scene(flat=flat)
        bad.materials.append(bad.materials[0])  # (one material more than the scene has: the binding names material 4)
        bad.SetMaterialTexture(len(bad.materials) - 1, 0)
        r.set_textures(bad)

    return [wrong_instance_count, wrong_triangle_count, bake_reserved, radiance_no_samples, texture_material_out_of_range]


@pytest.mark.parametrize("flat", [False, True], ids=["placed_copy", "world_mesh"])
def test_refused_calls_allocate_nothing_and_steady_state_allocates_nothing(flat):
    base = _baseline()
    scene = _scene(flat=flat)
    r, film = _create(scene)
    frame = _frame(r, film)
    # check 3: the steady state
    calls = prt.device_memory_info()[1]
    for _ in range(2):
        r.frame_index = 0
        r.ProgressiveRender(SPP)
    assert prt.device_memory_info()[1] == calls
    o, d = _rays()
    first = r.closest_hit(o, d)
    calls = prt.device_memory_info()[1]
    for _ in range(2):
        assert np.array_equal(r.closest_hit(o, d), first)
    assert prt.device_memory_info()[1] == calls
    # check 2: the refusals
    for call in _refusals(r, scene, flat):
        live = prt.device_memory_info()[0]
        with pytest.raises(prt.PrtError):
            call()
        assert prt.device_memory_info()[0] == live, call.__name__
        assert _same(_frame(r, film), frame), call.__name__
    _destroy(r)
    assert prt.device_memory_info()[0] == base
