"""CPU-side tests of the temporal reprojection's interface (include/prt.h "Temporal reprojection"): every refusal of
prt_temporal_reproject / _device / prt_film_temporal / prt_temporal_prev_surface on a host-only context (they are checked
before the device is asked for), the ctypes structs and the defaults, which calls drop the history and which keep it
(PrtTemporalInfo.resets counts the drops, whether a history existed or not), and prt_get_camera_basis against the oracle's."""
import ctypes as C

import numpy as np
import pytest

import temporal_replay as tr
from util import orc, prt

capi = prt.capi
NAN = float("nan")
INVALID, NO_DEVICE = 1, 2  # PRT_ERR_INVALID, PRT_ERR_NO_DEVICE
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
CUR = ("c", "n", "A", "Q", "prim", "Pprev", "Nprev")
OUTS = ("c_out", "n_out", "m1_out", "m2_out")


def test_structs_defaults_and_symbols():
    assert C.sizeof(capi.PrtTemporal) == 12 and C.sizeof(capi.PrtCameraBasis) == 60 and capi.PrtCameraBasis.tan_fov_y.offset == 56
    assert C.sizeof(capi.PrtTemporalInfo) == 24 and capi.PrtTemporalInfo.device_bytes.offset == 16
    k = capi.PrtTemporal()
    capi.lib().prt_temporal_defaults(C.byref(k))
    assert k.max_history == 32.0 and k.normal_min == np.float32(0.9) and k.plane_tol == np.float32(0.01)
    assert tr.DEFAULTS == dict(max_history=32.0, normal_min=0.9, plane_tol=0.01)
    capi.lib().prt_temporal_defaults(None)
    assert capi.TEMPORAL_MAX_PIXELS == 1 << 28
    for name in ("prt_temporal_defaults", "prt_get_camera_basis", "prt_temporal_reproject", "prt_temporal_reproject_device",
                 "prt_temporal_prev_surface", "prt_film_temporal", "prt_temporal_reset", "prt_temporal_info"):
        assert name in capi.SIGNATURES and getattr(capi.lib(), name)
    for name in ("temporal_step", "temporal_reset", "temporal_info", "temporal_arrays", "camera_basis", "temporal_prev_surface"):
        assert callable(getattr(prt.HipWavefrontRenderer, name))
    assert callable(prt.HipWavefrontGroupRenderer.temporal_step)


def _arrays(W=4, H=3):
    z3, z1, zi = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.int32)
    a = {k: (zi.copy() if k in ("prim", "hprim") else z3.copy() if k in ("c", "Pprev", "Nprev", "hc", "hP", "hN", "c_out") else z1.copy())
         for k in CUR + tr.HIST_KEYS + OUTS}
    return a


def _call(r, cfg=None, W=4, H=3, null=None, device=False, basis_size=None, null_basis=False, **fields):
    k = capi.PrtTemporal()
    capi.lib().prt_temporal_defaults(C.byref(k))
    for name, v in fields.items():
        setattr(k, name, v)
    a = _arrays()
    K = capi.PrtCameraBasis()
    (K.W, K.H), K.tan_fov_y = basis_size or (float(W), float(H)), 0.5
    K.front[2] = -1.0
    pK = None if null_basis else C.byref(K)
    if device:
        ptr = [None if n == null else C.c_void_p(a[n].ctypes.data) for n in CUR + tr.HIST_KEYS + OUTS]   # never dereferenced: there is no device
        return capi.lib().prt_temporal_reproject_device(r._ctx, C.byref(k) if cfg is None else cfg, W, H, pK, *ptr, None, None)
    ptr = [None if n == null else a[n].ctypes.data_as(_ip if n in ("prim", "hprim") else _fp) for n in CUR + tr.HIST_KEYS + OUTS]
    return capi.lib().prt_temporal_reproject(r._ctx, C.byref(k) if cfg is None else cfg, W, H, pK, *ptr, None, None)


REFUSALS = [
    ("max_history 0.5", dict(max_history=0.5)), ("max_history 0", dict(max_history=0.0)), ("max_history nan", dict(max_history=NAN)),
    ("normal_min above 1", dict(normal_min=1.5)), ("normal_min below -1", dict(normal_min=-1.0001)), ("normal_min nan", dict(normal_min=NAN)),
    ("plane_tol negative", dict(plane_tol=-0.01)), ("plane_tol nan", dict(plane_tol=NAN)),
    ("W = 0", dict(W=0)), ("H = 0", dict(H=0)), ("above 2^28 pixels", dict(W=1 << 15, H=(1 << 13) + 1)),
    ("the product wraps 32 bits", dict(W=1 << 16, H=1 << 16)), ("more rows than one launch covers", dict(W=1, H=262141)), ("a basis of another size", dict(basis_size=(5.0, 3.0))),
    ("a null basis", dict(null_basis=True)),
] + [(f"null {n}", dict(null=n)) for n in CUR + OUTS + ("hn", "h1", "h2", "hP", "hN", "hprim")]


@pytest.mark.parametrize("device", [False, True], ids=["host arrays", "device arrays"])
@pytest.mark.parametrize("what,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_on_a_host_only_context(what, kw, device):
    r = prt.HipWavefrontRenderer(device=-1)
    assert _call(r, device=device, **kw) == INVALID, what
    assert capi.lib().prt_last_error(r._ctx).decode().startswith("temporal:")


def test_valid_settings_reach_the_device_check():
    r = prt.HipWavefrontRenderer(device=-1)
    assert _call(r) == NO_DEVICE and _call(r, device=True) == NO_DEVICE
    assert _call(r, max_history=1.0, normal_min=-1.0, plane_tol=0.0) == NO_DEVICE
    assert _call(r, max_history=float("inf"), normal_min=1.0, plane_tol=float("inf")) == NO_DEVICE
    assert _call(r, W=1 << 14, H=1 << 14) == NO_DEVICE                      # exactly 2^28 pixels
    assert _call(r, W=1, H=262140) == NO_DEVICE                              # exactly 65535 blocks of 4 rows
    assert _call(r, null="hc") == NO_DEVICE and _call(r, null="hc", device=True) == NO_DEVICE   # hc NULL: no history at all
    assert _call(r, cfg=C.POINTER(capi.PrtTemporal)()) == NO_DEVICE          # NULL = the defaults
    K, cur, hist = tr.two_planes(8, 6)
    with pytest.raises(prt.PrtError):
        r.temporal_arrays(K, **cur, history=hist)
    with pytest.raises(TypeError):
        r.temporal_arrays(K, **cur, history=hist, sigma=1.0)
    with pytest.raises(ValueError):
        r.temporal_arrays(K, **dict(cur, n=cur["n"][:2]), history=hist)
    with pytest.raises(ValueError):
        r.temporal_arrays(K, **cur, history=dict(hc=hist["hc"]))


def test_film_temporal_on_a_host_only_context():
    L = capi.lib()
    r = prt.HipWavefrontRenderer(device=-1)
    out = np.zeros((3, 4, 3), np.float32)
    po = out.ctypes.data_as(_fp)
    assert L.prt_film_temporal(r._ctx, None, None, po, None, None) == INVALID      # statistics off
    assert b"statistics" in L.prt_last_error(r._ctx)
    r.set_film_statistics(True)
    assert L.prt_film_temporal(r._ctx, None, None, None, None, None) == INVALID    # a null array
    bad = capi.PrtTemporal(0.5, 0.9, 0.01)
    assert L.prt_film_temporal(r._ctx, C.byref(bad), None, po, None, None) == INVALID
    bad_dn = capi.PrtDenoise(7, 4.0, 0.1, 6, 1)
    assert L.prt_film_temporal(r._ctx, None, C.byref(bad_dn), po, None, None) == INVALID and b"iterations" in L.prt_last_error(r._ctx)
    assert L.prt_film_temporal(r._ctx, None, None, po, None, None) == NO_DEVICE
    assert L.prt_set_film(r._ctx, 16, 16, 1, 3) == 0
    assert L.prt_film_temporal(r._ctx, None, None, po, None, None) == INVALID      # a partitioned film, before the device is asked for
    assert b"group form" in L.prt_last_error(r._ctx)
    assert L.prt_film_temporal(None, None, None, po, None, None) == INVALID
    assert L.prt_temporal_reset(None) == INVALID and L.prt_temporal_info(r._ctx, None) == INVALID
    g = prt.HipWavefrontGroupRenderer.__new__(prt.HipWavefrontGroupRenderer)
    with pytest.raises(prt.PrtError, match="group form"):
        prt.HipWavefrontGroupRenderer.temporal_step(g)


def _placed_scene():
    sc = prt.scenes.mesh_scene(prt.Mesh(prt.scenes.asset("icosahedron.ply")))
    body = sc.AddLambertian((0.7, 0.6, 0.5))
    sc.AddInstance(prt.Mesh(prt.scenes.asset("cube_uv.ply")), body, scale=0.5, translation=(1.0, 0.0, 0.0))
    sc.AddInstance(prt.Mesh(prt.scenes.asset("icosahedron.ply")), body, scale=0.25, euler_deg=(0.0, 45.0, 0.0), translation=(-1.0, 0.0, 0.5))
    return sc


def test_what_drops_the_history_and_what_keeps_it():
    L = capi.lib()
    r = prt.HipWavefrontRenderer(device=-1)
    scene = _placed_scene()
    resets = lambda: r.temporal_info().resets  # noqa: E731
    assert resets() == 0 and r.temporal_info().steps == 0 and r.temporal_info().device_bytes == 0
    r.Init(prt.Film(16, 12), scene, prt.Camera(position=(2.0, 1.5, 3.0), width=16, height=12))
    base = resets()
    assert base >= 2                                                         # prt_set_scene and prt_set_film
    other = prt.HipWavefrontRenderer(device=-1)
    other.Init(prt.Film(16, 12), scene, prt.Camera(position=(2.0, 1.5, 3.0), width=16, height=12))
    d = scene.desc()
    drops = [
        ("prt_temporal_reset", r.temporal_reset),
        ("prt_set_scene", lambda: r._check(L.prt_set_scene(r._ctx, C.byref(d)))),
        ("prt_clone_scene", lambda: r._check(L.prt_clone_scene(r._ctx, other._ctx))),
        ("prt_set_film", lambda: r._check(L.prt_set_film(r._ctx, 16, 12, 0, 1))),
        ("prt_refit_meshes", lambda: L.prt_refit_meshes(r._ctx, d.meshes, d.n_meshes)),       # (needs a device: dropped all the same)
        ("prt_set_textures", lambda: r.set_textures(None)),
        ("prt_set_film_statistics on", lambda: r.set_film_statistics(True)),
        ("prt_set_film_statistics off", lambda: r.set_film_statistics(False)),
    ]
    for name, call in drops:
        before = resets()
        call()
        assert resets() == before + 1, name
    keeps = [
        ("prt_set_camera", lambda: r.SetCamera(prt.Camera(position=(2.2, 1.5, 2.9), width=16, height=12))),
        ("prt_set_lens", lambda: r.set_lens(fov_y=0.8)),
        ("prt_set_instance_transforms", lambda: (scene.SetInstanceTransform(0, scale=0.5, translation=(1.2, 0.0, 0.0)), r.UpdateInstances(scene))),
        ("prt_set_film_statistics unchanged", lambda: r.set_film_statistics(False)),
        ("prt_set_sampling", lambda: r.set_sampling(jitter=1)),
        ("prt_film_clear on a host-only context", lambda: L.prt_film_clear(r._ctx)),
    ]
    for name, call in keeps:
        before = resets()
        call()
        assert resets() == before, name


def test_camera_basis_is_the_oracle_basis():
    r = prt.HipWavefrontRenderer(device=-1)
    K = capi.PrtCameraBasis()
    assert capi.lib().prt_get_camera_basis(r._ctx, C.byref(K)) == INVALID   # no camera yet
    import lens_replay as lr
    for pos, front, fov in (((5.0, 5.0, 8.0), None, 0.0), ((-2.0, 0.3, 1.0), (0.3, -0.2, -1.0), 0.7), ((0.0, 9.0, 0.1), (0.0, -1.0, -0.01), 2.5)):
        cam = prt.Camera(position=pos, front=front, width=44, height=28)
        r.set_lens(fov_y=fov)
        r.SetCamera(cam)
        k = r.camera_basis()
        f, rt, up = orc.camera_basis(cam.desc())
        assert np.array_equal(k["front"], f) and np.array_equal(k["right"], rt) and np.array_equal(k["up"], up)
        assert np.array_equal(k["pos"], np.asarray(pos, np.float32)) and k["W"] == 44 and k["H"] == 28
        assert k["tan_fov_y"] == np.float32(lr.tan_fov_y(fov))
        want = tr.basis(pos, cam.front, 44, 28, fov)
        assert all(np.array_equal(np.asarray(k[n]), np.asarray(want[n])) for n in want)
    r.set_lens(fov_y=1.1)                                                    # the lens alone changes tan_fov_y
    assert r.camera_basis()["tan_fov_y"] == np.float32(lr.tan_fov_y(1.1))


def test_prev_surface_on_a_host_only_context():
    r = prt.HipWavefrontRenderer(device=-1)
    P = np.zeros((3, 3), np.float32)
    with pytest.raises(prt.PrtError, match="prt_set_scene"):
        r.temporal_prev_surface(P, P, np.zeros(3, np.int32))
    scene = _placed_scene()
    r.Init(prt.Film(16, 12), scene, prt.Camera(position=(2.0, 1.5, 3.0), width=16, height=12))
    before = [capi.PrtInstance.from_buffer_copy(i) for i in scene.instances]
    scene.SetInstanceTransform(1, scale=0.25 * 2.0 ** -3, euler_deg=(30.0, 45.0, 10.0), translation=(-1.0 + 1000.0, 0.0, 0.5))
    r.UpdateInstances(scene)
    n = len(scene.instances)
    base = r.instances_read()["prim_base"][-n:]
    tris = [scene.instanced_meshes[i.mesh].n_triangles for i in scene.instances]
    rng = np.random.default_rng(1)
    prim = np.concatenate([[-1, 0, 1, 2], np.arange(int(base[0]), int(base[1]) + tris[1])]).astype(np.int32)
    P = rng.uniform(-1, 1, (len(prim), 3)).astype(np.float32)
    N = tr.normalize3(rng.normal(size=(len(prim), 3)).astype(np.float32))
    got_P, got_N = r.temporal_prev_surface(P, N, prim, before)
    want_P, want_N = tr.prev_surface(P, N, prim, base, tris, [np.array(list(i.inv), np.float32) for i in scene.instances],
                                     [np.array(list(i.mat), np.float32) for i in before])
    assert np.array_equal(got_P.view(np.uint32), want_P.view(np.uint32)) and np.array_equal(got_N.view(np.uint32), want_N.view(np.uint32))
    still = prim < int(base[1])                                              # copy 0 did not move: inv . mat is the identity up to rounding
    assert np.array_equal(got_P[:4], P[:4]) and np.allclose(got_P[still], P[still], atol=1e-5) and not np.allclose(got_P[~still], P[~still], atol=1.0)
    assert capi.lib().prt_temporal_prev_surface(r._ctx, 3, None, None, None, None, 0, None, None) == INVALID
    with pytest.raises(prt.PrtError, match="placed copies"):
        r.temporal_prev_surface(P, N, prim, before[:1])


def test_prt_render_refuses_what_the_animation_cannot_do():
    """Checked while the arguments are parsed, before a device is opened."""
    import os
    import subprocess
    import util
    exe = os.path.join(util.ROOT, "parallelraytracing_amd", "csrc", "prt_render")
    for args, word in ((["--temporal"], "--orbit-deg"), (["--frames", "2", "--orbit-deg", "2", "--adaptive", "0.1"], "--adaptive"),
                       (["--frames", "2", "--orbit-deg", "2", "--temporal", "--gpus", "2"], "one GPU")):
        p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and word in p.stderr, (args, p.returncode, p.stderr)
