"""The temporal reprojection on the GPU (include/prt.h "Temporal reprojection").  Every comparison is bit for bit:
prt_temporal_reproject against the numpy restatement (tests/temporal_replay.py) on synthetic arrays at the sizes where the
kernel's blocks and waves are cut differently, the device form against the host form, prt_temporal_prev_surface against numpy,
and prt_film_temporal against the restatement fed with the film, the moments, the features, the basis and the transforms the
context itself reports.  Rendered frames are 44 x 28, 2 samples per frame, depth 5, seed 3."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import denoise_replay as dr
import temporal_replay as tr
import util
from util import prt

pytestmark = pytest.mark.gpu

U32 = np.uint32
F = np.float32
W, H, DEPTH, SEED, SPP = 44, 28, 5, 3, 2
CAM = (2.0, 1.5, 3.0)
OUT = ("c", "n", "m1", "m2", "var")


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(U32), np.ascontiguousarray(b, F).view(U32))


def _diff(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    bad = a.view(U32) != b.view(U32)
    return f"{int(bad.sum())} of {bad.size} values differ, max |a - b| = {float(np.nanmax(np.abs(a - b))):.3e}"


@functools.lru_cache(maxsize=None)
def _device():
    return prt.HipWavefrontRenderer(device=0)


def _orbit(pos, deg):
    a = math.radians(deg)
    return (float(F(pos[0] * math.cos(a) + pos[2] * math.sin(a))), float(pos[1]), float(F(-pos[0] * math.sin(a) + pos[2] * math.cos(a))))


# ---- 1. prt_temporal_reproject against the restatement on synthetic arrays ----------------------------------------------
# 37 x 29: narrower than a wave; 70 x 5: a partial second wave and fewer rows than two blocks; 1 x 1; 130 x 67: several blocks
# both ways.  The previous basis is translated and rotated against the current camera (two_planes), with another fov_y too.
SYNTHETIC = tr.GPU_FIXTURES


@pytest.mark.parametrize("name,w,h,fx,cfg", SYNTHETIC, ids=[s[0] for s in SYNTHETIC])
def test_reproject_equals_the_restatement_bit_for_bit(name, w, h, fx, cfg):
    K, cur, hist = tr.two_planes(w, h, **fx)
    want = tr.reproject(K, **cur, history=hist, **cfg)          # (guard on: a fixture holds no intermediate below 2^-120)
    got = _device().temporal_arrays(K, **cur, history=hist, **cfg)
    for k in OUT:
        assert _same(got[k], want[k]), (k, _diff(got[k], want[k]))
    assert np.array_equal(got["status"], want["status"])
    if w >= 37 and h >= 29 and not fx.get("hn_value") == 0.0:
        kinds = set(np.unique(want["kind"]))
        assert kinds == {0, 1, 2, 3, 4} and (cur["prim"] < 0).any(), kinds    # status 1, behind, off-screen, disoccluded, miss
    if fx.get("hn_value") == 0.0:
        assert (got["status"] == 0).all() and _same(got["c"], cur["c"])
    bare = _device().temporal_arrays(K, **cur, history=hist, return_variance=False, return_status=False, **cfg)   # var_out / status NULL
    assert set(bare) == {"c", "n", "m1", "m2"} and all(_same(bare[k], got[k]) for k in bare)
    none = _device().temporal_arrays(K, **cur, history=None, **cfg)                                               # no history at all
    ref = tr.reproject(K, **cur, history=None, **cfg)
    assert (none["status"] == 0).all() and all(_same(none[k], ref[k]) for k in OUT)


def test_non_finite_positions_take_no_history_and_never_fault():
    K, cur, hist = tr.two_planes(70, 29)
    P = cur["Pprev"].copy()
    spots = [(5, 10), (9, 30), (20, 50), (27, 69)]
    P[5, 10], P[9, 30], P[20, 50], P[27, 69] = np.nan, np.inf, -np.inf, (1e38, -1e38, 1e38)
    hP = hist["hP"].copy()
    hP[12, 33] = np.nan                                         # a tap of other pixels: it only fails their plane test
    want = tr.reproject(K, **cur, history=dict(hist, hP=hP), guard=False)
    assert not _same(want["c"], tr.reproject(K, **cur, history=hist)["c"])
    got = _device().temporal_arrays(K, **dict(cur, Pprev=P), history=dict(hist, hP=hP))
    elsewhere = np.ones((29, 70), bool)
    for (y, x) in spots:
        assert got["status"][y, x] == 0 and _same(got["c"][y, x], cur["c"][y, x]) and _same(got["n"][y, x], cur["n"][y, x])
        elsewhere[y, x] = False
    assert np.array_equal(got["status"][elsewhere], want["status"][elsewhere])
    assert all(_same(got[k][elsewhere], want[k][elsewhere]) for k in OUT) and np.isfinite(got["c"]).all()


# ---- 2. device arrays ----------------------------------------------------------------------------------------------------
def test_reproject_device_on_torch_tensors_equals_the_host_entry():
    import torch
    r = _device()
    K, cur, hist = tr.two_planes(70, 29, fov_y=0.8)
    host = r.temporal_arrays(K, **cur, history=hist)
    dev = torch.device("cuda", 0)
    tc = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cur.items()}
    th = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in hist.items()}
    got = r.temporal_arrays(K, **tc, history=th)
    assert got["c"].device == dev and tuple(got["c"].shape) == (29, 70, 3) and got["status"].dtype == torch.uint8
    for k in OUT:
        assert _same(got[k].cpu().numpy(), host[k]), k
    assert np.array_equal(got["status"].cpu().numpy(), host["status"])
    none = r.temporal_arrays(K, **tc, history=None, return_status=False)
    assert _same(none["c"].cpu().numpy(), cur["c"])
    with pytest.raises(ValueError):
        r.temporal_arrays(K, **dict(tc, prim=tc["prim"].float()), history=th)
    with pytest.raises(ValueError):
        r.temporal_arrays(K, **dict(tc, n=tc["n"][:5]), history=th)


# ---- 3. the moving scene ---------------------------------------------------------------------------------------------------
def _moving_scene():
    """A bunny (a world-space mesh) on the ground under a light, and two placed copies beside it."""
    sc = prt.scenes.mesh_scene(prt.Mesh(prt.scenes.asset("bunny.ply")))
    body, metal = sc.AddLambertian((0.7, 0.3, 0.2)), sc.AddMetal((0.9, 0.9, 0.9), 0.1)
    cube, ico = prt.Mesh(prt.scenes.asset("cube_uv.ply")), prt.Mesh(prt.scenes.asset("icosahedron.ply"))
    sc.AddInstance(cube, body, scale=0.5, euler_deg=(0.0, 30.0, 0.0), translation=(1.1, -0.5, 0.4))
    sc.AddInstance(ico, metal, scale=0.4, euler_deg=(10.0, 0.0, 0.0), translation=(-1.0, -0.4, 0.8))
    return sc


def _renderer(scene, cam_pos=CAM, rank=0, world=1, stats=True, setup=None):
    film = prt.Film(W, H)
    r = prt.HipWavefrontRenderer(device=0, max_depth=DEPTH, seed=SEED, rank=rank, world_size=world)
    r.Init(film, scene, prt.Camera(position=cam_pos, width=W, height=H))
    if setup:
        setup(r)
    if stats:
        r.set_film_statistics(True)
    return r, film


def _copies(r, scene):
    """(prim_base, n_tris, inv (16 floats), mat (16 floats)) of the placed copies as the scene has them now."""
    n = len(scene.instances)
    base = r.instances_read()["prim_base"][-n:]
    tris = [scene.instanced_meshes[i.mesh].n_triangles for i in scene.instances]
    return base, tris, [np.array(list(i.inv), F) for i in scene.instances], [np.array(list(i.mat), F) for i in scene.instances]


def _snapshot(scene):
    return [prt.capi.PrtInstance.from_buffer_copy(i) for i in scene.instances]


def test_prev_surface_follows_the_placed_copies_only():
    scene = _moving_scene()
    r, _ = _renderer(scene)
    before = _snapshot(scene)
    mats_before = [np.array(list(i.mat), F) for i in before]
    scene.SetInstanceTransform(0, scale=0.5 * 2.0 ** -3, euler_deg=(40.0, 70.0, -20.0), translation=(1.1, -0.5, 0.4))   # rotation, scale 2^-3
    scene.SetInstanceTransform(1, scale=0.4, euler_deg=(10.0, 0.0, 0.0), translation=(-1.0 + 1000.0, -0.4, 0.8))          # 10^3 away
    r.UpdateInstances(scene)
    base, tris, inv_cur, _ = _copies(r, scene)
    rng = np.random.default_rng(6)
    n_prims = int(base[0])
    # points of every kind: misses, analytic primitives, the world-space mesh, each copy (first and last triangle too)
    prim = np.concatenate([[-1, -1, 0, 1], rng.integers(2, n_prims, 20), [base[0], base[0] + tris[0] - 1, base[1], base[1] + tris[1] - 1],
                           rng.integers(base[0], base[1] + tris[1], 40)]).astype(np.int32)
    P = rng.uniform(-2, 2, (len(prim), 3)).astype(F)
    P[prim >= int(base[1])] += np.array([1000.0, 0, 0], F)
    N = tr.normalize3(rng.normal(size=(len(prim), 3)).astype(F))
    got_P, got_N = r.temporal_prev_surface(P, N, prim, before)
    want_P, want_N = tr.prev_surface(P, N, prim, base, tris, inv_cur, mats_before)
    assert _same(got_P, want_P), _diff(got_P, want_P)
    assert _same(got_N, want_N), _diff(got_N, want_N)
    still = prim < int(base[0])
    assert still.sum() >= 24 and _same(got_P[still], P[still]) and _same(got_N[still], N[still])     # misses, analytic, world mesh
    assert not (got_P[~still] == P[~still]).all(axis=1).any()
    same_P, same_N = r.temporal_prev_surface(P, N, prim, ())                                          # nothing moved
    assert _same(same_P, P) and _same(same_N, N)
    with pytest.raises(prt.PrtError, match="placed copies"):
        r.temporal_prev_surface(P, N, prim, before[:1])


ROUTES = {
    "plain": None,
    "jitter": lambda r: r.set_sampling(jitter=1),
    "mis": lambda r: r.set_lighting("mis"),
}


def _film_state(r, film):
    r.download()
    A, Q = r.film_statistics()
    return film.accum.copy(), film.weights.copy(), A, Q


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_film_temporal_equals_the_restatement_over_four_moving_frames(route):
    scene = _moving_scene()
    r, film = _renderer(scene, setup=ROUTES[route])
    hist, Kprev, prev_mats, pos = None, None, None, CAM
    reprojected = []
    for f in range(4):
        if f:
            pos = _orbit(pos, 2.0)
            r.SetCamera(prt.Camera(position=pos, width=W, height=H))
            scene.SetInstanceTransform(0, scale=0.5, euler_deg=(0.0, 30.0 + 8.0 * f, 0.0), translation=(1.1 + 0.05 * f, -0.5, 0.4))
            r.UpdateInstances(scene)
            film.Clear()
        r.ProgressiveRender(SPP)
        state = _film_state(r, film)
        dn_before = r.denoise()
        feat = r.render_features()
        K = r.camera_basis()
        base, tris, inv_cur, mats = _copies(r, scene)
        denoise = {} if f >= 2 else None                                   # frames 0, 1: the blend itself; 2, 3: through the a-trous filter
        got, got_var, got_n = r.temporal_step(return_variance=True, return_history=True, denoise=denoise)
        after = _film_state(r, film)
        assert all(_same(a, b) for a, b in zip(state, after)), f           # film and moments: not a bit
        assert _same(r.denoise(), dn_before), f                            # ... nor prt_film_denoise's own result
        c, n = tr.frame_inputs(*state)
        Pp, Np = (feat["position"], feat["normal"]) if hist is None else tr.prev_surface(feat["position"], feat["normal"], feat["prim"], base, tris,
                                                                                          inv_cur, prev_mats)
        want = tr.reproject(Kprev if Kprev is not None else K, c, n, state[2], state[3], feat["prim"], Pp, Np, history=hist, guard=False)
        info = r.temporal_info()
        assert info.steps == f + 1 and info.hit_pixels == int((feat["prim"] >= 0).sum()) and info.reprojected == int(want["status"].sum()), f
        assert info.device_bytes >= 2 * 56 * W * H
        assert _same(got_n, want["n"]), (f, _diff(got_n, want["n"]))
        if denoise is None:
            assert _same(got, want["c"]), (f, _diff(got, want["c"]))
            assert _same(got_var, want["var"]), (f, _diff(got_var, want["var"]))
        else:
            wd, wv = dr.denoise(want["c"], want["var"], feat["albedo"], feat["normal"], feat["position"], feat["prim"], guard=False)
            assert _same(got, wd), (f, _diff(got, wd))
            assert _same(got_var, wv), (f, _diff(got_var, wv))
        if f == 0:
            assert (want["status"] == 0).all() and _same(got, film.mean())  # no history: the film mean
        reprojected.append(int(want["status"].sum()))
        hist = tr.next_history(want, feat["position"], feat["normal"], feat["prim"])
        Kprev, prev_mats = K, mats
    moved = (feat["prim"] >= int(base[0])) & (feat["prim"] < int(base[0]) + tris[0])
    print(route, reprojected, int(moved.sum()))
    assert min(reprojected[1:]) > 0.5 * W * H and moved.sum() > 5 and want["status"][moved].any()   # the moving copy keeps its history


def test_the_first_step_after_a_reset_is_prt_film_denoise():
    r, film = _renderer(_moving_scene())
    r.ProgressiveRender(SPP)
    want, want_var = r.denoise(return_variance=True)
    got, got_var = r.temporal_step(return_variance=True, denoise={})
    assert _same(got, want) and _same(got_var, want_var)                    # no history: the variance is the existing rule
    r.temporal_step()                                                       # (now there is one)
    assert r.temporal_info().reprojected > 0
    r.temporal_reset()
    again = r.temporal_step(denoise=dict(iterations=3, sigma_l=2.0))
    assert _same(again, r.denoise(iterations=3, sigma_l=2.0)) and r.temporal_info().reprojected == 0
    r.temporal_reset()
    r.download()
    assert _same(r.temporal_step(denoise=None), film.mean())


def test_what_drops_the_history_and_what_keeps_it():
    scene = _moving_scene()
    r, film = _renderer(scene)
    L = prt.capi.lib()

    def step():
        r.ProgressiveRender(1)
        r.temporal_step()
        return r.temporal_info().reprojected
    step()
    assert step() > 0
    keeps = {
        "SetCamera": lambda: r.SetCamera(prt.Camera(position=_orbit(CAM, 2.0), width=W, height=H)),
        "set_lens": lambda: r.set_lens(fov_y=0.9),
        "UpdateInstances": lambda: (scene.SetInstanceTransform(1, scale=0.4, euler_deg=(10.0, 20.0, 0.0), translation=(-1.0, -0.4, 0.9)),
                                    r.UpdateInstances(scene)),
    }
    for name, call in keeps.items():
        call()
        assert step() > 0.5 * W * H, name
    drops = {
        "temporal_reset": r.temporal_reset,
        "prt_set_film": lambda: r._check(L.prt_set_film(r._ctx, W, H, 0, 1)),
        "set_textures": lambda: r.set_textures(None),
        "Refit (refused: this scene has placed copies; the history goes all the same)": lambda: pytest.raises(prt.PrtError, r.Refit, scene),
        "set_film_statistics": lambda: (r.set_film_statistics(False), r.set_film_statistics(True)),
        "prt_set_scene": lambda: r.Init(film, scene, prt.Camera(position=CAM, width=W, height=H)),
    }
    for name, call in drops.items():
        call()
        assert step() == 0 and r.temporal_info().steps == 1, name
        assert step() > 0, name
    other, _ = _renderer(scene)
    r._check(L.prt_clone_scene(r._ctx, other._ctx))
    assert step() == 0
    # a refit that succeeds: a scene of world-space meshes only
    plain = prt.scenes.mesh_scene(prt.Mesh(prt.scenes.asset("icosahedron.ply")))
    r, film = _renderer(plain)
    step()
    assert step() > 0
    r.Refit(plain)
    assert step() == 0 and step() > 0


def test_refusals():
    scene = prt.Scene("CORNELL")
    r, _ = _renderer(scene, stats=False)
    r.ProgressiveRender(1)
    with pytest.raises(prt.PrtError, match="statistics"):
        r.temporal_step()
    rp, _ = _renderer(scene, rank=1, world=3)
    rp.ProgressiveRender(1)
    with pytest.raises(prt.PrtError, match="group form"):
        rp.temporal_step()
    g = prt.HipWavefrontGroupRenderer([0, 0], max_depth=DEPTH, seed=SEED)
    g.Init(prt.Film(W, H), scene, prt.Camera(position=CAM, width=W, height=H))
    with pytest.raises(prt.PrtError, match="group form"):
        g.temporal_step()
    with pytest.raises(prt.PrtError, match="max_history"):
        _renderer(scene)[0].temporal_step(max_history=0.5)


def test_prt_render_writes_the_python_sequence(tmp_path):
    exe = os.path.join(util.ROOT, "parallelraytracing_amd", "csrc", "prt_render")
    out = str(tmp_path / "anim")
    p = subprocess.run([exe, "--preset", "CORNELL", "--width", str(W), "--height", str(H), "--depth", str(DEPTH), "--seed", str(SEED),
                        "--camera", "5", "5", "8", "--spp", str(SPP), "--frames", "3", "--orbit-deg", "2", "--temporal", "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    film = prt.Film(W, H)
    r = prt.HipWavefrontRenderer(device=0, max_depth=DEPTH, seed=SEED)
    r.Init(film, prt.Scene("CORNELL"), prt.Camera(position=(5.0, 5.0, 8.0), front=(-5.0, -5.0, -8.0), width=W, height=H))
    r.set_film_statistics(True)
    differs = 0
    for f in range(3):
        a = math.radians(2.0 * f)
        pos = (float(F(5.0 * math.cos(a) + 8.0 * math.sin(a))), 5.0, float(F(-5.0 * math.sin(a) + 8.0 * math.cos(a))))
        r.SetCamera(prt.Camera(position=pos, front=tuple(-v for v in pos), width=W, height=H))
        film.Clear()
        r.frame_index = f * SPP
        r.ProgressiveRender(SPP)
        r.download()
        assert _same(prt.read_pfm(f"{out}_f{f:03d}.pfm"), film.mean()), f
        want = r.temporal_step()
        assert _same(prt.read_pfm(f"{out}_f{f:03d}_temporal.pfm"), want), f
        differs += int(not _same(want, film.mean()))
    assert differs == 2                                                      # frames 1 and 2 carry history
