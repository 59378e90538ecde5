"""A path's last segment as a decision of the analytic scan (DESIGN.md section 3 "The last segment"; prt_set_param
("last_segment", 0 | 1 | 2)).  With no emissive triangle in the scene the film gets throughput x 0 from a last segment whose
analytic hit does not emit, whatever the tree walk would find, so setting 1 ends such a segment in the shade launch that
produces it and the last shade launch does not rebuild a triangle hit; setting 2 also answers the rays that are still walked
with the any-hit walk seeded by their analytic hit (k_occluded8_seeded).  Setting 0 walks and shades every ray.

Everything here is bit for bit: the three settings against each other (film sums, weights, rays_total, per-depth ray counts) and
against the oracle (with textures the replay tests/texture_replay.py, with an environment image tests/environment_replay.py).
So that nothing passes vacuously, the rays handed to the last tree walk (HipWavefrontRenderer.last_segment) must be fewer under settings 1 and 2 and not zero, and the oracle's own
paths must hold all three classes of last-segment ray: rays that cannot enter the mesh bounds before their analytic hit, rays
that can and whose analytic hit is the Lambertian ground, and rays that can and whose analytic hit is a miss or the light.

Base scene: icosahedron.ply on a Lambertian ground quad under an emissive quad, sky (0.4, 0.3, 0.6), 64 x 48 pixels."""
import functools

import numpy as np
import pytest

import environment_replay as er
import lighting_replay as lr
import texture_replay as tr
import util
from parallelraytracing_amd import scenes
from util import orc, prt

pytestmark = pytest.mark.gpu

W, H, SEED = 64, 48, 5
SKY = (0.4, 0.3, 0.6)
CAM_POS = (2.0, 1.5, 3.0)
SETTINGS = (0, 1, 2)
F = np.float32


def _cam(pos=CAM_POS):
    return prt.Camera(position=pos, width=W, height=H)


def _scene(kind="ico"):
    """ground quad (Lambertian), emissive quad above it, and per kind the triangles."""
    sc = prt.Scene(preset=None, sky=SKY)
    ground = sc.AddLambertian((0.5, 0.5, 0.5))
    light = sc.AddEmissive((15.0, 15.0, 15.0))
    body = sc.AddLambertian((0.8, 0.7, 0.6))
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    ico = prt.Mesh(scenes.asset("icosahedron.ply"))
    if kind == "ico":
        sc.AddMesh(ico, body)
    elif kind == "bunny":  # a tree deep enough for the stack_cap hook to overflow
        sc.AddMesh(prt.Mesh(scenes.asset("bunny.ply")), body)
    elif kind == "placed":  # placed copies only (the INST instances), one of them metal
        metal = sc.AddMetal((0.9, 0.8, 0.6), 0.1)
        for k in range(3):
            sc.AddInstance(ico, metal if k == 1 else body, scale=0.6, euler_deg=(10.0 * k, 25.0 * k, 0.0),
                           translation=(1.4 * k - 1.4, -0.2, 0.0))
    elif kind == "many":  # more than 16 analytic primitives with a mesh (the ABVH instances): 18 small spheres, one emissive
        sc.AddMesh(ico, body)
        glow = sc.AddEmissive((3.0, 2.0, 1.0))
        for k in range(18):
            a = 2.0 * np.pi * k / 18.0
            sc.AddCircle(0.2, glow if k == 4 else ground, translation=(2.2 * float(np.cos(a)), -0.6 + 0.05 * k, 2.2 * float(np.sin(a))))
    elif kind == "coplanar":  # two triangles in the emissive quad's plane, covering its middle, and the icosahedron
        sc.AddMesh(ico, body)
        v = np.array([[-1.0, 5.0, -1.0], [1.0, 5.0, -1.0], [-1.0, 5.0, 1.0], [1.0, 5.0, 1.0]], F)
        n = np.tile(np.array([[0.0, -1.0, 0.0]], F), (4, 1))
        sc.AddMesh(prt.Mesh(vertices=v, normals=n, indices=np.array([[0, 2, 1], [1, 2, 3]], np.uint32)), body)
    elif kind == "emissive_mesh":  # fallback: a triangle emits
        sc.AddMesh(ico, sc.AddEmissive((2.0, 3.0, 4.0)))
    else:
        raise ValueError(kind)
    return sc


@functools.lru_cache(maxsize=None)
def _scene_cached(kind):
    return _scene(kind)


def _sampling(r, sampling):
    return r.set_sampling(*sampling) if sampling != (0, 0, 0.0) else None


def _render(scene, setting, depth, S, sampling=(0, 0, 0.0), params=(), cam=None, lighting=None, env=None, seed=SEED, w=W, h=H):
    """One batch of S samples -> (accum, weights, rays_total, per-depth counts, (route setting taken, rays of the last walk), shade instance)"""
    film = prt.Film(w, h)
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=seed)
    r.Init(film, scene, cam or _cam())
    r.set_param("last_segment", setting)
    for k, v in params:
        r.set_param(k, v)
    _sampling(r, sampling)
    if lighting:
        r.set_lighting(lighting)
    if env is not None:
        r.set_environment(env, 0.5)
    r.set_samples_in_flight(S)
    r.ProgressiveRender(S)
    last = r.last_segment()
    r.download()
    st = r.stats()
    return film.accum.copy(), film.weights.copy(), int(st.rays_total), [int(x) for x in st.rays_per_depth], last, r.shade_instance()


@functools.lru_cache(maxsize=None)
def _oracle(kind, depth, S, sampling=(0, 0, 0.0), cam_pos=CAM_POS):
    sp = prt.capi.PrtSampling(int(sampling[0]), int(sampling[1]), float(sampling[2])) if sampling != (0, 0, 0.0) else None
    acc, wts, rays = util.oracle_scene(_scene_cached(kind)).render(_cam(cam_pos).desc(), W, H, spp=S, max_depth=depth, seed=SEED, iterative=True,
                                                                   use_bvh=True, n_threads=8, sampling=sp)
    for a in (acc, wts):
        a.setflags(write=False)
    return acc, wts, rays


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3] == b[3]


def _check_settings(kind, depth, S, sampling=(0, 0, 0.0), params=(), oracle=True, expect_on=True, instance=None):
    got = {s: _render(_scene_cached(kind), s, depth, S, sampling, params) for s in SETTINGS}
    for s in SETTINGS[1:]:
        assert _same(got[s], got[0]), (kind, depth, S, sampling, s)
    on = expect_on and depth >= 2
    assert [got[s][4][0] for s in SETTINGS] == [s if on else 0 for s in SETTINGS]
    if instance:
        assert all(got[s][5] == instance for s in SETTINGS), got[1][5]
    if oracle:
        acc, wts, rays = _oracle(kind, depth, S, sampling)
        for s in SETTINGS:
            assert np.array_equal(got[s][0], acc) and np.array_equal(got[s][1], wts) and got[s][2] == rays, (kind, depth, S, sampling, s)
    print(dict(kind=kind, depth=depth, S=S, sampling=sampling, last_walk_rays={s: got[s][4][1] for s in SETTINGS}), flush=True)
    if on:  # the skip happens, and the walk still has rays to answer
        assert 0 < got[1][4][1] < got[0][4][1] and got[2][4][1] == got[1][4][1], (got[0][4], got[1][4], got[2][4])
    else:
        assert got[1][4][1] == got[0][4][1] == got[2][4][1]
    return got


# 1: a one-sample batch; 8: the smallest pixel-major batch; 64: one full sample group; 70: a full group and a partial one
@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("S", [1, 8, 64, 70])
@pytest.mark.parametrize("depth", [1, 2, 3, 5])
def test_settings_agree_with_each_other_and_with_the_oracle(depth, S, jitter):
    _check_settings("ico", depth, S, (jitter, 0, 0.0))


def test_the_oracle_paths_hold_all_three_classes_of_last_segment():
    """The last segments (index DEPTH - 1) of the oracle's own paths, classified on the CPU: the analytic scan is the closest
    hit in the scene without its mesh; "enters" is a float64 slab test against the mesh bounds shrunk / grown by 2 %, so that
    rounding cannot move a ray across."""
    depth, S = 3, 8
    sc = _scene_cached("ico")
    pix = np.tile(np.arange(W * H), S)
    samp = np.repeat(np.arange(S), W * H)
    verts, _, _, _ = lr.walk(sc, util.oracle_scene(sc), _cam(), W, H, depth, SEED, pix, samp, use_bvh=True)
    assert len(verts) == depth
    o, d = verts[depth - 1]["o"], verts[depth - 1]["d"]
    bare = prt.Scene(preset=None, sky=SKY)
    bare.materials = list(sc.materials)
    bare.primitives = list(sc.primitives)
    h = util.oracle_scene(bare).closest_hit(o, d)
    V = prt.Mesh(scenes.asset("icosahedron.ply")).GetVertices().astype(np.float64)
    c, e = (V.min(0) + V.max(0)) / 2, (V.max(0) - V.min(0)) / 2

    def enters(lo, hi):
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - o.astype(np.float64)) / d.astype(np.float64), (hi - o.astype(np.float64)) / d.astype(np.float64)
        tn, tf = np.maximum(np.minimum(t0, t1).max(1), 0.0), np.maximum(t0, t1).min(1)
        return (tn <= tf), tn

    inside, t_in = enters(c - 0.98 * e, c + 0.98 * e)
    outside = ~enters(c - 1.02 * e, c + 1.02 * e)[0]
    miss = h["prim"] < 0
    emissive = h["prim"] == 1
    ground = h["prim"] == 0
    behind = np.sqrt(h["d2"].astype(np.float64)) > 1.02 * t_in + 1e-3
    n_back = int(outside.sum())
    n_front_ground = int((inside & ground & behind).sum())
    n_front_open = int((inside & (miss | (emissive & behind))).sum())
    print(dict(last_segments=len(o), back=n_back, front_ground=n_front_ground, front_miss_or_light=n_front_open), flush=True)
    assert n_back > 0 and n_front_ground > 0 and n_front_open > 0


def test_placed_copies():
    _check_settings("placed", 4, 8, instance="k_shade<0, true, true, false, false>")


def test_more_than_16_analytic_primitives_with_a_mesh():
    _check_settings("many", 4, 8, instance="k_shade<0, true, false, true, false>")


def test_roulette_with_clamp_and_jitter():
    _check_settings("ico", 5, 8, (1, 2, 0.75), instance="k_shade<0, true, false, false, false>")


def test_stack_overflow_path():
    """stack_cap 1: rays overflow the 8-wide kernel's stack and finish in the 4-wide closest-hit walk from the seeded bound.
    That rays do overflow: the instrumented walk of the same batch reports stacks deeper than the cap."""
    _check_settings("bunny", 3, 8, params=(("stack_cap", 1),))
    for s in SETTINGS:
        r = prt.HipWavefrontRenderer(device=0, max_depth=3, seed=SEED)
        r.Init(prt.Film(W, H), _scene_cached("bunny"), _cam())
        r.set_param("last_segment", s)
        r.set_param("stack_cap", 1)
        r.set_param("measure_spp", 8)
        assert int(r.measure_traversal().max_stack_used) > 1


def test_triangles_in_the_plane_of_the_emissive_quad():
    """The tie rule: where a triangle and the emissive quad lie at the same distance, the lower primitive index (the quad) wins
    on equal keys and rounding decides the rest; both settings and the oracle must agree on every such ray."""
    got = _check_settings("coplanar", 3, 8)
    base = _oracle("ico", 3, 8)
    assert not np.array_equal(got[0][0], base[0])  # the two triangles do change what the paths see


def test_environment_image_against_the_replay():
    """A non-constant map, every setting: each pixel sample whose path misses at a stable direction equals the replay's fp32 term
    bit for bit, as do the paths that end on a surface (tests/test_gpu_environment.py: at most 0.5 % of the samples left out), the
    segment count is the replay's, and the settings agree on every pixel, the left-out ones included."""
    sc, cam, depth = _scene_cached("ico"), _cam(), 3
    env = er.EnvMap(er.named_map("lognormal"))
    rep = er.replay(sc, env, cam, W, H, depth, SEED, lr.SAMPLES, "off", use_bvh=True)
    stable = ~rep.miss_unstable
    assert rep.n_misses > 0.1 * len(rep.pix) and 1.0 - stable.mean() <= 0.005
    frames, fronts = {}, {}
    for s in SETTINGS:
        film = prt.Film(W, H)
        r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=SEED)
        r.Init(film, sc, cam)
        r.set_param("last_segment", s)
        r.set_environment(env.rgb, 0.5)
        r.reset_stats()
        frames[s] = lr.render_samples(r, film, lr.SAMPLES)
        fronts[s] = r.last_segment()
        assert int(r.stats().rays_total) == rep.segments and r.shade_instance() == "k_shade_env<false, false>"
        for k in lr.SAMPLES:
            sel = (rep.samp == k) & stable
            got = frames[s][k].reshape(-1, 3)[rep.pix[sel]]
            assert np.array_equal(got.view(np.uint32), rep.delivered[sel].view(np.uint32)), (s, k)
            assert frames[s][k].tobytes() == frames[0][k].tobytes(), (s, k)
    assert [fronts[s][0] for s in SETTINGS] == list(SETTINGS) and 0 < fronts[1][1] < fronts[0][1] and fronts[2][1] == fronts[1][1]


def test_textured_materials_against_the_replay():
    c = tr.scene_a()
    want, wwts, per_depth = tr.frame(c["scene"], orc.OracleScene(c["scene"].desc()), c["cam"], c["W"], c["H"], c["depth"], tr.SEED, 0, 4)
    got = {s: _render(c["scene"], s, c["depth"], 4, cam=c["cam"], seed=tr.SEED, w=c["W"], h=c["H"]) for s in SETTINGS}
    for s in SETTINGS:
        assert np.array_equal(got[s][0].view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32)) and np.array_equal(got[s][1], wwts)
        assert got[s][3][:c["depth"]] == per_depth.tolist() and got[s][2] == int(per_depth.sum())
        assert got[s][4][0] == s and got[s][5].startswith("k_shade_tex<")
    assert 0 < got[1][4][1] < got[0][4][1] and got[2][4][1] == got[1][4][1]


@pytest.mark.parametrize("kind", ["emissive_mesh", "emissive_copy"])
def test_an_emissive_triangle_keeps_the_route_off(kind):
    if kind == "emissive_copy":
        c = lr.case("placed", W, H)
        sc, cam = c["scene"], c["cam"]
    else:
        sc, cam = _scene_cached(kind), _cam()
    acc, wts, rays = util.oracle_scene(sc).render(cam.desc(), W, H, spp=8, max_depth=4, seed=SEED, iterative=True, use_bvh=True, n_threads=8)
    for s in SETTINGS:
        a = _render(sc, s, 4, 8, cam=cam)
        assert a[4][0] == 0, "the route must be off"
        assert np.array_equal(a[0], acc) and np.array_equal(a[1], wts) and a[2] == rays


def test_lighting_keeps_the_route_off():
    sc = _scene_cached("ico")
    got = {s: _render(sc, s, 4, 8, lighting="mis") for s in SETTINGS}
    assert got[0][4] == got[1][4] and got[1][4][0] == 0
    assert _same(got[1], got[0])
