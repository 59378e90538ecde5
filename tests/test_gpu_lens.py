"""The thin-lens camera (include/prt.h "Thin lens and field of view") on one MI355X.

  1. rays: prt_camera_rays_lens against the float64 restatement (tests/lens_replay.py), bounds from the header's arithmetic:
     about ten dependent fp32 roundings of half an ulp plus sinf / cosf / sqrtf at a few ulp -> directions 16 * 2^-24 per
     component, origins 8 * 2^-24 (|pos|_inf + aperture), and every ray within 32 * 2^-24 f of its pixel's point on the
     plane in focus.
  2. frames, bit for bit: the library's own rays traced by the oracle (orc.trace, iterative), summed per pixel in sample order
     in fp32; stats().rays_per_depth = the traces' segment counts.  Four scenes x jitter 0 / 1 x 1, 3 and 9 samples per call.
  3. the frame does not depend on a tunable, on batching or on the partition.
  4. the all-zero lens and fov_y = 1 are the camera without a lens, bit for bit; fov_y alone passes (2) on the compact route.
  5. roulette + clamp, light sampling and an environment image under a lens, through the existing replays fed with the lens
     rays.
  6. the defocused edge of tests/test_lens_host.py on the device: every sample's hit or miss, and the columns' means.
  7. the group renderer and the prt_render command line."""
import math
import os
import subprocess

import numpy as np
import pytest

import environment_replay as er
import lens_replay as lp
import lighting_replay as lr
import util
from util import orc, prt

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEED = 5
SPP = 9                       # crosses both the slot reservation (2 rays) and the sample group of a block (8)


def _renderer(scene, cam, W, H, depth, lens=None, jitter=0, seed=SEED, sif=4, rank=0, world=1, sampling=None):
    film = prt.Film(W, H)
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=seed, rank=rank, world_size=world)
    if lens is not None:
        r.set_lens(*lens)                    # before Init: it stays across scene, film and camera
    r.Init(film, scene, cam)
    r.set_samples_in_flight(sif)
    if sampling is not None:
        r.set_sampling(*sampling)
    elif jitter:
        r.set_sampling(jitter=1)
    return r, film


def _library_rays(r, W, H, seed, n_samples, jitter):
    """The render's own primary rays of every pixel for samples 0 .. n_samples - 1 and the paths' states after them."""
    pix = np.tile(np.arange(W * H), n_samples)
    samp = np.repeat(np.arange(n_samples), W * H)
    keys = lp.path_seeds(pix, samp, seed)
    px, py, keys = lp.jittered_points(pix, W, keys, jitter)
    o, d, keys = r.camera_rays_lens(px, py, keys)
    return pix, samp, o, d, keys


def _traces(osc, o, d, keys, depth, use_bvh):
    L = np.empty((len(o), 3), np.float32)
    segs = np.empty(len(o), np.int64)
    for i in range(len(o)):
        L[i], segs[i], _ = osc.trace(o[i], d[i], depth, int(keys[i]), iterative=True, use_bvh=use_bvh)
    return L, segs


def _sum_in_sample_order(L, W, H, n_samples):
    acc = np.zeros((H * W, 3), np.float32)
    for s in range(n_samples):
        acc += L[s * W * H:(s + 1) * W * H]
    return acc.reshape(H, W, 3)


# ---- 1. rays ------------------------------------------------------------------------------------------------------------------
RAY_CAM = dict(position=(3.0, 2.5, 6.0), front=(-0.4, -0.3, -1.0), width=9, height=7)
RAY_LENSES = [(0.6, 0.0, 0.0), (0.0, 0.3, 5.0), (0.8, 0.3, 5.0)]


def _ray_inputs():
    gy, gx = np.mgrid[0:7, 0:9]
    rng = np.random.default_rng(9)
    keys = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    px = np.repeat((gx.ravel() + 0.37).astype(np.float32), 64)
    py = np.repeat((gy.ravel() + 0.61).astype(np.float32), 64)
    return px, py, np.tile(keys, 63)


@pytest.fixture(scope="module")
def ray_renderer():
    cam = prt.Camera(RAY_CAM["position"], front=prt.glm_normalize(np.array(RAY_CAM["front"], np.float32)), width=9, height=7)
    r, _ = _renderer(prt.Scene("CORNELL"), cam, 9, 7, 2)
    return r, cam


@pytest.mark.parametrize("lens", RAY_LENSES)
def test_rays_match_the_restatement(ray_renderer, lens):
    r, cam = ray_renderer
    px, py, keys = _ray_inputs()
    r.set_lens(*lens)
    o, d, after = r.camera_rays_lens(px, py, keys)
    wo, wd, wafter = lp.lens_rays(cam, lens, px, py, keys)
    fov, ap, f = lens
    if ap > 0:
        assert np.array_equal(after, lp.pcg(lp.pcg(keys)).astype(np.uint32))
    else:
        assert np.array_equal(after, keys)
    assert np.array_equal(after, wafter)
    pos = np.asarray(cam.position, np.float64)
    d_err = float(np.abs(d - wd).max())
    o_err = float(np.abs(o - wo).max())
    d_tol = 16 * U
    o_tol = 8 * U * (np.abs(pos).max() + ap)
    print(f"lens {lens}: direction error {d_err / d_tol:.3f} of its bound, origin error {o_err / o_tol:.3f} of its bound")
    assert d_err <= d_tol and o_err <= o_tol
    if ap > 0:
        # every ray of a pixel passes through the pixel's pinhole point on the plane in focus
        front = orc.camera_basis(cam.desc())[0].astype(np.float64)
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        s = (f - (o64 - pos) @ front) / (d64 @ front)
        P = o64 + s[:, None] * d64
        _, d0, _ = lp.lens_rays(cam, (fov, 0.0, 0.0), px, py, keys)
        P0 = pos + (f / (d0 @ front))[:, None] * d0
        p_err = float(np.abs(P - P0).max())
        print(f"lens {lens}: focus point error {p_err / (32 * U * f):.3f} of its bound")
        assert p_err <= 32 * U * f
        assert np.abs(o64 - pos).max() > 0.5 * ap          # the origins do leave the camera position
    r.set_lens()


def test_the_zero_lens_gives_the_pinhole_rays_bit_for_bit(ray_renderer):
    r, _ = ray_renderer
    px, py, keys = _ray_inputs()
    r.set_lens()
    o, d, after = r.camera_rays_lens(px, py, keys)
    o0, d0 = r.camera_rays(px, py)
    assert np.array_equal(after, keys)
    assert np.array_equal(o.view(np.uint32), o0.view(np.uint32)) and np.array_equal(d.view(np.uint32), d0.view(np.uint32))
    r.set_lens(fov_y=1.0)
    o1, d1, _ = r.camera_rays_lens(px, py, keys)
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32)) and np.array_equal(o1, o0)
    r.set_lens()


# ---- 2. frames, bit for bit ---------------------------------------------------------------------------------------------------
def _bunny_scene():
    return prt.scenes.mesh_scene(prt.scenes.refined("bunny.ply", 4000))


def _placed_scene():
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.5, 0.5, 0.5))
    light = sc.AddEmissive((15.0, 15.0, 15.0))
    body = sc.AddLambertian((0.8, 0.7, 0.6))
    glass = sc.AddDielectric(1.5)
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    ico = prt.Mesh(prt.scenes.asset("icosahedron.ply")).refine(300)
    sc.AddInstance(ico, body, scale=0.8, euler_deg=(10.0, 25.0, 0.0), translation=(-0.9, 0.0, 0.0))
    sc.AddInstance(ico, glass, scale=0.6, euler_deg=(0.0, 50.0, 20.0), translation=(0.9, -0.2, 0.6))
    return sc


def _frame_case(name):
    """-> scene, camera, W, H, depth, lens, use_bvh (for the oracle's traces)"""
    if name == "DEFAULT":          # partial tiles
        return prt.Scene("DEFAULT"), prt.Camera(width=70, height=45), 70, 45, 4, (0.0, 0.2, 9.0), False
    if name == "bunny":
        return _bunny_scene(), prt.Camera((2.0, 1.5, 3.0), width=64, height=48), 64, 48, 5, (0.0, 0.06, 3.6), True
    if name == "placed":           # two placed copies: the two-level tree
        return _placed_scene(), prt.Camera((1.5, 1.5, 4.0), width=64, height=48), 64, 48, 5, (0.8, 0.08, 4.2), True
    if name == "balls":            # many analytic primitives: the ABVH instances
        return prt.Scene("RANDOM_BALLS_LARGE"), prt.Camera(width=48, height=32), 48, 32, 4, (0.0, 0.25, 10.0), False
    raise ValueError(name)


def _check_frames(scene, cam, W, H, depth, lens, use_bvh, jitter, spps=(1, 3, SPP)):
    r, film = _renderer(scene, cam, W, H, depth, lens, jitter)
    pix, samp, o, d, keys = _library_rays(r, W, H, SEED, SPP, jitter)
    L, segs = _traces(orc.OracleScene(scene.desc()), o, d, keys, depth, use_bvh)
    for spp in spps:
        film.Clear()
        r.frame_index = 0
        r.reset_stats()
        r.ProgressiveRender(spp)
        r.download()
        want = _sum_in_sample_order(L, W, H, spp)
        assert np.array_equal(film.accum.view(np.uint32), want.view(np.uint32)), (jitter, spp)
        assert np.all(film.weights == np.float32(spp))
        st = r.stats()
        sg = segs[:spp * W * H]
        assert [int(st.rays_per_depth[k]) for k in range(depth + 1)] == [int((sg > k).sum()) for k in range(depth + 1)]
        assert st.rays_total == int(sg.sum())
    return r, film


@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("name", ["DEFAULT", "bunny", "placed", "balls"])
def test_lens_frames_equal_the_oracles_traces_of_the_librarys_rays(name, jitter):
    scene, cam, W, H, depth, lens, use_bvh = _frame_case(name)
    r, _ = _check_frames(scene, cam, W, H, depth, lens, use_bvh, jitter)
    # the origins differ from sample to sample: it is a lens
    _, _, o, _, _ = _library_rays(r, W, H, SEED, 2, jitter)
    assert np.abs(o[:W * H] - o[W * H:]).max() > 0.1 * lens[1]


# ---- 3. invariance ------------------------------------------------------------------------------------------------------------
def _bunny_frame(jitter, setup=None, calls=(SPP,), sif=4, rank=0, world=1):
    scene, cam, W, H, depth, lens, _ = _frame_case("bunny")
    r, film = _renderer(scene, cam, W, H, depth, lens, jitter, sif=sif, rank=rank, world=world)
    if setup:
        setup(r)
    for c in calls:
        r.ProgressiveRender(c)
    r.download()
    return r, film.accum.copy(), film.weights.copy()


@pytest.fixture(scope="module")
def bunny_base():
    out = {}
    for jitter in (0, 1):
        r, acc, wts = _bunny_frame(jitter)
        out[jitter] = (acc, wts, [int(v) for v in r.stats().rays_per_depth])
    return out


VARIANTS = {
    "sif1": dict(sif=1),
    "nine_calls": dict(calls=(1,) * SPP),
    "compact_primary0": dict(setup=lambda r: r.set_param("compact_primary", 0)),
    "primary_walk0": dict(setup=lambda r: r.set_param("primary_walk", 0)),
    "path_kernel2": dict(setup=lambda r: r.set_param("path_kernel", 2)),
    "fuse0": dict(setup=lambda r: r.set_param("fuse", 0)),
    "fuse1": dict(setup=lambda r: r.set_param("fuse", 1)),
    "exact_grids2": dict(setup=lambda r: r.set_param("exact_grids", 2)),
    "exact_grids0": dict(setup=lambda r: r.set_param("exact_grids", 0)),
    "wide1": dict(setup=lambda r: r.set_param("wide", 1)),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_lens_frame_does_not_depend_on_a_tunable_or_on_batching(bunny_base, variant):
    for jitter in (0, 1):
        r, acc, wts = _bunny_frame(jitter, **VARIANTS[variant])
        want, wwts, rays = bunny_base[jitter]
        assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)) and np.array_equal(wts, wwts), (variant, jitter)
        assert [int(v) for v in r.stats().rays_per_depth] == rays, (variant, jitter)


def test_two_rank_partition_adds_up_to_the_one_rank_frame(bunny_base):
    for jitter in (0, 1):
        want, wwts, rays = bunny_base[jitter]
        acc = np.zeros_like(want)
        wts = np.zeros_like(wwts)
        per_depth = np.zeros(len(rays), np.int64)
        for rank in (0, 1):
            r, a, w = _bunny_frame(jitter, rank=rank, world=2)
            assert not np.any(a[w == 0])          # a rank only fills its own tiles
            acc += a
            wts += w
            per_depth += np.array([int(v) for v in r.stats().rays_per_depth])
        assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)) and np.array_equal(wts, wwts)
        assert per_depth.tolist() == rays


def test_measurements_run_under_a_lens():
    scene, cam, W, H, depth, lens, _ = _frame_case("bunny")
    for jitter in (0, 1):
        r, film = _renderer(scene, cam, W, H, depth, lens, jitter)
        r.frame_index = 2
        r.ProgressiveRender(1)
        st = r.stats()
        m = r.measure_traversal(sample=2)
        assert [int(v) for v in m.rays_per_depth] == [int(v) for v in st.rays_per_depth]
        assert m.rays_traversed > 0 and m.bvh_node_visits > 0
        st2 = r.stats()
        assert st2.rays_total == st.rays_total          # a measurement counts into its own counters
        assert r.measure_shade_divergence(sample=2).sum() > 0


# ---- 4. neutral settings ------------------------------------------------------------------------------------------------------
def test_zero_lens_and_one_radian_are_the_camera_without_a_lens():
    scene, cam, W, H, depth, _, _ = _frame_case("bunny")
    frames = []
    for lens in (None, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), "set and reset"):
        if lens == "set and reset":
            r, film = _renderer(scene, cam, W, H, depth, (0.7, 0.1, 3.0))
            r.set_lens()
        else:
            r, film = _renderer(scene, cam, W, H, depth, lens)
        r.ProgressiveRender(SPP)
        r.download()
        frames.append((film.accum.copy(), film.weights.copy(), [int(v) for v in r.stats().rays_per_depth]))
    for acc, wts, rays in frames[1:]:
        assert np.array_equal(acc.view(np.uint32), frames[0][0].view(np.uint32))
        assert np.array_equal(wts, frames[0][1]) and rays == frames[0][2]
    # and that frame is the oracle's (the compact route, one walk per pixel)
    want, wwts, total = util.oracle_scene(scene).render(cam.desc(), W, H, spp=SPP, max_depth=depth, seed=SEED, iterative=True,
                                                        use_bvh=True, n_threads=8)
    assert np.array_equal(frames[0][0], want) and sum(frames[0][2]) == total


def test_field_of_view_alone_keeps_every_route():
    scene, cam, W, H, depth, _, use_bvh = _frame_case("bunny")
    r, film = _check_frames(scene, cam, W, H, depth, (0.6, 0.0, 0.0), use_bvh, 0, spps=(SPP,))
    narrow = film.accum.copy()
    # the compact route is available: switching it off changes nothing
    r2, film2 = _renderer(scene, cam, W, H, depth, (0.6, 0.0, 0.0))
    r2.set_param("compact_primary", 0)
    r2.ProgressiveRender(SPP)
    r2.download()
    assert np.array_equal(film2.accum.view(np.uint32), narrow.view(np.uint32))
    r3, film3 = _renderer(scene, cam, W, H, depth)
    r3.ProgressiveRender(SPP)
    r3.download()
    assert not np.array_equal(film3.accum, narrow)


# ---- 5. sampling upgrades and lights under a lens -----------------------------------------------------------------------------
def _lens_primary_rays(r):
    """lighting_replay.primary_rays with the renderer's own lens rays and the states after the lens draws."""
    def primary_rays(cam_desc, W, pix, rng, jitter):
        px, py, keys = lp.jittered_points(pix, W, rng, jitter)
        return r.camera_rays_lens(px, py, keys)
    return primary_rays


def test_roulette_and_clamp_under_a_lens(monkeypatch):
    scene, cam = prt.Scene("DEFAULT"), prt.Camera(width=64, height=48)
    W, H, depth, smp, n = 64, 48, 6, (1, 1, 1.0), 4
    r, film = _renderer(scene, cam, W, H, depth, (0.0, 0.2, 9.0), sampling=smp, seed=lr.SEED)
    monkeypatch.setattr(lr, "primary_rays", _lens_primary_rays(r))
    pix = np.tile(np.arange(W * H), n)
    samp = np.repeat(np.arange(n), W * H)
    _, delivered, _, segs = lr.walk(scene, orc.OracleScene(scene.desc()), cam, W, H, depth, lr.SEED, pix, samp, smp)
    want, wwts = lr.film_from_delivered(delivered, pix, samp, W, H)
    r.ProgressiveRender(n)
    r.download()
    assert np.array_equal(film.accum.view(np.uint32), want.view(np.uint32)) and np.array_equal(film.weights, wwts)
    assert r.stats().rays_total == segs
    assert film.accum.max() <= n * 1.0          # the clamp


def test_light_sampling_under_a_lens(monkeypatch):
    c = lr.case("penumbra")
    r, film = _renderer(c["scene"], c["cam"], c["W"], c["H"], c["depth"], (0.0, 0.15, 7.0), seed=lr.SEED, sif=16)
    r.set_lighting("mis")
    monkeypatch.setattr(lr, "primary_rays", _lens_primary_rays(r))
    rep = lr.replay_case(c, "mis")
    r.reset_stats()
    frames = lr.render_samples(r, film, lr.SAMPLES)
    rec = lr.check_against_gpu(rep, frames, r.light_stats(), r.light_info())
    assert rec["compared"] >= 0.995 * len(rep.pix)


def test_environment_under_a_lens(monkeypatch):
    c = er.case("DEFAULT_sun")
    film = prt.Film(c["W"], c["H"])
    r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=lr.SEED)
    r.set_environment(er.named_map(c["env"]), c["light_share"])
    r.set_lens(0.9, 0.2, 9.0)
    r.Init(film, c["scene"], c["cam"])
    r.set_samples_in_flight(16)
    r.set_lighting("mis")
    monkeypatch.setattr(lr, "primary_rays", _lens_primary_rays(r))
    rep = er.replay_case(c, "mis")
    assert r.environment_info().t_env == int(rep.t_env)
    r.reset_stats()
    frames = lr.render_samples(r, film, lr.SAMPLES)
    rec = er.check_against_gpu(rep, frames, r.light_stats())
    assert rec["compared"] >= 0.995 * len(rep.pix)


# ---- 6. the closed form on the device -----------------------------------------------------------------------------------------
def test_defocused_edge_on_the_device():
    E = lp.EDGE
    W, H, S = E["W"], E["H"], E["spp"]
    scene, cam = lp.edge_scene()
    want_hit, band = lp.edge_samples(cam)
    r, film = _renderer(scene, cam, W, H, 1, lp.edge_lens(), seed=E["seed"], sif=1)
    got_hit = np.zeros((S, H, W), bool)
    prev = np.zeros((H, W), np.float32)
    for s in range(S):
        r.ProgressiveRender(1)
        r.download()
        delta = film.accum[..., 0] - prev          # exact: the sums are small integers times the emission 1
        prev = film.accum[..., 0].copy()
        assert np.all((delta == 0.0) | (delta == np.float32(E["emission"]))), s
        got_hit[s] = delta != 0.0
    assert np.all(film.weights == np.float32(S))
    undecided = band < lp.EDGE_BAND
    share = float(undecided.mean())
    differ = got_hit != want_hit
    print(f"edge: {int(differ.sum())} samples differ from the restatement, {int(undecided.sum())} lie inside the band")
    assert share <= lr.MAX_UNSTABLE
    assert not np.any(differ & ~undecided)
    F = lp.edge_expected()
    n = S * H
    mean = film.accum[..., 0].astype(np.float64).sum(0) / n
    z = np.abs(mean - E["emission"] * F) / (E["emission"] * lp.edge_sigma(F, n))
    print(f"edge: worst column {float(z.max()):.2f} sigma")
    assert z.max() <= 5.0
    # one 256-sample call gives the same frame
    r2, film2 = _renderer(scene, cam, W, H, 1, lp.edge_lens(), seed=E["seed"], sif=8)
    r2.ProgressiveRender(S)
    r2.download()
    assert np.array_equal(film2.accum, film.accum)


# ---- 7. group and command line ------------------------------------------------------------------------------------------------
def test_group_renderer_applies_the_lens_on_every_rank():
    scene, cam, W, H, depth, lens, _ = _frame_case("bunny")
    for jitter in (0, 1):
        _, want, wwts = _bunny_frame(jitter)
        film = prt.Film(W, H)
        g = prt.HipWavefrontGroupRenderer([0, 0], max_depth=depth, seed=SEED)
        g.Init(film, scene, cam)
        g.set_lens(*lens)
        g.set_samples_in_flight(4)
        if jitter:
            g.set_sampling(jitter=1)
        g.ProgressiveRender(SPP)
        g.download()
        assert np.array_equal(film.accum.view(np.uint32), want.view(np.uint32)) and np.array_equal(film.weights, wwts)
        with pytest.raises(prt.PrtError):
            g.set_lens(aperture=0.1, focus_distance=0.0)
        del g


def test_cli_renders_the_lens_frame_of_the_python_path(tmp_path):
    exe = os.path.join(util.ROOT, "parallelraytracing_amd", "csrc", "prt_render")
    out = str(tmp_path / "frame")
    W, H = 64, 48
    p = subprocess.run([exe, "--preset", "DEFAULT", "--width", str(W), "--height", str(H), "--spp", "3", "--depth", "4", "--seed", "7",
                        "--fov-deg", "40", "--aperture", "0.2", "--focus", "9", "--out", out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    raw = open(out + ".pfm", "rb").read()
    hdr = f"PF\n{W} {H}\n-1.0\n".encode()
    assert raw.startswith(hdr)
    img = np.frombuffer(raw[len(hdr):], "<f4").reshape(H, W, 3)[::-1]
    cam = prt.Camera((5.0, 5.0, 8.0), front=(-5.0, -5.0, -8.0), width=W, height=H)     # what the command line sets
    fov = float(np.float32(40.0 * math.pi / 180.0))
    r, film = _renderer(prt.Scene("DEFAULT"), cam, W, H, 4, (fov, 0.2, 9.0), seed=7, sif=1)
    r.ProgressiveRender(3)
    r.download()
    assert np.array_equal(img, film.accum / film.weights[..., None])
    assert f"{r.stats().rays_total} rays" in p.stdout
    # and the lens arguments are checked
    p = subprocess.run([exe, "--preset", "DEFAULT", "--width", "16", "--height", "16", "--aperture", "0.2", "--out", out],
                       capture_output=True, text=True)
    assert p.returncode == 1 and "lens" in p.stderr
