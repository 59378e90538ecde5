"""The environment image on one MI355X with lighting OFF: identity with the constant sky, the device lookup against the float64
mapping, and every miss of non-constant maps against the oracle's path (tests/environment_replay.py).

160 x 120, depth 5, sample indices 0, 1, 2, 5 as one-sample frames.

Identity: a 1 x 1 map and a constant 16 x 8 map equal to `sky` must give the film and the ray counts of no environment bit for
bit, on DEFAULT, an icosahedron mesh scene and a placed-copy scene, with 1 and 16 samples in flight and with `fuse`,
`path_kernel` and `exact_grids` toggled (an environment runs the unfused route whatever they say).

Lookup: 200,000 seeded unit directions and the six axes through prt_environment_eval.  A direction is stable when its
float64 (u W, v H) lies farther than 2^-12 texel from every texel edge (environment_replay.EDGE: ROCm documents atan2f to
2 ulp and acosf to 4 ulp, which for |phi| <= pi, theta <= pi is below 1e-6 rad = 1e-5 texel at W = 64, a twentieth of the
margin); every stable direction must return the float64 texel and its exact rgb, at most 0.5 % may be left out, and the
others must still return an in-range texel.

Lighting OFF, non-constant maps: every pixel sample whose path misses at a stable direction equals the replay's fp32 term
bit for bit (the oracle gives throughput and direction exactly, the term is one fp32 product); paths that end on a surface
must equal it as well; at most 0.5 % of the samples may be left out."""
import numpy as np
import pytest

import environment_replay as er
import lighting_replay as lr
import util
from util import orc, prt

pytestmark = pytest.mark.gpu

SKY = (0.4, 0.3, 0.6)


def _scene(name):
    from parallelraytracing_amd import scenes
    if name == "DEFAULT":
        return prt.Scene("DEFAULT", sky=SKY), prt.Camera(width=er.W_, height=er.H_), False
    if name == "ico":
        def fill(sc):
            sc.AddMesh(prt.Mesh(scenes.asset("icosahedron.ply")), sc.AddLambertian((0.8, 0.7, 0.6)))
        sc, cam = lr._ground_and(fill, (1.5, 1.5, 4.5), er.W_, er.H_, sky=SKY)
        return sc, cam, True
    c = lr.case("placed", er.W_, er.H_)
    return c["scene"], c["cam"], True


def _frames(r, film, env=None, share=0.5):
    r.set_environment(env, share)
    r.reset_stats()
    frames = lr.render_samples(r, film, lr.SAMPLES)
    st = r.stats()
    return frames, (st.rays_total, tuple(st.rays_per_depth[:er.DEPTH]))


@pytest.mark.parametrize("scene", ["DEFAULT", "ico", "placed"])
def test_constant_map_equal_to_sky_is_the_sky_bit_for_bit(scene):
    sc, cam, _ = _scene(scene)
    film = prt.Film(er.W_, er.H_)
    r = prt.HipWavefrontRenderer(device=0, max_depth=er.DEPTH, seed=lr.SEED)
    r.Init(film, sc, cam)
    sky = np.asarray(sc.sky, np.float32)
    maps = [sky.reshape(1, 1, 3), np.broadcast_to(sky, (8, 16, 3)).copy()]
    base = None
    for sif in (1, 16):
        for tunables in ({}, {"fuse": 1}, {"path_kernel": 2}, {"exact_grids": 2}):
            r.set_samples_in_flight(sif)
            for k, v in tunables.items():
                r.set_param(k, v)
            ref, ref_rays = _frames(r, film, None)
            if base is None:
                base = ref
            for s in lr.SAMPLES:    # (the routes agree among themselves: the project's standing property)
                assert np.array_equal(ref[s].view(np.uint32), base[s].view(np.uint32))
            for m in maps:
                got, rays = _frames(r, film, m)
                assert rays == ref_rays
                for s in lr.SAMPLES:
                    assert np.array_equal(got[s].view(np.uint32), ref[s].view(np.uint32)), (scene, sif, tunables, m.shape, s)
            r.set_param("fuse", 0)
            r.set_param("path_kernel", 0)
            r.set_param("exact_grids", 1)


@pytest.mark.parametrize("name", er.MAPS)
def test_device_lookup_returns_the_float64_texel(name):
    env = er.EnvMap(er.named_map(name))
    r = prt.HipWavefrontRenderer(device=0)
    r.set_environment(env.rgb, 0.5)
    rng = np.random.default_rng(12)
    d = rng.normal(size=(200000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    d = np.concatenate([d, axes])
    out = r.environment_eval(d)
    i, j, edge = er.lookup64(env, d)
    stable = edge > er.EDGE
    left_out = 1.0 - stable.mean()
    print(dict(map=name, left_out=round(float(left_out), 6)), flush=True)
    assert left_out <= 0.005
    assert np.all(out["texel"] < env.W * env.H)
    assert np.array_equal(out["texel"][stable], (i * env.W + j)[stable].astype(np.uint32))
    assert np.array_equal(out["rgb"][stable].view(np.uint32), env.rgb[i, j][stable].view(np.uint32))
    # the density of the environment sample at the direction: p_ij W H / (2 pi^2 sin theta)
    pdf, sin_t = er.miss_pdf(env, d, i, j)
    ok = stable & (sin_t > 1e-3)
    np.testing.assert_allclose(out["pdf_w"][ok], pdf[ok], rtol=2e-6)
    assert np.all(out["pdf_w"][stable & (pdf == 0)] == 0)
    for n in util.WORKSPACE_COUNTS:
        part, sel = r.environment_eval(d[:n]), stable[:n]
        assert np.array_equal(part["texel"][sel], (i * env.W + j)[:n][sel].astype(np.uint32)), n
        assert np.array_equal(part["rgb"][sel].view(np.uint32), env.rgb[i, j][:n][sel].view(np.uint32)), n
        np.testing.assert_allclose(part["pdf_w"][ok[:n]], pdf[:n][ok[:n]], rtol=2e-6)


@pytest.mark.parametrize("scene,name", [("DEFAULT", "sun"), ("ico", "lognormal"), ("placed", "blackrows"), ("DEFAULT", "5x3")])
def test_lighting_off_every_stable_miss_is_the_replay_bit_for_bit(scene, name):
    sc, cam, bvh = _scene(scene)
    env = er.EnvMap(er.named_map(name))
    rep = er.replay(sc, env, cam, er.W_, er.H_, er.DEPTH, lr.SEED, lr.SAMPLES, "off", use_bvh=bvh)
    film = prt.Film(er.W_, er.H_)
    r = prt.HipWavefrontRenderer(device=0, max_depth=er.DEPTH, seed=lr.SEED)
    r.Init(film, sc, cam)
    r.set_samples_in_flight(16)
    frames, rays = _frames(r, film, env.rgb)
    assert rays[0] == rep.segments
    stable = ~rep.miss_unstable
    left_out = 1.0 - stable.mean()
    print(dict(scene=scene, map=name, misses=rep.n_misses, on_edge=rep.n_miss_edge, left_out=round(float(left_out), 6)), flush=True)
    assert rep.n_misses > 0.2 * len(rep.pix) and left_out <= 0.005
    for s in lr.SAMPLES:
        sel = (rep.samp == s) & stable
        got = frames[s].reshape(-1, 3)[rep.pix[sel]]
        assert np.array_equal(got.view(np.uint32), rep.delivered[sel].view(np.uint32)), (scene, name, s)
