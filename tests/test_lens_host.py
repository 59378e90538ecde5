"""CPU-side tests of the thin-lens camera (include/prt.h "Thin lens and field of view", prt_set_lens) on host-only contexts:
argument validation with the previous lens left in place, what the lens survives, the Python round trip, and the float64
restatement (tests/lens_replay.py) against the closed form of a defocused edge.

The closed form (lens_replay: camera at the origin looking down -z, an emitter filling x <= 0 at z = -2, focus 4, lens radius
0.25, 64 x 64 pixels, 256 samples, no jitter): per pixel column 64 rows x 256 samples = 16384 trials whose hit share must lie
within 4 sigma (binomial, floored at 1 / 16384) of F; each deliberately wrong lens must break that in some column.  Measured:
the right lens 1.3 sigma at worst over the 64 columns; "r_linear" 24.8 sigma, "focus_sphere" 7.4 sigma; 12 samples of the
1,048,576 lie within 64 * 2^-24 * zq of the edge (a share of 1.1e-5)."""
import ctypes as C
import math

import numpy as np
import pytest

import lens_replay as lp
from util import orc, prt

capi = prt.capi
NAN, INF = float("nan"), float("inf")
PI32 = float(np.float32(math.pi))                              # the fp32 nearest to pi lies above pi
BELOW_PI = float(np.nextafter(np.float32(math.pi), np.float32(0.0)))


def _host():
    return prt.HipWavefrontRenderer(device=-1)


def _lens(r):
    ln = r.get_lens()
    return (ln.fov_y, ln.aperture, ln.focus_distance)


def _f32(*v):
    return tuple(float(np.float32(x)) for x in v)


BAD = [
    ("nan fov", (NAN, 0.0, 0.0)), ("nan aperture", (0.0, NAN, 1.0)), ("nan focus, pinhole", (0.0, 0.0, NAN)),
    ("nan focus", (0.0, 0.1, NAN)),
    ("negative fov", (-0.1, 0.0, 0.0)), ("fov = pi", (PI32, 0.0, 0.0)), ("fov > pi", (4.0, 0.0, 0.0)), ("fov = inf", (INF, 0.0, 0.0)),
    ("negative aperture", (0.0, -0.1, 1.0)), ("infinite aperture", (0.0, INF, 1.0)),
    ("aperture without focus", (0.0, 0.1, 0.0)), ("aperture, negative focus", (0.0, 0.1, -2.0)),
    ("aperture, infinite focus", (0.0, 0.1, INF)),
]
GOOD = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.6, 0.0, 0.0), (BELOW_PI, 0.0, 0.0), (0.0, 0.25, 4.0), (0.9, 1e-3, 1e-3),
        (0.0, 0.0, -1.0), (0.0, 0.0, INF), (2.0, 0.0, 5.0)]


def test_a_new_context_has_the_all_zero_lens():
    assert _lens(_host()) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("what,bad", BAD, ids=[b[0] for b in BAD])
def test_invalid_lens_is_refused_and_the_previous_one_stays(what, bad):
    r = _host()
    for keep in ((0.0, 0.0, 0.0), (0.7, 0.125, 3.0)):
        r.set_lens(*keep)
        with pytest.raises(prt.PrtError):
            r.set_lens(*bad)
        assert _lens(r) == _f32(*keep), what
    # the C entry point itself: PRT_ERR_INVALID
    ln = capi.PrtLens(*bad)
    assert capi.lib().prt_set_lens(r._ctx, C.byref(ln)) == capi.lib().prt_set_lens(None, None) != 0


@pytest.mark.parametrize("good", GOOD)
def test_valid_lens_round_trips(good):
    r = _host()
    ln = r.set_lens(*good)
    assert (ln.fov_y, ln.aperture, ln.focus_distance) == _f32(*good)
    assert _lens(r) == _f32(*good)


def test_null_resets_to_zeros_and_defaults_are_zeros():
    r = _host()
    r.set_lens(0.6, 0.25, 4.0)
    assert capi.lib().prt_set_lens(r._ctx, None) == 0
    assert _lens(r) == (0.0, 0.0, 0.0)
    r.set_lens(0.6, 0.25, 4.0)
    r.set_lens()
    assert _lens(r) == (0.0, 0.0, 0.0)
    assert capi.lib().prt_get_lens(r._ctx, None) != 0


def test_lens_survives_camera_scene_and_film():
    r = _host()
    r.set_lens(0.6, 0.25, 4.0)
    want = _f32(0.6, 0.25, 4.0)
    r.SetCamera(prt.Camera((1.0, 2.0, 3.0), width=32, height=16))
    assert _lens(r) == want
    r.set_scene_host_only(prt.Scene("CORNELL"))
    assert _lens(r) == want
    assert capi.lib().prt_set_film(r._ctx, 32, 16, 0, 1) == 0
    assert _lens(r) == want
    r.SetCamera(prt.Camera((3.0, 2.0, 1.0), width=16, height=16))
    assert _lens(r) == want


def test_rays_need_a_device():
    r = _host()
    r.SetCamera(prt.Camera(width=8, height=8))
    for lens in ((0.0, 0.0, 0.0), (0.0, 0.25, 4.0)):
        r.set_lens(*lens)
        with pytest.raises(prt.PrtError):
            r.camera_rays_lens([0.5], [0.5], [1])


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_seed_restatement_is_the_oracles():
    rng = np.random.default_rng(2)
    pix = rng.integers(0, 1 << 22, 40)
    samp = rng.integers(0, 1 << 12, 40)
    for seed in (0, 3, 0xFFFFFFFF):
        got = lp.path_seeds(pix, samp, seed)
        assert [int(g) for g in got] == [orc.path_seed(int(p), int(s), seed) for p, s in zip(pix, samp)]


def test_pinhole_restatement_is_the_oracles_camera():
    cam = prt.Camera((3.0, 2.5, 6.0), front=prt.glm_normalize(np.array([-0.4, -0.3, -1.0], np.float32)), width=9, height=7)
    py, px = (a.ravel().astype(np.float32) + np.float32(0.25) for a in np.mgrid[0:7, 0:9])
    keys = np.arange(63, dtype=np.uint32)
    o, d, after = lp.lens_rays(cam, (0.0, 0.0, 0.0), px, py, keys)
    oo, od = orc.camera_rays(cam.desc(), px, py)
    assert np.array_equal(after, keys)
    assert np.array_equal(o.astype(np.float32), oo)
    assert np.abs(d - od).max() <= 4 * lp.U
    # a field of view of 1 rad is the default; a wider one spreads the directions
    assert np.array_equal(lp.lens_rays(cam, (1.0, 0.0, 0.0), px, py, keys)[1], d)
    wide = lp.lens_rays(cam, (1.4, 0.0, 0.0), px, py, keys)[1]
    f = np.asarray(cam.front, np.float64)
    assert (wide @ f).min() < (d @ f).min()


def test_lens_rays_meet_on_the_plane_in_focus():
    cam = prt.Camera((3.0, 2.5, 6.0), front=prt.glm_normalize(np.array([-0.4, -0.3, -1.0], np.float32)), width=9, height=7)
    lens = (0.8, 0.3, 5.0)
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32)
    px, py = np.full(500, 2.25, np.float32), np.full(500, 5.5, np.float32)
    o, d, after = lp.lens_rays(cam, lens, px, py, keys)
    assert np.array_equal(after, lp.pcg(lp.pcg(keys)).astype(np.uint32))
    front, right, up = (v.astype(np.float64) for v in orc.camera_basis(cam.desc()))
    pos = np.asarray(cam.position, np.float64)
    s = (5.0 - (o - pos) @ front) / (d @ front)
    P = o + s[:, None] * d
    # one point for every lens point, as far as the oracle's fp32 basis is orthonormal (each vector to a few 2^-24, times the
    # focus distance 5)
    tol = 16 * lp.U * 5.0
    assert np.abs(P - P[0]).max() < tol
    _, d0, _ = lp.lens_rays(cam, (0.8, 0.0, 0.0), px[:1], py[:1], keys[:1])
    assert np.abs(pos + (5.0 / (d0[0] @ front)) * d0[0] - P[0]).max() < tol       # the pinhole ray's point on that plane
    # the lens points fill the disk of radius 0.3 uniformly: mean r^2 = R^2 / 2
    l2 = ((o - pos) ** 2).sum(1)
    assert l2.max() <= 0.09 * (1 + tol) and abs(l2.mean() / 0.045 - 1.0) < 0.1
    assert np.abs((o - pos) @ front).max() < tol


@pytest.fixture(scope="module")
def edge():
    sc, cam = lp.edge_scene()
    return dict(cam=cam, F=lp.edge_expected(), right=lp.edge_samples(cam))


def _worst_sigma(hit, F):
    n = hit.shape[0] * hit.shape[1]
    share = hit.sum((0, 1)) / n
    return float((np.abs(share - F) / lp.edge_sigma(F, n)).max())


def test_edge_columns_follow_the_closed_form(edge):
    hit, band = edge["right"]
    F = edge["F"]
    assert F[0] == 1.0 and F[-1] == 0.0 and np.all(np.diff(F) <= 0) and ((F > 0.02) & (F < 0.98)).sum() >= 6
    z = _worst_sigma(hit, F)
    print("edge: worst column", z, "sigma; samples inside the band:", int((band < lp.EDGE_BAND).sum()))
    assert z <= 4.0
    # the band the device comparison leaves out: x at the plane has density at most 2 / (pi w), w = R (1 - zq / f) = 0.125,
    # so at most 2 * 64 * 2^-24 * zq * 2 / (pi w) = 7.8e-5 of a column's samples can fall into it: orders of magnitude
    # below the 0.005 it may take
    assert (band < lp.EDGE_BAND).mean() <= 1e-4


@pytest.mark.parametrize("wrong", lp.WRONG)
def test_edge_check_tells_a_wrong_lens_apart(edge, wrong):
    hit, _ = lp.edge_samples(edge["cam"], wrong)
    z = _worst_sigma(hit, edge["F"])
    print("edge:", wrong, "worst column", z, "sigma")
    assert z > 4.0
