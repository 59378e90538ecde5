"""Float64 restatement of the thin-lens camera (include/prt.h "Thin lens and field of view"), written from the header text
alone, and the closed form of a defocused edge.

  * lens_rays: origin and direction of the primary ray through a pixel-space point for an RNG state, and the state after
    the lens draws.  The basis is the oracle's (orc.camera_basis), the draws are lighting_replay's pcg / rnd.
  * `wrong=` selects a deliberately wrong lens (WRONG), used only to show that the closed-form check tells it apart:
      "r_linear"      r = aperture * u3 (not uniform over the disk)
      "focus_sphere"  the focus point at distance `focus` ALONG the pinhole ray, not on the plane perpendicular to `front`
  * the edge case: camera at the origin looking down -z, sky 0, one emitter filling x <= 0 in the plane z = -zq.  A ray of
    pixel column a = pcx from the lens point (lx, ly) meets that plane at x = a zq + lx (1 - zq / f), so the column's
    expected value is E F(t), t = clip(-a zq / (R (1 - zq / f)), -1, 1), F(t) = 1/2 + (t sqrt(1 - t^2) + asin t) / pi:
    the share of the unit disk with abscissa <= t.

No kernel code and no GPU is involved."""
from __future__ import annotations

import math

import numpy as np

from lighting_replay import M32, pcg, rnd
from util import orc, prt

WRONG = ("r_linear", "focus_sphere")
TWO_PI_F32 = float(np.float32(6.2831855))
U = 2.0 ** -24


def path_seeds(pixel, sample, seed):
    """path_seed(pixel, sample, seed) = pcg((pixel ^ (sample * 719393)) + seed * 0x9E3779B9), vectorised (uint32)."""
    pixel = np.asarray(pixel).astype(np.uint64)
    sample = np.asarray(sample).astype(np.uint64)
    v = ((pixel ^ ((sample * 719393) & M32)) + ((int(seed) * 0x9E3779B9) & M32)) & M32
    return pcg(v).astype(np.uint32)


def tan_fov_y(fov_y):
    f = float(np.float32(fov_y))
    return math.tan(0.5) if f == 0.0 else math.tan(0.5 * f)


def _normalize(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def lens_rays(cam, lens, px, py, keys, wrong=None):
    """cam: prt.Camera; lens: (fov_y, aperture, focus_distance); px, py: pixel-space points (taken as fp32); keys: the paths'
    RNG states before the lens draws.  -> (origins [n, 3], dirs [n, 3]) in float64 and the states afterwards (uint32): two
    draws further while aperture > 0, untouched otherwise."""
    assert wrong is None or wrong in WRONG, wrong
    fov, ap, focus = (float(np.float32(v)) for v in lens)
    front, right, up = (v.astype(np.float64) for v in orc.camera_basis(cam.desc()))
    pos = np.asarray(cam.position, np.float32).astype(np.float64)
    W, H = float(np.float32(cam.width)), float(np.float32(cam.height))
    px = np.asarray(px, np.float32).astype(np.float64).ravel()
    py = np.asarray(py, np.float32).astype(np.float64).ravel()
    keys = np.asarray(keys).astype(np.uint32).ravel()
    t = tan_fov_y(fov)
    ndcx = (px / W) * 2.0 - 1.0
    ndcy = 1.0 - (py / H) * 2.0
    aspect = W / H
    pcx = ndcx * aspect * t
    pcy = ndcy * t
    if ap == 0.0:
        dc = _normalize(np.stack([pcx, pcy, -np.ones_like(pcx)], 1))
        d = _normalize(dc[:, 0:1] * right + dc[:, 1:2] * up + dc[:, 2:3] * -front)
        return np.broadcast_to(pos, d.shape).copy(), d, keys.copy()
    u3, s = rnd(keys)
    u4, s = rnd(s)
    r = ap * (u3 if wrong == "r_linear" else np.sqrt(u3))
    phi = TWO_PI_F32 * u4
    lx = r * np.cos(phi)
    ly = r * np.sin(phi)
    if wrong == "focus_sphere":
        P = focus * _normalize(np.stack([pcx, pcy, -np.ones_like(pcx)], 1))
    else:
        P = np.stack([pcx * focus, pcy * focus, np.full_like(pcx, -focus)], 1)
    dc = _normalize(P - np.stack([lx, ly, np.zeros_like(lx)], 1))
    d = _normalize(dc[:, 0:1] * right + dc[:, 1:2] * up + dc[:, 2:3] * -front)
    o = pos + lx[:, None] * right + ly[:, None] * up
    return o, d, s.astype(np.uint32)


def jittered_points(pix, W, keys, jitter):
    """Pixel-space points of pixel indices `pix` as the render forms them in fp32: centres, or (x + u1, y + u2) with the
    path's first two draws.  -> (px, py) float32 and the states afterwards."""
    x = (np.asarray(pix) % W).astype(np.float32)
    y = (np.asarray(pix) // W).astype(np.float32)
    keys = np.asarray(keys).astype(np.uint32)
    if not jitter:
        return x + np.float32(0.5), y + np.float32(0.5), keys
    u1, keys = rnd(keys)
    u2, keys = rnd(keys)
    return (x + u1.astype(np.float32)).astype(np.float32), (y + u2.astype(np.float32)).astype(np.float32), keys


# ---- the defocused edge -----------------------------------------------------------------------------------------------------
EDGE = dict(W=64, H=64, focus=4.0, zq=2.0, aperture=0.25, spp=256, seed=3, emission=1.0)
EDGE_BAND = 64.0 * U      # x relative to zq: closer to the edge than this, hit or miss is not decidable from outside


def edge_scene():
    """Sky 0 and one emissive triangle in the plane z = -zq whose edge x = 0 runs from y = -8 to y = 8; the other two edges
    are far outside the view (and the lens)."""
    zq, E = EDGE["zq"], EDGE["emission"]
    sc = prt.Scene(preset=None, sky=(0.0, 0.0, 0.0))
    e = sc.AddEmissive((E, E, E))
    v = np.array([[0.0, -8.0, -zq], [0.0, 8.0, -zq], [-16.0, 0.0, -zq]], np.float32)   # faces +z, the camera's side
    sc.AddMesh(prt.Mesh(vertices=v, indices=np.array([[0, 1, 2]], np.uint32)), e)
    cam = prt.Camera((0.0, 0.0, 0.0), front=(0.0, 0.0, -1.0), width=EDGE["W"], height=EDGE["H"])
    return sc, cam


def edge_lens():
    return (0.0, EDGE["aperture"], EDGE["focus"])


def edge_F(t):
    t = np.clip(t, -1.0, 1.0)
    return 0.5 + (t * np.sqrt(1.0 - t * t) + np.arcsin(t)) / np.pi


def edge_expected():
    """F per pixel column (no jitter: every sample of a column goes through the column's pixel centres)."""
    W, H, R, f, zq = EDGE["W"], EDGE["H"], EDGE["aperture"], EDGE["focus"], EDGE["zq"]
    a = (((np.arange(W) + 0.5) / W) * 2.0 - 1.0) * (W / H) * tan_fov_y(0.0)
    return edge_F(-a * zq / (R * (1.0 - zq / f)))


def edge_samples(cam, wrong=None):
    """The restatement's decision for every sample of the edge frame: (hit [spp, H, W] bool, |x| / zq at the plane
    [spp, H, W])."""
    W, H, S, seed, zq = EDGE["W"], EDGE["H"], EDGE["spp"], EDGE["seed"], EDGE["zq"]
    pix = np.tile(np.arange(W * H), S)
    samp = np.repeat(np.arange(S), W * H)
    keys = path_seeds(pix, samp, seed)
    px, py, keys = jittered_points(pix, W, keys, 0)
    o, d, _ = lens_rays(cam, edge_lens(), px, py, keys, wrong)
    s = (-zq - o[:, 2]) / d[:, 2]
    x = o[:, 0] + s * d[:, 0]
    return (x <= 0.0).reshape(S, H, W), (np.abs(x) / zq).reshape(S, H, W)


def edge_sigma(F, n):
    return np.maximum(np.sqrt(F * (1.0 - F) / n), 1.0 / n)
