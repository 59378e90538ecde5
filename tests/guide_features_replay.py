"""Restatement of the guide features through specular chains (include/prt.h "Guide features through specular chains", "The
chain") in numpy float32: every operation in the contract's order, on all live chains of a round at once.  The closest hit of
a round is a callable (the oracle's linear scan in every test), fresnelReflectance is the oracle's contract form
(oracle.fresnel_batch), and the vector helpers spell csrc/prt_device.h's reflect3, refract3, normalize3, dot3 and glm_min
operation for operation."""
import numpy as np

from util import prt
from oracle import oracle as orc

F = np.float32
KEYS = ("albedo", "normal", "position", "depth", "prim", "bounces")


def dot3(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(F)


def glm_min(x, y):
    return np.where(y < x, y, x).astype(F)


def normalize3(v):
    return (v * (F(1) / np.sqrt(dot3(v, v)))[:, None]).astype(F)


def reflect3(I, N):
    return (I - (N * dot3(N, I)[:, None]) * F(2)).astype(F)


def refract3(uv, n, eta):
    cos_theta = glm_min(dot3(-uv, n), F(1))
    perp = (eta[:, None] * (uv + cos_theta[:, None] * n)).astype(F)
    par = ((-np.sqrt(np.abs(F(1) - dot3(perp, perp))))[:, None] * n).astype(F)
    return (perp + par).astype(F)


def linear_scan(osc):
    """The closest hit of a round: the oracle's linear scan."""
    return lambda o, d: osc.closest_hit(o, d, use_bvh=False, n_threads=8)


def centre_rays(cam_desc, W, H):
    """The oracle's pinhole rays through the pixel centres (1 rad, no lens): denoise_replay.oracle_features' rays."""
    ys, xs = np.mgrid[0:H, 0:W]
    return orc.camera_rays(cam_desc, xs.ravel().astype(F) + F(0.5), ys.ravel().astype(F) + F(0.5))


def guide_features(closest_hit, scene, o, d, W, H, max_specular=0, roughness_max=0.1, albedo_of=None, trace=None):
    """The guide set of the W * H centre rays (o, d): albedo, normal, position (H, W, 3) float32, depth (H, W) float32, prim
    (H, W) int32, bounces (H, W) uint32.  albedo_of(o, d, hits) -> (n, 3): the colour prt_hit_uv reports for a round's hits
    while a binding textures a material; None: the material table.  trace: a dict that receives, per pixel, whether a
    dielectric vertex reflected ("dielectric_reflect"), whether the chain crossed a dielectric at all ("dielectric") and
    whether it ended because of the cap ("capped": a specular surface that would have been followed with a larger
    max_specular)."""
    assert 0 <= max_specular <= 8
    n = W * H
    mats = scene.materials
    mtype = np.array([m.type for m in mats], np.uint32)
    mrgb = np.array([[m.rgb[0], m.rgb[1], m.rgb[2]] for m in mats], F)
    mscalar = np.array([m.scalar for m in mats], F)
    rmax = F(roughness_max)
    out = dict(albedo=np.zeros((n, 3), F), normal=np.zeros((n, 3), F), position=np.zeros((n, 3), F), depth=np.zeros(n, F),
               prim=np.full(n, -1, np.int32), bounces=np.zeros(n, np.uint32))
    seen = dict(dielectric_reflect=np.zeros(n, bool), dielectric=np.zeros(n, bool), capped=np.zeros(n, bool))
    o, d = np.array(o, F).reshape(n, 3), np.array(d, F).reshape(n, 3)
    pixel = np.arange(n)
    T = np.ones((n, 3), F)
    L = np.zeros(n, F)
    with np.errstate(all="ignore"):
        for k in range(max_specular + 1):
            hits = closest_hit(o, d)
            is_hit = hits["prim"] >= 0
            mid = np.where(is_hit, hits["material_id"], 0).astype(np.int64)
            t, s = mtype[mid], mscalar[mid]
            rgb = mrgb[mid] if albedo_of is None else np.asarray(albedo_of(o, d, hits), F)
            N = hits["normal"].astype(F)
            seg = np.sqrt(hits["d2"].astype(F)).astype(F)
            metal = is_hit & (t == 2) & (s <= rmax)
            glass = is_hit & (t == 3)
            # Metal: material_scatter's branch without its roughness term
            r = normalize3(normalize3(reflect3(d, N)))
            ok_m = metal & (dot3(r, N) > F(0)) & np.isfinite(r).all(axis=1)
            # Dielectric: the more probable branch
            ri = np.where(hits["front_face"] != 0, F(1) / s, s).astype(F)
            cos_theta = glm_min(dot3(-d, N), F(1))
            sin_theta = np.sqrt(F(1) - cos_theta * cos_theta).astype(F)
            cannot = (ri * sin_theta).astype(F) > F(1)
            refl = cannot.copy()
            if glass.any():
                refl[glass] = cannot[glass] | (orc.fresnel_batch(cos_theta[glass], ri[glass])[0] > F(0.5))
            g = normalize3(np.where(refl[:, None], reflect3(d, N), refract3(d, N, ri)).astype(F))
            ok_g = glass & np.isfinite(g).all(axis=1)
            would = ok_m | ok_g
            follow = would & (k < max_specular)
            # terminal chains: the records of their pixel
            end = ~follow
            p = pixel[end]
            hit_e = is_hit[end]
            coloured = (t[end] == 1) | (t[end] == 2)
            a = np.where(coloured[:, None], rgb[end], F(1)).astype(F)
            out["albedo"][p] = np.where(hit_e[:, None], (T[end] * a).astype(F), T[end])
            out["normal"][p] = np.where(hit_e[:, None], N[end], F(0))
            out["position"][p] = np.where(hit_e[:, None], hits["position"][end], F(0))
            out["depth"][p] = np.where(hit_e, (L[end] + seg[end]).astype(F), F(0))
            out["prim"][p] = np.where(hit_e, hits["prim"][end], -1)
            out["bounces"][p] = k
            seen["capped"][p] = would[end]
            # the others move on
            pf = pixel[follow]
            seen["dielectric"][pf] |= ok_g[follow]
            seen["dielectric_reflect"][pf] |= (ok_g & refl)[follow]
            T = np.where(ok_m[follow][:, None], (T[follow] * rgb[follow]).astype(F), T[follow]).astype(F)
            L = (L[follow] + seg[follow]).astype(F)
            o = hits["position"][follow].astype(F)
            d = np.where(ok_m[follow][:, None], r[follow], g[follow]).astype(F)
            pixel = pf
            if pixel.size == 0:
                break
    assert pixel.size == 0
    if trace is not None:
        trace.update({key: v.reshape(H, W) for key, v in seen.items()})
    return dict(albedo=out["albedo"].reshape(H, W, 3), normal=out["normal"].reshape(H, W, 3), position=out["position"].reshape(H, W, 3),
                depth=out["depth"].reshape(H, W), prim=out["prim"].reshape(H, W), bounces=out["bounces"].reshape(H, W))


def mirror_room(pane=False):
    """MIRROR_ROOM: a grey ground under a row of lights, a wall mirror, a mirror ball, a glass ball and a red ball.  pane (the
    GPU tests' scene, not the quality fixture): also a glass quad just above the ground that faces down, so that the camera
    sees its back at more than the critical angle: dielectric vertices that reflect."""
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.6, 0.6, 0.6))
    light = sc.AddEmissive((4.0, 4.0, 4.0))
    mirror = sc.AddMetal((0.9, 0.9, 0.9), 0.0)
    glass = sc.AddDielectric(1.5)
    red = sc.AddLambertian((0.8, 0.2, 0.2))
    sc.AddQuad(30.0, 30.0, ground)
    for i in range(-5, 6):
        sc.AddCircle(0.5, light, translation=(2.0 * i, 6.0, 0.0))
    sc.AddQuad(14.0, 6.0, mirror, euler_deg=(90.0, 0.0, 0.0), translation=(0.0, 3.0, -4.0))
    sc.AddCircle(1.0, mirror, translation=(-2.0, 1.0, 1.0))
    sc.AddCircle(1.0, glass, translation=(2.0, 1.0, 2.0))
    sc.AddCircle(0.7, red, translation=(0.5, 0.7, -1.5))
    if pane:
        sc.AddQuad(3.0, 2.0, glass, euler_deg=(180.0, 0.0, 0.0), translation=(3.0, 0.4, 3.5))
    return sc
