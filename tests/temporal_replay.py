"""Restatement of the temporal reprojection (include/prt.h "Temporal reprojection") in numpy: every line in float32,
operation for operation in the contract's order, the one variance line in float64 rounded once.  All pixels are evaluated at
once; within a pixel the four taps are visited in the contract's order and each running sum receives its terms in that order.

Rules the header leaves to "the same words": a dot product a . b is (a.x b.x + a.y b.y) + a.z b.z; transform_point(M, p)
component r = (M[r] p.x + M[4 + r] p.y) + (M[8 + r] p.z + M[12 + r] * 1) on the column-major 4 x 4; lin(M, n) component r =
(M[r] n.x + M[4 + r] n.y) + M[8 + r] n.z; normalize3(v) = v * (1 / sqrt(v . v)); the bilinear weight is bx * by with bx =
1 - tx at ix and tx at ix + 1 (the x factor first).

Subnormals are outside what "bit for bit" covers: the replay watches every intermediate of the pixels that evaluate it and,
with guard=True, refuses a fixture in which a non-zero one lies below 2^-120 in magnitude."""
import numpy as np

import denoise_replay as dr
from denoise_replay import Watch

F = np.float32
SB_MIN = F(2.0 ** -6)
DEFAULTS = dict(max_history=32.0, normal_min=0.9, plane_tol=0.01)
HIST_KEYS = ("hc", "hn", "h1", "h2", "hP", "hN", "hprim")


def _dot(a, b, T, where):
    return T(T(T(a[..., 0] * b[..., 0], where) + T(a[..., 1] * b[..., 1], where), where) + T(a[..., 2] * b[..., 2], where), where)


def basis(position, front, W, H, fov_y=0.0):
    """What prt_set_camera / prt_set_lens give the kernels: front normalised, right = normalize(front x (0, 1, 0)), up =
    normalize(right x front), tan_fov_y = tanf(0.5 fov_y) (1 rad when fov_y = 0), through the oracle's own basis."""
    from util import orc, prt  # (util puts the repository root on sys.path)
    import lens_replay as lr
    cam = prt.Camera(position=position, front=front, width=W, height=H)
    f, r, u = orc.camera_basis(cam.desc())
    return dict(pos=np.asarray(position, F), right=r.astype(F), up=u.astype(F), front=f.astype(F), W=F(W), H=F(H),
                tan_fov_y=F(lr.tan_fov_y(fov_y)))


def transform_point(M, p):
    M = np.asarray(M, F)
    return np.stack([((M[r] * p[..., 0]).astype(F) + (M[4 + r] * p[..., 1]).astype(F)).astype(F)
                     + ((M[8 + r] * p[..., 2]).astype(F) + (M[12 + r] * F(1))).astype(F) for r in range(3)], axis=-1).astype(F)


def lin(M, n):
    M = np.asarray(M, F)
    return np.stack([(((M[r] * n[..., 0]).astype(F) + (M[4 + r] * n[..., 1]).astype(F)).astype(F) + (M[8 + r] * n[..., 2]).astype(F))
                     for r in range(3)], axis=-1).astype(F)


def normalize3(v):
    with np.errstate(all="ignore"):
        d = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]).astype(F) + v[..., 2] * v[..., 2]).astype(F)
        s = (F(1) / np.sqrt(d).astype(F)).astype(F)
    return (v * s[..., None]).astype(F)


def prev_surface(position, normal, prim, prim_base, n_tris, inv_cur, mat_prev):
    """The previous-surface rule: placed copy k owns the prims [prim_base[k], prim_base[k] + n_tris[k]); inv_cur[k] / mat_prev[k]
    are its current inverse and its previous matrix, 16 floats column-major.  No copies: the inputs."""
    P, N = np.array(position, F), np.array(normal, F)
    prim = np.asarray(prim)
    for k in range(len(prim_base)):
        m = (prim >= int(prim_base[k])) & (prim < int(prim_base[k]) + int(n_tris[k]))
        if m.any():
            P[m] = transform_point(mat_prev[k], transform_point(inv_cur[k], P[m]))
            N[m] = normalize3(lin(mat_prev[k], lin(inv_cur[k], N[m])))
    return P, N


def frame_inputs(accum, weights, A, Q):
    """prt_film_temporal's c and n from the film: c = rgb_sum / weight per channel in float32, 0 where the weight is 0."""
    mean, _ = dr.film_inputs(accum, weights, A, Q)
    return mean, np.asarray(weights, F)


def reproject(K, c, n, A, Q, prim, Pprev, Nprev, history=None, max_history=32.0, normal_min=0.9, plane_tol=0.01, guard=True, info=None,
              variant=None):
    """The contract.  K: the previous basis (basis()'s dict); history: None or a dict of HIST_KEYS.  Returns a dict of c, n,
    m1, m2, var, status (uint8) and, for the tests, kind: 0 no history asked (miss / none at all), 1 status 1, 2 behind the
    previous camera, 3 projected off-screen, 4 the taps were rejected.  variant (the deliberately wrong filters the tests
    tell apart): "no_plane", "no_normal", "nearest"."""
    T = Watch()
    c, n, A, Q = np.array(c, F), np.array(n, F), np.asarray(A, F), np.asarray(Q, F)
    prim = np.asarray(prim)
    P, N = np.asarray(Pprev, F), np.asarray(Nprev, F)
    H, W = n.shape
    assert c.shape == P.shape == N.shape == (H, W, 3) and prim.shape == A.shape == Q.shape == (H, W)
    assert float(K["W"]) == W and float(K["H"]) == H
    maxh, nmin, ptol = F(max_history), F(normal_min), F(plane_tol)
    with np.errstate(all="ignore"):
        pos_n = n > 0
        m1 = np.where(pos_n, T(A / n, pos_n), F(0)).astype(F)
        m2 = np.where(pos_n, T(Q / n, pos_n), F(0)).astype(F)
        var0 = dr.film_inputs(np.zeros((H, W, 3), F), n, A, Q)[1]
        out = dict(c=c.copy(), n=n.copy(), m1=m1.copy(), m2=m2.copy(), var=var0.copy(), status=np.zeros((H, W), np.uint8),
                   kind=np.zeros((H, W), np.uint8))
        if history is None:
            return _done(out, T, guard, info)
        h = {k: np.asarray(history[k], np.int32 if k == "hprim" else F) for k in HIST_KEYS}
        want = prim >= 0
        Kp, Kr, Ku, Kf = (np.asarray(K[k], F) for k in ("pos", "right", "up", "front"))
        KW, KH, tan = F(K["W"]), F(K["H"]), F(K["tan_fov_y"])
        v = T(P - Kp, want)
        bc = lambda a: np.broadcast_to(a, v.shape)  # noqa: E731
        z = _dot(v, bc(Kf), T, want)
        front_ok = want & (z > 0)
        x = _dot(v, bc(Kr), T, front_ok)
        y = _dot(v, bc(Ku), T, front_ok)
        aspect = F(KW / KH)
        ndcX = T(T(x / z, front_ok) / F(aspect * tan), front_ok)
        ndcY = T(T(y / z, front_ok) / tan, front_ok)
        fx = T(T(T(T(ndcX + F(1), front_ok) * F(0.5), front_ok) * KW, front_ok) - F(0.5), front_ok)
        fy = T(T(T(T(F(1) - ndcY, front_ok) * F(0.5), front_ok) * KH, front_ok) - F(0.5), front_ok)
        vv = _dot(v, v, T, front_ok)
        inside = front_ok & (fx > -1) & (fx < KW) & (fy > -1) & (fy < KH)
        out["kind"][want & ~front_ok] = 2
        out["kind"][front_ok & ~inside] = 3
        fxs, fys = np.where(inside, fx, F(0)).astype(F), np.where(inside, fy, F(0)).astype(F)
        flx, fly = np.floor(fxs).astype(F), np.floor(fys).astype(F)
        tx, ty = T(fxs - flx, inside), T(fys - fly, inside)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        lim = T(ptol * T(np.sqrt(vv).astype(F), inside), inside)
        Sb = np.zeros((H, W), F)
        Sc = np.zeros((H, W, 3), F)
        Sn, S1, S2 = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
        near = (np.where(tx >= F(0.5), 1, 0) + 2 * np.where(ty >= F(0.5), 1, 0))
        for t in range(4):
            xx, yy = ix + (t & 1), iy + (t >> 1)
            inimg = inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            xc, yc = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1)
            hn, hpr, hN, hP = h["hn"][yc, xc], h["hprim"][yc, xc], h["hN"][yc, xc], h["hP"][yc, xc]
            ok = inimg & (hn > 0) & (hpr >= 0)
            nd = _dot(N, hN, T, ok)
            if variant != "no_normal":
                ok = ok & (nd >= nmin)
            D = T(hP - P, ok)
            pd = np.abs(_dot(D, N, T, ok))
            if variant != "no_plane":
                ok = ok & (pd <= lim)
            bx = T(F(1) - tx, ok) if (t & 1) == 0 else tx
            by = T(F(1) - ty, ok) if (t >> 1) == 0 else ty
            b = T(bx * by, ok)
            if variant == "nearest":
                b = np.where(near == t, F(1), F(0)).astype(F)
            Sb = np.where(ok, T(Sb + b, ok), Sb).astype(F)
            Sc = np.where(ok[..., None], T(Sc + T(b[..., None] * h["hc"][yc, xc], ok), ok), Sc).astype(F)
            Sn = np.where(ok, T(Sn + T(b * hn, ok), ok), Sn).astype(F)
            S1 = np.where(ok, T(S1 + T(b * h["h1"][yc, xc], ok), ok), S1).astype(F)
            S2 = np.where(ok, T(S2 + T(b * h["h2"][yc, xc], ok), ok), S2).astype(F)
        st = inside & ~(Sb < SB_MIN)
        out["kind"][inside & ~st] = 4
        out["kind"][st] = 1
        hc, Nh, H1, H2 = T(Sc / Sb[..., None], st), T(Sn / Sb, st), T(S1 / Sb, st), T(S2 / Sb, st)
        N1 = np.minimum(T(Nh + n, st), maxh).astype(F)
        a = np.minimum(T(n / N1, st), F(1)).astype(F)
        cb = T(hc + T(a[..., None] * T(c - hc, st), st), st)
        m1b = T(H1 + T(a * T(m1 - H1, st), st), st)
        m2b = T(H2 + T(a * T(m2 - H2, st), st), st)
        m1d, m2d = m1b.astype(np.float64), m2b.astype(np.float64)
        V = np.maximum(0.0, m2d - m1d * m1d)
        varb = T((V / np.maximum(N1.astype(np.float64) - 1.0, 1.0)).astype(F), st)
        out["c"][st], out["n"][st], out["m1"][st], out["m2"][st], out["var"][st] = cb[st], N1[st], m1b[st], m2b[st], varb[st]
        out["status"][st] = 1
    return _done(out, T, guard, info)


def _done(out, T, guard, info):
    if info is not None:
        info["smallest"] = T.smallest
        info["below_guard"] = T.below_guard
    if guard:
        assert T.below_guard == 0, f"{T.below_guard} non-zero intermediates below 2^-120 (smallest {T.smallest:.3e}): not a fixture"
    return out


def next_history(out, position, normal, prim):
    """The history a step leaves: its blended outputs and the frame's own surface."""
    return dict(hc=out["c"], hn=out["n"], h1=out["m1"], h2=out["m2"], hP=np.asarray(position, F), hN=np.asarray(normal, F),
                hprim=np.asarray(prim, np.int32))


# ---- fixtures -------------------------------------------------------------------------------------------------------------
def pinhole_points(K, depth_fn):
    """Per pixel of K's image: the point at which the ray through the pixel centre meets a surface at distance-along-front
    depth_fn(xs, ys) (float64 geometry, rounded once: a fixture, not a contract)."""
    W, H = int(K["W"]), int(K["H"])
    ys, xs = np.mgrid[0:H, 0:W]
    ndcX = (xs + 0.5) / W * 2 - 1
    ndcY = 1 - (ys + 0.5) / H * 2
    t = float(K["tan_fov_y"])
    z = np.broadcast_to(np.asarray(depth_fn(xs, ys), np.float64), xs.shape)
    pc = np.stack([ndcX * (W / H) * t * z, ndcY * t * z, z], axis=-1)
    R = np.stack([np.asarray(K[k], np.float64) for k in ("right", "up", "front")])
    return (np.asarray(K["pos"], np.float64) + pc @ R).astype(F)


def two_planes(W=44, H=28, shift=0.35, seed=7, prev=None, fov_y=0.0, hn_value=None):
    """The disocclusion fixture.  Previous frame: camera at the origin looking down -z at a back wall z = -6 (prim 0, normal
    +z) with a front plane z = -3 (prim 1) over the middle of the image.  Current frame: the camera moved right by `shift` and
    turned, so that part of the wall it sees projects off the previous screen, and the front plane moved right, so that the
    wall behind its old place is newly revealed.  A band of misses on top; a patch at the lower left whose points are placed
    behind the previous camera by hand (prim 2, a surface of its own); a corner of the history that was a miss (hn = 0);
    a side wall x = -2.4 (prim 3) that meets the back wall in a corner, where only the normals tell the two apart.
    Returns (K_prev, current frame dict, history dict)."""
    rng = np.random.default_rng(seed)
    Kp = basis((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), W, H, fov_y) if prev is None else prev
    Kc = basis((shift, 0.05, 0.1), (0.12, 0.0, -1.0), W, H)
    ys, xs = np.mgrid[0:H, 0:W]

    def frame(K, front_lo, front_hi):
        wall = pinhole_points(K, lambda x, y: 1.0)  # unit depth: scaled onto the planes below
        o = np.asarray(K["pos"], np.float64)
        d = wall.astype(np.float64) - o
        tb = (-6.0 - o[2]) / d[..., 2]
        tf = (-3.0 - o[2]) / d[..., 2]
        Pb, Pf = o + d * tb[..., None], o + d * tf[..., None]
        on_front = (Pf[..., 0] > front_lo) & (Pf[..., 0] < front_hi) & (np.abs(Pf[..., 1]) < 1.0)
        with np.errstate(all="ignore"):
            ts = (-2.4 - o[0]) / d[..., 0]
            Ps = o + d * ts[..., None]
        on_side = ~on_front & (Pb[..., 0] < -2.4)            # the side wall x = -2.4 (prim 3, normal +x) meets the back wall
        P = np.where(on_front[..., None], Pf, np.where(on_side[..., None], Ps, Pb)).astype(F)
        prim = np.where(on_front, 1, np.where(on_side, 3, 0)).astype(np.int32)
        N = np.zeros((H, W, 3), F)
        N[..., 2] = 1
        N[on_side] = (1, 0, 0)
        return P, N, prim
    hP, hN, hprim = frame(Kp, -0.8, 0.6)
    P, N, prim = frame(Kc, -0.2, 1.2)
    band = 3 if H >= 12 else H // 4                           # (a single row has neither band)
    miss = ys < band
    P[miss], N[miss], prim[miss] = 0, 0, -1
    behind = (ys >= H - band) & (xs < 6)
    P[behind] = np.stack([xs[behind] * 0.1, np.full(behind.sum(), -1.0), np.full(behind.sum(), 2.0)], axis=-1).astype(F)
    N[behind], prim[behind] = (0, 1, 0), 2
    hmiss = (ys < 2) & (xs > W - 8)
    hP[hmiss], hN[hmiss], hprim[hmiss] = 0, 0, -1
    n = np.full((H, W), F(2))
    y1 = rng.uniform(0.1, 2.0, (H, W))
    y2 = rng.uniform(0.1, 2.0, (H, W))
    cur = dict(c=rng.uniform(0.0, 2.0, (H, W, 3)).astype(F), n=n, A=(y1 + y2).astype(F), Q=(y1 * y1 + y2 * y2).astype(F), prim=prim, Pprev=P,
               Nprev=N)
    hn = rng.integers(1, 9, (H, W)).astype(F) if hn_value is None else np.full((H, W), F(hn_value))
    hm = rng.uniform(0.1, 2.0, (H, W))
    hist = dict(hc=rng.uniform(0.0, 2.0, (H, W, 3)).astype(F), hn=hn, h1=hm.astype(F), h2=(hm * hm + rng.uniform(0.0, 0.5, (H, W))).astype(F),
                hP=hP, hN=hN, hprim=hprim)
    hist["hn"][hmiss] = 0
    return Kp, cur, hist


# The fixtures the GPU is compared on bit for bit (tests/test_gpu_temporal.py): name, W, H, two_planes' arguments, the
# settings.  tests/test_temporal_replay.py holds the guard on every one of them.
GPU_FIXTURES = [
    ("37x29", 37, 29, {}, {}),
    ("37x29 other fov_y", 37, 29, dict(fov_y=0.7), {}),
    ("37x29 zero-length history", 37, 29, dict(hn_value=0.0), {}),
    ("37x29 max_history 1", 37, 29, {}, dict(max_history=1.0)),
    ("37x29 max_history 1000", 37, 29, dict(hn_value=900.0), dict(max_history=1000.0)),
    ("37x29 loose tests", 37, 29, {}, dict(normal_min=-1.0, plane_tol=0.05)),
    ("70x5", 70, 5, {}, {}),
    ("70x5 other fov_y", 70, 5, dict(fov_y=1.4), {}),
    ("1x1", 1, 1, {}, {}),
    ("130x67", 130, 67, {}, {}),
    ("130x67 other fov_y, max_history 4", 130, 67, dict(fov_y=0.7), dict(max_history=4.0)),
]
