"""Restatement of the film denoiser (include/prt.h "First-hit feature images and the edge-avoiding film denoiser") in numpy:
the filter in float32, operation for operation in the contract's order, and the variance of the mean luminance in float64,
rounded once.  Every pixel of an iteration is evaluated at once on shifted views, which changes no operation and no order
within a pixel: the taps are visited row-major, and each running sum receives its terms in that order.

Subnormals are outside what "bit for bit" covers, so the replay watches every intermediate the contract evaluates and, with
guard=True, refuses a fixture in which a non-zero one lies below 2^-120 in magnitude."""
import numpy as np

F = np.float32
KR, KG, KB = F(0.2126), F(0.7152), F(0.0722)
K5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))
K3 = (F(1 / 4), F(1 / 2), F(1 / 4))
RHO_MIN, EPS_L, TINY, W_MIN = F(2.0 ** -6), F(2.0 ** -20), F(2.0 ** -100), F(2.0 ** -30)
GUARD = 2.0 ** -120
DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_z=0.1, normal_power_log2=6, demodulate=1)


class Watch:
    """Passes float32 arrays through and remembers the smallest non-zero finite magnitude it saw."""

    def __init__(self):
        self.smallest = np.inf
        self.below_guard = 0

    def __call__(self, a, where=None):
        assert a.dtype == F, a.dtype
        v = a if where is None else a[where]
        m = np.abs(v[np.isfinite(v)])
        m = m[m > 0]
        if m.size:
            self.smallest = min(self.smallest, float(m.min()))
            self.below_guard += int((m < GUARD).sum())
        return a


def _lum(c, T):
    return T(T(T(KR * c[..., 0]) + T(KG * c[..., 1])) + T(KB * c[..., 2]))


def _dot(a, b, T, where):
    return T(T(T(a[..., 0] * b[..., 0], where) + T(a[..., 1] * b[..., 1], where), where) + T(a[..., 2] * b[..., 2], where), where)


def _views(H, W, oy, ox):
    """(slices of p, slices of q = p + (oy, ox)) over the pixels p whose tap lies in the image; None if there is none."""
    y0, y1 = max(0, -oy), min(H, H - oy)
    x0, x1 = max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def film_inputs(accum, weights, A, Q):
    """prt_film_denoise's inputs from the film and its moments: mean = rgb_sum / weight per channel in float32, and
    var in float64 rounded once: m = A / n, V = max(0, Q / n - m m), var = V / (n - 1); fl(m) * fl(m) where 0 < n < 2;
    mean and var 0 where n = 0."""
    n = np.asarray(weights, F)
    acc = np.asarray(accum, F)
    with np.errstate(all="ignore"):
        mean = np.where(n[..., None] > 0, acc / n[..., None], F(0)).astype(F)
        n64 = n.astype(np.float64)
        m = np.asarray(A, F).astype(np.float64) / n64
        V = np.maximum(0.0, np.asarray(Q, F).astype(np.float64) / n64 - m * m)
        var = (V / (n64 - 1.0)).astype(F)
        mf = m.astype(F)
        var = np.where(n < F(2), (mf * mf).astype(F), var)
        var = np.where(n > 0, var, F(0)).astype(F)
    return mean, var


def denoise(mean, var, albedo, normal, position, prim, iterations=5, sigma_l=4.0, sigma_z=0.1, normal_power_log2=6,
            demodulate=1, guard=True, info=None):
    """(out (H, W, 3), var_out (H, W)) of the contract.  info: a dict that receives the smallest intermediate seen."""
    T = Watch()
    c = np.array(mean, F)
    v = np.array(var, F)
    alb, N, P = np.asarray(albedo, F), np.asarray(normal, F), np.asarray(position, F)
    hit = np.asarray(prim) >= 0
    H, W = v.shape
    assert c.shape == (H, W, 3) and alb.shape == N.shape == P.shape == (H, W, 3) and hit.shape == (H, W)
    assert 0 <= iterations <= 6 and 0 <= normal_power_log2 <= 8
    sl, sz = F(sigma_l), F(sigma_z)
    with np.errstate(all="ignore"):
        if demodulate:
            rho = np.where(hit[..., None], np.maximum(alb, RHO_MIN), F(1)).astype(F)
            lr = _lum(rho, T)
            lr2 = T(lr * lr)
            c = T(c / rho)
            v = T(v / lr2)
        for i in range(iterations):
            s = 1 << i
            num = np.zeros((H, W), F)
            ks = np.zeros((H, W), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    pq = _views(H, W, dy, dx)
                    if pq is None:
                        continue
                    p, q = pq
                    k = F(K3[dy + 1] * K3[dx + 1])
                    num[p] = T(num[p] + T(k * v[q]))
                    ks[p] = ks[p] + k
            g = T(num / ks)
            den = T(T(sl * T(np.sqrt(g))) + EPS_L)
            lm = _lum(c, T)
            Sw = np.zeros((H, W), F)
            Sc = np.zeros((H, W, 3), F)
            Sv = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    pq = _views(H, W, dy * s, dx * s)
                    if pq is None:
                        continue
                    p, q = pq
                    h = F(K5[dy + 2] * K5[dx + 2])
                    cq, vq = c[q], v[q]
                    if dy == 0 and dx == 0:
                        w = np.full(vq.shape, h, F)
                    else:
                        hp, hq = hit[p], hit[q]
                        both = hp & hq
                        same = hp == hq
                        Np, Nq = N[p], N[q]
                        wn = np.maximum(F(0), _dot(Np, Nq, T, both)).astype(F)
                        for _ in range(normal_power_log2):
                            wn = T(wn * wn, both)
                        D = T(P[q] - P[p], both)
                        dn = _dot(D, Np, T, both)
                        dd = _dot(D, D, T, both)
                        xz = T(np.abs(dn) / T(T(sz * T(np.sqrt(dd), both), both) + TINY, both), both)
                        wn = np.where(both, wn, F(1)).astype(F)
                        xz = np.where(both, xz, F(0)).astype(F)
                        xl = T(np.abs(T(lm[p] - lm[q], same)) / den[p], same)
                        x = T(xl + xz, same)
                        w = T(T(h * wn, same) / T(T(F(1) + x, same) + T(T(F(0.5) * x, same) * x, same), same), same)
                        w = np.where(w < W_MIN, F(0), w).astype(F)
                        w = np.where(same, w, F(0)).astype(F)
                    Sw[p] = T(Sw[p] + w)
                    Sc[p] = T(Sc[p] + T(w[..., None] * cq))
                    Sv[p] = T(Sv[p] + T(T(w * w) * vq))
            c = T(Sc / Sw[..., None])
            v = T(Sv / T(Sw * Sw))
        if demodulate:
            c = T(c * rho)
            v = T(v * lr2)
    if info is not None:
        info["smallest"] = T.smallest
        info["below_guard"] = T.below_guard
    if guard:
        assert T.below_guard == 0, f"{T.below_guard} non-zero intermediates below 2^-120 (smallest {T.smallest:.3e}): not a fixture"
    return c, v


def oracle_features(osc, scene, cam_desc, W, H):
    """The feature images from the oracle's linear-scan closest hit of the pixel-centre rays (the oracle's own pinhole
    camera: 1 rad, no lens).  scene: the prt.Scene the OracleScene was built from (untextured)."""
    from oracle import oracle as orc
    ys, xs = np.mgrid[0:H, 0:W]
    o, d = orc.camera_rays(cam_desc, xs.ravel().astype(F) + F(0.5), ys.ravel().astype(F) + F(0.5))
    return features_from_hits(osc.closest_hit(o, d, use_bvh=False, n_threads=8), scene, W, H)


def features_from_hits(hits, scene, W, H, textured_albedo=None):
    """What prt_render_features stores, from HIT_DTYPE records of the centre rays.  textured_albedo: (n, 3) albedo as
    prt_hit_uv reports it (used for Lambertian / Metal hits), or None: the material table."""
    mats = scene.materials
    mtype = np.array([m.type for m in mats], np.uint32)
    mrgb = np.array([[m.rgb[0], m.rgb[1], m.rgb[2]] for m in mats], F)
    is_hit = hits["prim"] >= 0
    mid = np.where(is_hit, hits["material_id"], 0).astype(np.int64)
    diffuse = is_hit & ((mtype[mid] == 1) | (mtype[mid] == 2))
    src = mrgb[mid] if textured_albedo is None else np.asarray(textured_albedo, F)
    alb = np.where(diffuse[:, None], src, F(1)).astype(F)
    nrm = np.where(is_hit[:, None], hits["normal"], F(0)).astype(F)
    pos = np.where(is_hit[:, None], hits["position"], F(0)).astype(F)
    with np.errstate(all="ignore"):
        depth = np.where(is_hit, np.sqrt(hits["d2"]), F(0)).astype(F)
    prim = np.where(is_hit, hits["prim"], -1).astype(np.int32)
    return dict(albedo=alb.reshape(H, W, 3), normal=nrm.reshape(H, W, 3), position=pos.reshape(H, W, 3),
                depth=depth.reshape(H, W), prim=prim.reshape(H, W))


def synthetic(W, H, seed=1, cap=False):
    """Arrays for prt_denoise that exercise every case of the weight: a wall facing +z, a floor facing +y (perpendicular to
    it) or, with cap=True, a shallow sphere cap facing +z (normals within 0.1 rad of it), a tilted plane (N.N = 0.8 with the
    wall, 0.6 with the floor), miss regions, single-pixel islands of each kind inside the others, colours in [0, 2) and
    variances of which a quarter are exactly zero.  The normals' dot products are chosen so that max(0, N.N)^(2^k) never
    lands between 2^-149 and 2^-120 for k <= 8: the floor and the cap, whose products would, never share an image."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    u, v = (xs * F(0.05)).astype(F), (ys * F(0.05)).astype(F)
    N = np.zeros((H, W, 3), F)
    P = np.zeros((H, W, 3), F)
    prim = np.zeros((H, W), np.int32)
    N[..., 2] = 1                                            # the wall: prim 0
    P[..., 0], P[..., 1] = u, v
    second = (xs * 3 + ys * 2) % max(8, (W + H) // 2) < max(3, (W + H) // 6)     # diagonal bands
    if cap:
        R = F(40.0)
        cx, cy = F(W * 0.025), F(H * 0.025)
        nx, ny = ((u - cx) / R).astype(F), ((v - cy) / R).astype(F)
        inside = second & (np.hypot(nx, ny) < 0.09)
        nz = np.sqrt(np.maximum(F(0), F(1) - nx * nx - ny * ny)).astype(F)
        n = np.stack([nx, ny, nz], axis=-1)
        n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
        N[inside] = n[inside]
        P[inside] = (n[inside] * R).astype(F) + np.array([cx, cy, -R + F(0.5)], F)
        prim[inside] = 2
    else:
        N[second] = (0, 1, 0)                                # the floor: prim 1
        P[second] = np.stack([u[second], np.full(second.sum(), F(-0.3)), v[second]], axis=-1)
        prim[second] = 1
    tilted = (xs + 2 * ys) % max(10, W // 2 + 3) < 3
    N[tilted] = (0, F(0.6), F(0.8))
    P[tilted] = np.stack([u[tilted], (v[tilted] * F(0.8)).astype(F), (v[tilted] * F(-0.6)).astype(F)], axis=-1)
    prim[tilted] = 3
    miss = ((xs // max(3, W // 5) + ys // max(2, H // 4)) % 4 == 3)
    for (y, x), kind in zip(rng.integers(0, [H, W], (max(2, W * H // 40), 2)), range(10 ** 6)):   # single-pixel islands
        if kind % 2:
            miss[y, x] = True
        else:
            miss[y, x] = False
            N[y, x], P[y, x], prim[y, x] = (0, 0, 1), (u[y, x], v[y, x], F(0.25)), 4
    N[miss], P[miss], prim[miss] = 0, 0, -1
    alb = rng.uniform(0.0, 1.0, (H, W, 3)).astype(F)         # (below RHO_MIN in places)
    alb[rng.random((H, W)) < 0.05] = 0
    mean = rng.uniform(0.0, 2.0, (H, W, 3)).astype(F)
    var = (rng.uniform(1e-4, 0.2, (H, W)) * (rng.random((H, W)) < 0.75)).astype(F)
    return dict(mean=mean, var=var, albedo=alb, normal=N, position=P, prim=prim)
