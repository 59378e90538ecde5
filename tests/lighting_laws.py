"""Float64 per-pixel laws of one light-sampled sample (include/prt.h PrtLighting), for the one-bounce scenes of
closed_form.py: a Lambertian ground point (normal n) under ONE light, a two-sided emissive quad (kind D) or an emissive
sphere wholly above the ground (kind E), under a constant sky.  Nothing here calls the renderer or the oracle.

One sample of a ground pixel is X = X_B + X_L, two independent parts (the light sample draws from its own stream):
  X_B  the scattered segment: cosine-distributed; it meets the light with probability F (emission E weighted by w_B) or
       the sky (L); times the albedo, with Russian roulette at rr_depth 1 (survival p = max(albedo), survivors / p) and the
       clamp on the delivered term
  X_L  the light sample: a E (n.w / pi) w_L / pdf_L, pdf_L = pmf pdf_w, clamped on its own; with probability 1 - pmf the
       sample goes to another light that contributes nothing here (pmf < 1 only in the checks of this module)
Both are integrals over the light, done by Gauss-Legendre quadrature in the light's own sampling parameters (u1, u2): the
light sample IS uniform in them, and the scattered segment's hit has mass pdf_B / pdf_w per unit of them.  The integrands
are smooth (without clamp), so Q = 12 nodes per axis (8 for whole frames) give the moments far below the statistical
resolution; the mean
without clamp is also exact in closed form, a E F + a L (1 - F) (closed_form.form_factor; F = cos(theta) R^2 / D^2 for a
sphere), which the tests compare with the quadrature.  mode "mis": power heuristic; "nee": w_L = 1, w_B = 0."""
from __future__ import annotations

import numpy as np

import closed_form as cf

Q = 12
_GX, _GW = np.polynomial.legendre.leggauss(Q)
U = 0.5 * (_GX + 1.0)           # nodes on [0, 1]
UW = 0.5 * _GW                  # weights (sum 1)


def _f64(v):
    return np.asarray(v, np.float32).astype(np.float64)


def light_nodes(p, light, q=Q):
    """For ground points p [m, 3]: per quadrature node (u1, u2) the direction w [m, K, 3], distance^2 to the light point d2,
    solid-angle pdf of the light's sampling pdf_w [m, K] and the node weight [K].
    light: ("quad", mat16, w, h) or ("sphere", centre, R)."""
    gx, gw = np.polynomial.legendre.leggauss(q)
    uq, uw = 0.5 * (gx + 1.0), 0.5 * gw
    u1, u2 = np.meshgrid(uq, uq, indexing="ij")
    u1, u2 = u1.ravel(), u2.ravel()
    wq = np.outer(uw, uw).ravel()
    if light[0] == "quad":
        A, t0 = cf.quad_frame(light[1])
        uu, vv = light[2] * A[:, 0], light[3] * A[:, 2]
        area = abs(light[2] * light[3]) * (A[:, 0] @ A[:, 0])
        nl = np.cross(A[:, 0], A[:, 2])
        nl /= np.linalg.norm(nl)
        y = t0 + (u1 - 0.5)[:, None] * uu + (u2 - 0.5)[:, None] * vv          # [K, 3]
        v = y[None, :, :] - p[:, None, :]
        d2 = (v ** 2).sum(2)
        w = v / np.sqrt(d2)[..., None]
        pdf_w = d2 / (area * np.abs(w @ nl))
        return w, d2, pdf_w, wq
    c, R = np.asarray(light[1], np.float64), float(light[2])
    cd = c[None, :] - p
    D2 = (cd ** 2).sum(1)
    q = R * R / D2
    omc = q / (1.0 + np.sqrt(1.0 - q))                                       # [m]
    a = u1[None, :] * omc[:, None]
    cos_t, sin_t = 1.0 - a, np.sqrt(a * (2.0 - a))
    phi = 2.0 * np.pi * u2[None, :]
    wc = cd / np.sqrt(D2)[:, None]
    t1 = np.cross(wc, np.where(np.abs(wc[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]]))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(wc, t1)
    w = (t1[:, None, :] * (sin_t * np.cos(phi))[..., None] + t2[:, None, :] * (sin_t * np.sin(phi))[..., None]
         + wc[:, None, :] * cos_t[..., None])
    tn = np.sqrt(D2)[:, None] * cos_t - np.sqrt(np.maximum(R * R - D2[:, None] * a * (2 - a), 0.0))
    return w, tn ** 2, np.broadcast_to((1.0 / (2.0 * np.pi * omc))[:, None], a.shape), wq


def _mom(prob, val):
    """Raw -> (mean, var, fourth central moment, min, max) of a discrete law over axis 1 (prob [m, K], val [m, K])."""
    mu = (prob * val).sum(1)
    dv = val - mu[:, None]
    var = np.maximum((prob * dv ** 2).sum(1), 0.0)
    m4 = (prob * dv ** 4).sum(1)
    big = np.where(prob > 0, val, -np.inf).max(1)
    small = np.where(prob > 0, val, np.inf).min(1)
    return mu, var, m4, small, big


def ground_moments(p, n, light, mode, albedo, emission, sky, rr=0, clamp=0.0, pmf=1.0, max_depth=5, wrong=None, q=Q):
    """Per ground point: mean, variance, fourth central moment and spread of the channel sum of ONE sample.
    wrong (checks of the statistics only): "double" (w_L = w_B = 1), "no_cos_l" (pdf_w without |n_l.w|),
    "no_pmf" (the light sample not divided by pmf), "last" (a light sample also where the vertex cannot scatter)."""
    a, E, L = _f64(albedo), _f64(emission), _f64(sky)
    m = len(p)
    if max_depth < 2 and wrong != "last":
        z = np.zeros(m)
        return z, z.copy(), z.copy(), z.copy()
    w, d2, pdf_w, wq = light_nodes(p, light, q)
    if wrong == "no_cos_l" and light[0] == "quad":
        A, _ = cf.quad_frame(light[1])
        pdf_w = d2 / (abs(light[2] * light[3]) * (A[:, 0] @ A[:, 0]))
    cos = np.einsum("mkj,mj->mk", w, n)
    pb = np.maximum(cos, 0.0) / np.pi
    pl = pmf * pdf_w
    wl = np.ones_like(pl) if mode == "nee" or wrong == "double" else pl ** 2 / (pl ** 2 + pb ** 2)
    wb = np.ones_like(pl) if wrong == "double" else (np.zeros_like(pl) if mode == "nee" else pb ** 2 / (pl ** 2 + pb ** 2))
    lim = clamp if clamp > 0 else np.inf
    # light sample: picked w.p. pmf, uniform in (u1, u2)
    f = np.where(cos > 0, pb * wl / (pdf_w if wrong == "no_pmf" else pl), 0.0)
    vL = np.minimum(lim, (a * E)[None, None, :] * f[..., None]).sum(2)           # [m, K]
    probL = np.concatenate([pmf * wq[None, :] * np.ones((m, 1)), np.full((m, 1), 1.0 - pmf)], 1)
    valL = np.concatenate([vL, np.zeros((m, 1))], 1)
    muL, varL, m4L, loL, hiL = _mom(probL, valL)
    if max_depth < 2:  # ("last": the wrong estimator's light sample alone; the ground emits nothing)
        return muL, varL, m4L, hiL - loL
    # scattered segment: hit mass per node pdf_B / pdf_w * weight; the sky takes the rest
    hit = wq[None, :] * pb / pdf_w
    F = hit.sum(1)
    s = 1.0
    pk = 1.0
    if rr:
        pk = min(max(a.max(), 0.05), 1.0)
        s = 1.0 / pk
    vB = np.minimum(lim, (a * E * s)[None, None, :] * wb[..., None]).sum(2)
    vS = np.minimum(lim, a * L * s).sum()
    probB = np.concatenate([pk * hit, (pk * (1.0 - F))[:, None], np.full((m, 1), 1.0 - pk)], 1)
    valB = np.concatenate([vB, np.full((m, 1), vS), np.zeros((m, 1))], 1)
    muB, varB, m4B, loB, hiB = _mom(probB, valB)
    return muB + muL, varB + varL, m4B + m4L + 6.0 * varB * varL, (hiB - loB) + (hiL - loL)


def exact_mean(p, n, light, albedo, emission, sky):
    """a E F + a L (1 - F), channel sum (unclamped, any mode, any roulette)."""
    a, E, L = _f64(albedo), _f64(emission), _f64(sky)
    if light[0] == "quad":
        F = cf.form_factor(p, n, cf.quad_corners(light[1], light[2], light[3]))
    else:
        v = np.asarray(light[1], np.float64)[None, :] - p
        D2 = (v ** 2).sum(1)
        F = (v @ np.asarray([0.0, 1.0, 0.0])) / np.sqrt(D2) * light[2] ** 2 / D2
    return (a * E).sum() * F + (a * L).sum() * (1.0 - F)


def frame_law(o, d, ground, light, mode, albedo, emission, sky, rr=0, clamp=0.0, max_depth=5, chunk=32768, q=8):
    """Per pixel of a frame whose primary rays are (o, d): moments dict for frame_stats.  ground: (mat16, w, h); pixels
    on the ground get ground_moments, the rest see the sky (exact, value L); the light must not be in view."""
    n = len(o)
    tg, pg, _, _, exg = cf.quad_hit(o, d, *ground)
    on_g = np.isfinite(tg)
    A, _ = cf.quad_frame(ground[0])
    ng = A[:, 1] / np.linalg.norm(A[:, 1])
    mu, var, m4, spread = (np.zeros(n) for _ in range(4))
    idx = np.nonzero(on_g)[0]
    for k in range(0, len(idx), chunk):
        ii = idx[k:k + chunk]
        r = ground_moments(pg[ii], np.tile(ng, (len(ii), 1)), light, mode, albedo, emission, sky, rr, clamp, 1.0, max_depth, q=q)
        mu[ii], var[ii], m4[ii], spread[ii] = r
    exact = np.full((n, 3), np.nan, np.float32)
    sky32 = np.asarray(sky, np.float32)
    exact[~on_g] = sky32 if not clamp else np.minimum(np.float32(clamp), sky32)
    mu[~on_g] = exact[~on_g].astype(np.float64).sum(1)
    return dict(mu=mu, var=var, m4=m4, spread=spread, exact=exact, excluded=exg, on_g=on_g)


def frame_stats(accum, weights, S, law, W, H):
    """closed_form.frame_stats restated on moments (a light-sampled law has no two-point lattice): z per pixel against
    mean and variance, sum z^2 over the well-sampled pixels (S var / spread^2 >= 1) with Var z^2 = 2 + excess kurtosis / S,
    max |z| where S var / spread^2 >= 10, frame Z, 8x8-tile Z; point-law pixels compared bit for bit."""
    acc = accum.reshape(-1, 3)
    w = weights.reshape(-1)
    n = W * H
    res = {"S": S, "n": n, "weights_ok": bool(np.all(w == np.float32(S)))}
    keep = ~law["excluded"]
    res["excluded"] = int((~keep).sum())
    ex = keep & np.all(np.isfinite(law["exact"]), axis=1)
    want = cf.seq_sum_f32(law["exact"][ex], S)
    res["exact_pixels"] = int(ex.sum())
    res["exact_mismatch"] = int((~np.all(acc[ex] == want, axis=1)).sum())
    mu, var, m4, spread = law["mu"], law["var"], law["m4"], law["spread"]
    st = keep & ~ex & (var > 0)
    X = acc[st].astype(np.float64).sum(axis=1)
    z = (X - S * mu[st]) / np.sqrt(S * var[st])
    N = int(st.sum())
    res["N"] = N
    if N:
        ns = S * var[st] / np.maximum(spread[st], 1e-300) ** 2
        ws = ns >= 1
        vz2 = 2 + (m4[st] / var[st] ** 2 - 3) / S
        res["N_chi2"] = int(ws.sum())
        res["chi2"] = float((z[ws] ** 2).sum())
        res["chi2_dev"] = float((res["chi2"] - ws.sum()) / np.sqrt(vz2[ws].sum())) if ws.any() else 0.0
        big = ns >= 10
        res["maxz"] = float(np.abs(z[big]).max()) if big.any() else 0.0
        res["Z"] = float((X - S * mu[st]).sum() / np.sqrt((S * var[st]).sum()))
        pix = np.nonzero(st)[0]
        tile = (pix // W // 8) * ((W + 7) // 8) + (pix % W) // 8
        num = np.bincount(tile, X - S * mu[st])
        den = np.bincount(tile, S * var[st])
        cnt = np.bincount(tile, ns)
        ok = cnt >= 10
        res["tileZ"] = float(np.abs(num[ok] / np.sqrt(den[ok])).max()) if ok.any() else 0.0
    return res


def passes(r, z_max=6.5, chi2_sig=6.0, Z_max=6.0, tile_max=6.0):
    """closed_form.passes on the moment-based statistics."""
    if not r["weights_ok"] or r["exact_mismatch"]:
        return False
    if r["N"] == 0:
        return True
    return (abs(r["chi2_dev"]) <= chi2_sig and r["maxz"] <= z_max and abs(r["Z"]) <= Z_max and r["tileZ"] <= tile_max)


# ---- a plain float64 Monte Carlo of the same estimator (the module's own check) -------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _hit_light(x, w, light):
    """Distance^2 along w from x to the light, inf on a miss."""
    if light[0] == "quad":
        A, t0 = cf.quad_frame(light[1])
        nl = _unit(np.cross(A[:, 0], A[:, 2]))
        den = w @ nl
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((t0 - x) @ nl) / den
        y = x + t[..., None] * w
        lx = ((y - t0) @ A[:, 0]) / (A[:, 0] @ A[:, 0])
        lz = ((y - t0) @ A[:, 2]) / (A[:, 2] @ A[:, 2])
        ok = (t > 0) & (np.abs(lx) < light[2] / 2) & (np.abs(lz) < light[3] / 2)
        return np.where(ok, t * t, np.inf)
    c, R = np.asarray(light[1], np.float64), light[2]
    oc = x - c
    b = (oc * w).sum(-1)
    h = b * b - ((oc * oc).sum(-1) - R * R)
    t = -b - np.sqrt(np.maximum(h, 0))
    return np.where((h > 0) & (t > 0), t * t, np.inf)


def mc_samples(rng, p, n, light, mode, albedo, emission, sky, S, rr=0, clamp=0.0, pmf=1.0, max_depth=5, wrong=None):
    """S samples of the channel sum at each ground point, drawn as the renderer draws them: the scattered direction
    normalize(n + random unit vector), the light sample uniform in its parameters.  -> [m, S]."""
    a, E, L = _f64(albedo), _f64(emission), _f64(sky)
    m = len(p)
    lim = clamp if clamp > 0 else np.inf
    x = np.repeat(p[:, None, :], S, 1)
    nn = np.repeat(n[:, None, :], S, 1)
    out = np.zeros((m, S))
    scat = max_depth >= 2
    if scat or wrong == "last":  # light sample
        u1, u2, u0 = rng.random((m, S)), rng.random((m, S)), rng.random((m, S))
        if light[0] == "quad":
            A, t0 = cf.quad_frame(light[1])
            y = t0 + (u1 - 0.5)[..., None] * (light[2] * A[:, 0]) + (u2 - 0.5)[..., None] * (light[3] * A[:, 2])
            v = y - x
            d2 = (v * v).sum(-1)
            w = v / np.sqrt(d2)[..., None]
            nl = _unit(np.cross(A[:, 0], A[:, 2]))
            area = abs(light[2] * light[3]) * (A[:, 0] @ A[:, 0])
            pdf_w = d2 / (area * (1.0 if wrong == "no_cos_l" else np.abs(w @ nl)))
        else:
            c, R = np.asarray(light[1], np.float64), light[2]
            cd = c - x
            D2 = (cd * cd).sum(-1)
            q = R * R / D2
            omc = q / (1 + np.sqrt(1 - q))
            aa = u1 * omc
            cos_t, sin_t = 1 - aa, np.sqrt(aa * (2 - aa))
            phi = 2 * np.pi * u2
            wc = cd / np.sqrt(D2)[..., None]
            t1 = _unit(np.cross(wc, np.array([1.0, 0.0, 0.0])))
            t2 = np.cross(wc, t1)
            w = t1 * (sin_t * np.cos(phi))[..., None] + t2 * (sin_t * np.sin(phi))[..., None] + wc * cos_t[..., None]
            pdf_w = 1 / (2 * np.pi * omc)
        cos = (w * nn).sum(-1)
        pb = np.maximum(cos, 0) / np.pi
        pl = pmf * pdf_w
        wl = np.ones_like(pl) if mode == "nee" or wrong == "double" else pl ** 2 / (pl ** 2 + pb ** 2)
        f = np.where((cos > 0) & (u0 < pmf), pb * wl / (pdf_w if wrong == "no_pmf" else pl), 0.0)
        out += np.minimum(lim, (a * E)[None, None, :] * f[..., None]).sum(-1)
    if not scat:
        return out
    rv = rng.normal(size=(m, S, 3))
    w = _unit(nn + _unit(rv))
    d2 = _hit_light(x, w, light)
    hit = np.isfinite(d2)
    cos = (w * nn).sum(-1)
    pb = np.maximum(cos, 0) / np.pi
    if light[0] == "quad":
        A, _ = cf.quad_frame(light[1])
        nl = _unit(np.cross(A[:, 0], A[:, 2]))
        area = abs(light[2] * light[3]) * (A[:, 0] @ A[:, 0])
        pdf_w = d2 / (area * (1.0 if wrong == "no_cos_l" else np.abs(w @ nl)))
    else:
        c, R = np.asarray(light[1], np.float64), light[2]
        D2 = ((c - x) ** 2).sum(-1)
        q = R * R / D2
        pdf_w = 1 / (2 * np.pi * (q / (1 + np.sqrt(1 - q))))
    pl = pmf * pdf_w
    wb = np.ones_like(pl) if wrong == "double" else (np.zeros_like(pl) if mode == "nee" else pb ** 2 / (pl ** 2 + pb ** 2))
    s = 1.0
    alive = np.ones((m, S), bool)
    if rr:
        pk = min(max(a.max(), 0.05), 1.0)
        alive = rng.random((m, S)) < pk
        s = 1.0 / pk
    vB = np.where(hit[..., None], (a * E * s)[None, None, :] * wb[..., None], (a * L * s)[None, None, :])
    out += np.where(alive, np.minimum(lim, vB).sum(-1), 0.0)
    return out
