"""Closed-form float64 references for one-object scenes under a constant sky, and the statistics that hold a rendered
frame to them.  Plain numpy: nothing here calls the oracle's tracer or the kernels; the only inputs
taken from the renderer's side are the fp32 primary rays (prt_camera_rays / oracle.camera_rays, bit-exact to each
other) and the scene's fp32 parameters.

Semantics restated from include/prt.h and the reference's CPURenderer::TraceRay (cpu/renderer.cpp:59-103), not from
the oracle's code: a path adds throughput * sky when a segment misses and throughput * emission when it hits an
emitter; Lambertian, Metal and Dielectric multiply the throughput by their attenuation (albedo, albedo, 1); a metal
scatter whose new direction has dot(out, n) <= 0 is absorbed; the dielectric reflects with Schlick's probability,
r0 = ((1 - ri) / (1 + ri))^2; max_depth counts ray segments.  With one convex object (or a plane and an emitter
that cannot see each other's back) every path has at most a handful of segments whose law is known exactly:

  A  Lambertian sphere / convex flat-shaded mesh, albedo a: fl(a L) on object pixels, L elsewhere   (sigma = 0)
  B  metal sphere, fuzz f: fl(a L) w.p. P, else 0; P = clamp((1 + cos_i / f) / 2, 0, 1)  (u.n is uniform on [-1, 1])
  C  dielectric sphere: L w.p. R0 1{D >= 2} + (1 - R0) sum_{k=0}^{D-3} R1^k (1 - R1), else 0
  D  Lambertian ground under a two-sided emissive rectangle E: a E w.p. F (Lambert's form factor), else a L

Every pixel's per-sample value takes a few values with known probabilities (`Dist`), so mean, variance and the
per-depth ray-count law follow.  The values are really k 2^-24 lattice draws; at the sample counts used here that
resolution is far below the statistical one, so the probabilities are treated as continuous.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

# ---- pixel exclusion margins (relative, in f64): decisions this close to a boundary are ill-conditioned in fp32 -----
SIL_MARGIN = 1e-4     # |closest approach / R - 1| of a sphere's silhouette
EDGE_MARGIN = 1e-4    # distance of a quad hit point to an edge, in units of the quad's half size
COS_MIN = 1e-3        # grazing hits
MAX_EXCLUDED = 0.005  # every test asserts that at most this share of the pixels is excluded
ACNE_PER_PATH = 1e-6  # ray-count slack for self-hits at grazing exits (depth_counts_z)


@dataclass
class Dist:
    """Per-pixel law of one sample: value vals[k] (RGB, f64) with probability probs[k] and n_seg[k] ray segments.
    `exact` holds the fp32 per-sample value where the law is a single point (NaN elsewhere); `excluded` marks
    pixels too close to an ill-conditioned decision."""
    probs: np.ndarray     # [K, n]
    vals: np.ndarray      # [K, n, 3]
    nseg: np.ndarray      # [K, n] int
    exact: np.ndarray     # [n, 3] float32
    excluded: np.ndarray  # [n] bool
    extra: dict = field(default_factory=dict)

    @property
    def n(self):
        return self.probs.shape[1]


def dist_from(outcomes, n, exact=None, excluded=None):
    """outcomes: list of (prob [n], value [n,3] or [3], n_seg [n] or int)."""
    K = len(outcomes)
    probs = np.zeros((K, n))
    vals = np.zeros((K, n, 3))
    nseg = np.zeros((K, n), np.int64)
    for k, (p, v, s) in enumerate(outcomes):
        probs[k] = p
        vals[k] = np.broadcast_to(np.asarray(v, np.float64), (n, 3)) if np.ndim(v) < 2 else v
        nseg[k] = s
    if exact is None:
        exact = np.full((n, 3), np.nan, np.float32)
    if excluded is None:
        excluded = np.zeros(n, bool)
    return Dist(probs, vals, nseg, exact, excluded)


def select(mask, a: Dist, b: Dist) -> Dist:
    """Per pixel: a where mask, else b (same K after padding with zero-probability outcomes)."""
    K = max(a.probs.shape[0], b.probs.shape[0])

    def pad(d):
        k = K - d.probs.shape[0]
        return (np.concatenate([d.probs, np.zeros((k, d.n))]), np.concatenate([d.vals, np.zeros((k, d.n, 3))]),
                np.concatenate([d.nseg, np.ones((k, d.n), np.int64)]))
    pa, va, sa = pad(a)
    pb, vb, sb = pad(b)
    m = mask[None, :]
    return Dist(np.where(m, pa, pb), np.where(m[..., None], va, vb), np.where(m, sa, sb),
                np.where(mask[:, None], a.exact, b.exact), np.where(mask, a.excluded, b.excluded))


def average(d: Dist, group: int) -> Dist:
    """Mixture of `group` consecutive rays per pixel with equal weights (jitter's sub-pixel grid)."""
    K, n = d.probs.shape
    m = n // group
    probs = (d.probs.reshape(K, m, group) / group).transpose(0, 2, 1).reshape(K * group, m)
    vals = d.vals.reshape(K, m, group, 3).transpose(0, 2, 1, 3).reshape(K * group, m, 3)
    nseg = d.nseg.reshape(K, m, group).transpose(0, 2, 1).reshape(K * group, m)
    ex = d.exact.reshape(m, group, 3)
    same = np.all(ex == ex[:, :1], axis=(1, 2))
    exact = np.where(same[:, None], ex[:, 0], np.float32(np.nan)).astype(np.float32)
    # a sub-ray in an exclusion band is one of `group` equal-weight points of a continuum whose band has measure ~0:
    # the pixel is only excluded when a quarter of its grid is
    return Dist(probs, vals, nseg, exact, d.excluded.reshape(m, group).mean(axis=1) > 0.25)


# ---- sampling upgrades (include/prt.h PrtSampling) ------------------------------------------------------------------
def with_roulette(d: Dist, thr_after_first, max_depth):
    """rr_depth = 1 on a law whose only scatter starts segment 1 (kinds A, B, D): that scatter survives with
    p = clamp(max component of the throughput, 0.05, 1) and the survivor's value is divided by p."""
    p = float(np.clip(np.max(thr_after_first), 0.05, 1.0))
    if max_depth < 2 or p >= 1.0:
        return d
    probs, vals, nseg = [], [], []
    for k in range(d.probs.shape[0]):
        scat = d.nseg[k] >= 2
        probs.append(np.where(scat, d.probs[k] * p, d.probs[k]))
        vals.append(np.where(scat[:, None], d.vals[k] / p, d.vals[k]))
        nseg.append(d.nseg[k])
        probs.append(np.where(scat, d.probs[k] * (1 - p), 0.0))    # killed after the primary segment: nothing added
        vals.append(np.zeros_like(d.vals[k]))
        nseg.append(np.ones_like(d.nseg[k]))
    exact = np.where((d.nseg.max(axis=0) >= 2)[:, None], np.float32(np.nan), d.exact).astype(np.float32)
    return Dist(np.array(probs), np.array(vals), np.array(nseg), exact, d.excluded)


def with_clamp(d: Dist, c: float) -> Dist:
    c32 = np.float32(c)
    return Dist(d.probs, np.minimum(d.vals, float(c32)), d.nseg, np.minimum(d.exact, c32), d.excluded)


# ---- geometry in float64 from the fp32 rays -------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def sphere_hit(o, d, center, R):
    """-> hit mask, cos_i, excluded mask (silhouette band / grazing)."""
    o = o.astype(np.float64)
    d = _unit(d.astype(np.float64))
    oc = o - np.asarray(center, np.float64)
    b = np.einsum("ij,ij->i", oc, d)
    h2 = np.maximum(np.einsum("ij,ij->i", oc, oc) - b * b, 0.0)
    hit = (h2 < R * R) & (b < 0)
    cos_i = np.sqrt(np.maximum(R * R - h2, 0.0)) / R
    excl = (np.abs(np.sqrt(h2) / R - 1.0) < SIL_MARGIN) | (hit & (cos_i < COS_MIN))
    return hit, np.where(hit, cos_i, 0.0), excl


def quad_frame(mat16):
    """World <- local affine map of a primitive (column-major float[16], glm layout) in f64."""
    M = np.asarray(mat16, np.float64).reshape(4, 4).T
    return M[:3, :3], M[:3, 3]


def quad_hit(o, d, mat16, w, h, internal_edges=False):
    """Quad::Intersect in f64 (local y = 0 plane, |x| < w/2, |z| < h/2) for a rigid transform.
    -> t (inf on a miss), world hit point, local (x, z), cos_i, excluded mask."""
    A, t0 = quad_frame(mat16)
    Ai = np.linalg.inv(A)
    o = o.astype(np.float64)
    d = _unit(d.astype(np.float64))
    ol = (o - t0) @ Ai.T
    dl = _unit(d @ Ai.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        tl = -ol[:, 1] / dl[:, 1]
    pl = ol + dl * tl[:, None]
    x, z = pl[:, 0], pl[:, 2]
    front = (tl > 1e-3) & (np.abs(dl[:, 1]) >= 1e-8)
    inside = front & (np.abs(x) < w / 2) & (np.abs(z) < h / 2)
    p = pl @ A.T + t0
    cos_i = np.abs(dl[:, 1])
    edge = np.minimum(np.abs(np.abs(x) - w / 2) / (w / 2), np.abs(np.abs(z) - h / 2) / (h / 2))
    excl = (front & (edge < EDGE_MARGIN)) | (inside & (cos_i < COS_MIN))
    if internal_edges:  # scenes.triangulate_quads: 2x2 cells, each split along its anti-diagonal (not watertight)
        u, v = (x + w / 2) / (w / 2), (z + h / 2) / (h / 2)      # cell coordinates in [0, 2)
        fu, fv = u - np.floor(u), v - np.floor(v)
        near = (np.minimum(np.abs(u - 1.0), np.abs(v - 1.0)) < EDGE_MARGIN) | (np.abs(fu + fv - 1.0) < EDGE_MARGIN)
        excl |= inside & near
    t = np.where(inside, np.linalg.norm(p - o, axis=1), np.inf)
    return t, p, np.stack([x, z], 1), cos_i, excl


def quad_corners(mat16, w, h):
    A, t0 = quad_frame(mat16)
    loc = np.array([[-w / 2, 0, -h / 2], [w / 2, 0, -h / 2], [w / 2, 0, h / 2], [-w / 2, 0, h / 2]], np.float64)
    return loc @ A.T + t0


def form_factor(p, n, corners):
    """Point-to-polygon form factor by Lambert's formula, F = (1/2pi) sum_i beta_i cos gamma_i: the probability that
    a cosine-distributed direction about n leaves p through the polygon."""
    r = _unit(corners[None, :, :] - p[:, None, :])          # [m, 4, 3]
    acc = np.zeros(len(p))
    for i in range(4):
        a, b = r[:, i], r[:, (i + 1) % 4]
        beta = np.arccos(np.clip(np.einsum("ij,ij->i", a, b), -1, 1))
        c = np.cross(a, b)
        acc += beta * np.einsum("ij,ij->i", _unit(c), n)
    return np.abs(acc) / (2 * np.pi)


def solid_angle_fraction(p, corners):
    """Share of the hemisphere's solid angle (uniform-hemisphere probability) the polygon subtends (power checks)."""
    def tri(a, b, c):
        num = np.abs(np.einsum("ij,ij->i", a, np.cross(b, c)))
        la, lb, lc = (np.linalg.norm(v, axis=1) for v in (a, b, c))
        den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", a, c) * lb \
            + np.einsum("ij,ij->i", b, c) * la
        return 2 * np.arctan2(num, den)
    v = corners[None, :, :] - p[:, None, :]
    return (tri(v[:, 0], v[:, 1], v[:, 2]) + tri(v[:, 0], v[:, 2], v[:, 3])) / (2 * np.pi)


def schlick(cos, ri, power=5):
    r0 = ((1 - ri) / (1 + ri)) ** 2
    return r0 + (1 - r0) * (1 - cos) ** power


# ---- the scene kinds --------------------------------------------------------------------------------------------------
def f32mul(a, b):
    return (np.asarray(a, np.float32) * np.asarray(b, np.float32)).astype(np.float32)


def sky_only(n, sky):
    sky32 = np.asarray(sky, np.float32)
    return dist_from([(np.ones(n), sky32.astype(np.float64), 1)], n, exact=np.tile(sky32, (n, 1)))


def kind_a(hit, excl, albedo, sky):
    """Lambertian convex object: every sample of an object pixel is fl(a L) with two segments."""
    n = hit.size
    v32 = f32mul(albedo, sky)
    obj = dist_from([(np.ones(n), v32.astype(np.float64), 2)], n, exact=np.tile(v32, (n, 1)))
    d = select(hit, obj, sky_only(n, sky))
    d.excluded = excl
    return d


def kind_b(hit, cos_i, excl, albedo, fuzz, sky, fuzz_law="sphere"):
    """Metal sphere: scattered iff cos_i + f u.n > 0 with u uniform on the unit sphere (u.n uniform on [-1, 1]).
    fuzz_law="ball" is a deliberately wrong reference (u uniform in the ball: u.n has density 3/4 (1 - x^2))."""
    n = hit.size
    v32 = f32mul(albedo, sky)
    if fuzz == 0:
        P = np.ones(n)
    else:
        t = np.clip(-cos_i / fuzz, -1.0, 1.0)
        P = (1 - t) / 2 if fuzz_law == "sphere" else 1 - (0.75 * (t - t ** 3 / 3) + 0.5)
    exact = np.where((P >= 1.0)[:, None], v32, np.float32(np.nan)).astype(np.float32)
    obj = dist_from([(P, v32.astype(np.float64), 2), (1 - P, 0.0, 1)], n, exact=exact)
    d = select(hit, obj, sky_only(n, sky))
    d.excluded = excl
    return d


def kind_c(hit, cos_i, excl, eta, max_depth, sky, power=5, r1_at_incidence=False):
    """Dielectric sphere.  R0 = Schlick(cos_i) on the way in; inside, every bounce meets the surface at the same
    angle, cos_t = sqrt(1 - sin_i^2 / eta^2), so R1 = Schlick(cos_t) at each internal hit; the escaping segment
    adds L.  (power / r1_at_incidence: deliberately wrong references for the power checks.)"""
    n = hit.size
    D = max_depth
    L = np.asarray(sky, np.float32).astype(np.float64)
    cos_t = np.sqrt(np.maximum(1 - (1 - cos_i ** 2) / eta ** 2, 0.0))
    R0 = schlick(cos_i, 1 / eta, power)
    R1 = schlick(cos_i if r1_at_incidence else cos_t, eta, power)
    if D == 1:
        outs = [(np.ones(n), 0.0, 1)]
    else:
        outs = [(R0, L, 2)]
        for k in range(0, D - 2):
            outs.append(((1 - R0) * R1 ** k * (1 - R1), L, k + 3))
        outs.append(((1 - R0) * R1 ** (D - 2), 0.0, D))   # still inside when the segments run out
    obj = dist_from(outs, n)
    d = select(hit, obj, sky_only(n, sky))
    d.excluded = excl
    d.extra.update(R0=R0, R1=R1)
    return d


def kind_d(o, d, ground, emitter, albedo, emission, sky, internal_edges=False, pdf="cosine"):
    """ground / emitter: (mat16, w, h).  A ground point scatters a cosine-distributed ray that reaches the emitter
    w.p. F (then a E, the emitter does not scatter) or the sky (a L).  The camera may see the emitter (value E) or
    the sky directly.  pdf="uniform": deliberately wrong reference (uniform hemisphere: F = solid angle / 2pi)."""
    n = len(o)
    tg, pg, _, cg, exg = quad_hit(o, d, *ground, internal_edges=internal_edges)
    te, _, _, _, exe = quad_hit(o, d, *emitter, internal_edges=internal_edges)
    on_e = np.isfinite(te) & (te <= tg)
    on_g = np.isfinite(tg) & ~on_e
    A, _ = quad_frame(ground[0])
    ng = _unit(np.tile(A[:, 1], (n, 1)))
    corners = quad_corners(*emitter)
    F = np.zeros(n)
    if pdf == "cosine":
        F[on_g] = form_factor(pg[on_g], ng[on_g], corners)
    else:
        F[on_g] = solid_angle_fraction(pg[on_g], corners)
    a = np.asarray(albedo, np.float32).astype(np.float64)
    E = np.asarray(emission, np.float32).astype(np.float64)
    L = np.asarray(sky, np.float32).astype(np.float64)
    g = dist_from([(F, a * E, 2), (1 - F, a * L, 2)], n)
    E32 = np.asarray(emission, np.float32)
    e = dist_from([(np.ones(n), E, 1)], n, exact=np.tile(E32, (n, 1)))
    out = select(on_g, g, select(on_e, e, sky_only(n, sky)))
    out.excluded = exg | exe
    out.extra.update(F=F, on_g=on_g)
    return out


# ---- convex flat-shaded mesh --------------------------------------------------------------------------------------
def geodesic_sphere(freq: int):
    """Icosahedron with every face cut into freq^2 triangles, vertices pushed onto the unit sphere, and per-face
    vertices whose normals are the face normal (flat shading: the shading normal IS the geometric one, so the
    object is convex to its own scattered rays).  -> positions [3m, 3], normals [3m, 3], indices [m, 3] (float32),
    and the f64 radii of the inscribed / circumscribed spheres of the fp32 mesh."""
    t = (1 + 5 ** 0.5) / 2
    V = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    F = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5],
                  [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    tris = []
    ii, jj = np.meshgrid(np.arange(freq + 1), np.arange(freq + 1), indexing="ij")
    for a, b, c in F:
        A, B, C = V[a], V[b], V[c]

        def P(i, j):
            return A + (B - A) * (i[..., None] / freq) + (C - A) * (j[..., None] / freq)
        i, j = np.meshgrid(np.arange(freq), np.arange(freq), indexing="ij")
        up = (i + j) < freq
        tris.append(np.stack([P(i[up], j[up]), P(i[up] + 1, j[up]), P(i[up], j[up] + 1)], 1))
        dn = (i + j) < freq - 1
        tris.append(np.stack([P(i[dn] + 1, j[dn]), P(i[dn] + 1, j[dn] + 1), P(i[dn], j[dn] + 1)], 1))
    T = np.concatenate(tris)
    T = (T / np.linalg.norm(T, axis=-1, keepdims=True)).astype(np.float32)
    T64 = T.astype(np.float64)
    nrm = np.cross(T64[:, 1] - T64[:, 0], T64[:, 2] - T64[:, 0])
    flip = np.einsum("ij,ij->i", nrm, T64.mean(axis=1)) < 0
    T[flip] = T[flip][:, ::-1]
    T64 = T.astype(np.float64)
    nrm = _unit(np.cross(T64[:, 1] - T64[:, 0], T64[:, 2] - T64[:, 0]))
    r_in = float(np.min(np.einsum("ij,ij->i", nrm, T64[:, 0])))
    r_out = float(np.max(np.linalg.norm(T64.reshape(-1, 3), axis=1)))
    m = len(T)
    pos = T.reshape(-1, 3)
    nor = np.repeat(nrm.astype(np.float32), 3, axis=0)
    idx = np.arange(3 * m, dtype=np.uint32).reshape(m, 3)
    return pos, nor, idx, r_in, r_out


def mesh_edge_band(o, d, pos, mat16=None, margin=1e-3, k=8):
    """Rays whose f64 hit on the triangle mesh `pos` [3m, 3] (mesh space; mat16 = the copy's placement) lies within
    `margin` (barycentric) of an edge of the face it hits.  Triangle::Intersect is not watertight: a primary ray
    through a shared edge can slip between two faces and meet the far side from inside (4 of 2.07 M pixels of the
    512 k-face geodesic sphere at 1080p, identical in the oracle and on the GPU).  Those pixels are excluded."""
    from scipy.spatial import cKDTree
    o = o.astype(np.float64)
    d = d.astype(np.float64)
    if mat16 is not None:
        A, t0 = quad_frame(mat16)
        Ai = np.linalg.inv(A)
        o = (o - t0) @ Ai.T
        d = d @ Ai.T
    d = _unit(d)
    T = pos.reshape(-1, 3, 3).astype(np.float64)
    b = np.einsum("ij,ij->i", o, d)
    h2 = np.einsum("ij,ij->i", o, o) - b * b
    cand = h2 < 1.0
    idx = np.nonzero(cand)[0]
    t = -b[idx] - np.sqrt(1.0 - h2[idx])
    p = o[idx] + d[idx] * t[:, None]
    _, nb = cKDTree(T.mean(axis=1)).query(p, k=k)
    best_t = np.full(idx.size, np.inf)
    best_m = np.full(idx.size, -np.inf)
    for j in range(k):
        P0, P1, P2 = T[nb[:, j], 0], T[nb[:, j], 1], T[nb[:, j], 2]
        E1, E2, Sv = P1 - P0, P2 - P0, o[idx] - P0
        S1 = np.cross(d[idx], E2)
        S2 = np.cross(Sv, E1)
        div = np.einsum("ij,ij->i", S1, E1)
        tt = np.einsum("ij,ij->i", S2, E2) / div
        b1 = np.einsum("ij,ij->i", S1, Sv) / div
        b2 = np.einsum("ij,ij->i", S2, d[idx]) / div
        m = np.minimum(np.minimum(b1, b2), 1 - b1 - b2)
        take = (m > -margin) & (tt > 0) & (tt < best_t)
        best_t = np.where(take, tt, best_t)
        best_m = np.where(take, m, best_m)
    band = np.zeros(len(o), bool)
    band[idx] = best_m < margin        # (no face found among the k nearest: excluded as well)
    return band


def convex_hit(o, d, center, r_in, r_out):
    """A convex object between two concentric spheres: certainly hit inside the inner one, certainly missed outside
    the outer one; rays in between (and a margin) are excluded."""
    hi, _, ei = sphere_hit(o, d, center, r_in)
    ho, _, eo = sphere_hit(o, d, center, r_out)
    return hi, (ho & ~hi) | ei | eo


# ---- statistics -------------------------------------------------------------------------------------------------------
def moments(d: Dist):
    """Per pixel mean, variance and fourth central moment of the channel sum of one sample."""
    v = d.vals.sum(axis=2)                       # [K, n]
    mu = (d.probs * v).sum(axis=0)
    dv = v - mu
    var = np.maximum((d.probs * dv ** 2).sum(axis=0), 0.0)
    m4 = (d.probs * dv ** 4).sum(axis=0)
    spread = v.max(axis=0, initial=-np.inf, where=d.probs > 0) - v.min(axis=0, initial=np.inf, where=d.probs > 0)
    return mu, var, m4, spread


def seq_sum_f32(v32, S):
    """Film::AddSample S times in fp32, in order: the film value of a pixel whose every sample is v32."""
    acc = np.zeros_like(v32, dtype=np.float32)
    for _ in range(S):
        acc = (acc + v32).astype(np.float32)
    return acc


def frame_stats(accum, weights, S, d: Dist, W, H):
    """z = (X/S - mu) / (sigma / sqrt S) per pixel (X = channel sum of the film); returns the numbers the
    assertions use.  Pixels whose law is a single point are compared exactly instead."""
    acc = accum.reshape(-1, 3)
    w = weights.reshape(-1)
    n = W * H
    assert acc.shape[0] == n == d.n
    res = {"S": S, "n": n, "weights_ok": bool(np.all(w == np.float32(S)))}
    keep = ~d.excluded
    res["excluded"] = int((~keep).sum())
    mu, var, m4, spread = moments(d)
    ex = keep & np.all(np.isfinite(d.exact), axis=1)
    want = seq_sum_f32(d.exact[ex], S)
    bad = ~np.all(acc[ex] == want, axis=1)
    res["exact_pixels"] = int(ex.sum())
    res["exact_mismatch"] = int(bad.sum())
    st = keep & ~ex & (var > 0)
    X = acc[st].astype(np.float64).sum(axis=1)
    # Most laws here have two values.  Their fp32 film sum is then decoded into the number of samples that took the
    # upper one: the fp32 accumulation error (< S ulp of the sum) is far below the gap, but NOT below sigma / sqrt S
    # of a pixel whose p is within 1e-6 of 0 or 1, where it would bias z.  A sum that is not within a quarter gap of
    # the two values' lattice means a sample took a value outside the law: counted in "off_lattice".
    v = d.vals[:, st].sum(axis=2)
    pos = d.probs[:, st] > 0
    hi = np.max(np.where(pos, v, -np.inf), axis=0)
    lo = np.min(np.where(pos, v, np.inf), axis=0)
    tol = 1e-9 * np.maximum(1.0, np.abs(hi))
    two = np.all(~pos | (np.abs(v - hi) <= tol) | (np.abs(v - lo) <= tol), axis=0)
    gap = hi - lo
    k = np.rint((X - S * lo) / np.where(two, gap, 1.0))
    resid = np.abs(X - S * lo - k * gap)
    res["off_lattice"] = int((two & ((resid > 0.25 * gap) | (k < 0) | (k > S))).sum())
    X = np.where(two, S * lo + k * gap, X)
    sd = np.sqrt(S * var[st])
    z = (X - S * mu[st]) / sd
    N = int(st.sum())
    res["N"] = N
    if N:
        # "well sampled": S p (1 - p) >= 1 (two-point laws; S sigma^2 / spread^2 in general).  Below that a pixel's z is a
        # rare-event count whose z^2 is heavy-tailed; such pixels still enter the frame aggregate Z.
        ns = S * var[st] / np.maximum(spread[st], 1e-300) ** 2
        ws = ns >= 1
        vz2 = 2 + (m4[st] / var[st] ** 2 - 3) / S   # Var(z^2) of a mean of S iid samples (= 2 for a normal law)
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
    """(a) |sum z^2 - N| within chi2_sig standard deviations of its law (Var z^2 = 2 + excess kurtosis / S, i.e.
    6 sqrt(2N) for normal z), over the well-sampled pixels; (b) max |z| <= 6.5 over pixels with S p (1 - p) >= 10;
    (c) whole-frame |Z| <= 6; (d) max |Z| <= 6 over 8x8 tiles holding sum S p (1 - p) >= 10; exact pixels all
    equal, two-valued sums on their lattice, weights = S.

    Why these hold although pixels share RNG streams (path_seed hashes pixel ^ sample * 719393): within one pixel the
    S streams are distinct (719393 is odd, so sample * 719393 differs for every sample), so each z is a sum of S
    independent draws.  Two pixels share a stream only for the few sample pairs whose products xor to the pixels'
    index difference, i.e. a pixel's sum shares O(1) of its S draws with any other pixel, which moves sum z^2 and the
    aggregates by O(1/S) of their spread; the measured values (test files) sit well inside the bounds."""
    if not r["weights_ok"] or r["exact_mismatch"] or r.get("off_lattice", 0):
        return False
    if r["N"] == 0:
        return True
    return (abs(r["chi2_dev"]) <= chi2_sig and r["maxz"] <= z_max and abs(r["Z"]) <= Z_max
            and r["tileZ"] <= tile_max)


def depth_counts_z(rays_per_depth, S, d: Dist, max_depth):
    """z of the per-depth ray counts: segments at depth k = paths with more than k segments; each pixel contributes
    a binomial(S, P(n_seg > k)).  Exact (z = 0 required) where every P is 0 or 1.  Slack: S segments per excluded
    pixel, plus ACNE_PER_PATH of all paths for tmin acne (a metal reflection fuzzed to just above the tangent plane at
    a grazing hit can start inside the sphere by a rounding error and meet it again: 1-3 extra segments per 8-17 M
    paths in the oracle with this file's seeds, film unchanged)."""
    keep = ~d.excluded
    out = []
    slack = S * (~keep).sum() + ACNE_PER_PATH * S * d.n
    for k in range(max_depth):
        P = (d.probs * (d.nseg > k)).sum(axis=0)
        mean = S * P.sum()
        var = S * (P * (1 - P)).sum()
        got = float(rays_per_depth[k])
        dev = max(0.0, abs(got - mean) - slack)
        out.append((got, mean, var, dev / np.sqrt(var) if var > 0 else (0.0 if dev == 0 else np.inf)))
    return out


# ---- the scenes and cameras the tests render --------------------------------------------------------------------------
SKY = (0.4, 0.3, 0.6)
ALBEDO = (0.7, 0.5, 0.3)
GROUND_ALBEDO = (0.5, 0.6, 0.7)
EMISSION = (15.0, 12.0, 9.0)
SPHERE_CAM = (0.4, 0.3, 3.0)          # looks at the origin; a unit sphere there covers ~21 % of the frame
GROUND_CAM = ((0.0, 3.0, 6.0), (0.0, -4.0, -6.0))   # below the emitter, looking down: ground and sky, never the emitter


def sphere_scene(prt, kind, param=0.0, sky=SKY):
    sc = prt.Scene(preset=None, sky=sky)
    if kind == "A":
        m = sc.AddLambertian(ALBEDO)
    elif kind == "B":
        m = sc.AddMetal(ALBEDO, param)
    else:
        m = sc.AddDielectric(param)
    sc.AddCircle(1.0, m)
    return sc


def ground_scene(prt, sky=SKY):
    """Kind D: mesh_scene's ground quad and two-sided emitter without the mesh.  -> scene, ground, emitter
    ((mat16, w, h) each)."""
    sc = prt.Scene(preset=None, sky=sky)
    g = sc.AddLambertian(GROUND_ALBEDO)
    e = sc.AddEmissive(EMISSION)
    sc.AddQuad(20.0, 20.0, g, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, e, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    gp, ep = sc.primitives
    return sc, (list(gp.mat), 20.0, 20.0), (list(ep.mat), 4.0, 4.0)


def camera(prt, which, W, H):
    if which == "sphere":
        return prt.Camera(SPHERE_CAM, width=W, height=H)
    pos, look = GROUND_CAM
    return prt.Camera(pos, front=prt.glm_normalize(np.asarray(look, np.float32)), width=W, height=H)


def pixel_rays(ray_fn, W, H, sub=1):
    """The fp32 primary rays through pixel centres (sub = 1) or a sub x sub grid of sub-pixel points (jitter's
    average), pixel-major, from ray_fn(px, py) = prt_camera_rays or oracle.camera_rays."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    g = (np.arange(sub) + 0.5) / sub
    gy, gx = np.meshgrid(g, g, indexing="ij")
    px = (xs.reshape(-1, 1) + gx.reshape(1, -1)).astype(np.float32).ravel()
    py = (ys.reshape(-1, 1) + gy.reshape(1, -1)).astype(np.float32).ravel()
    return ray_fn(px, py)


def reference(kind, o, d, param=None, max_depth=5, sky=SKY, ground=None, emitter=None, sampling=(0, 0, 0.0),
              mesh_radii=None, center=(0.0, 0.0, 0.0), scale=1.0, sub=1, mesh=None, **wrong):
    """The law of every pixel of a one-object frame.  sampling = (jitter, rr_depth, clamp); with jitter the rays
    are the sub x sub grid of pixel_rays and the law is their average.  mesh: (positions, mat16 or None) of a convex
    mesh whose primary rays through its edges are excluded."""
    if kind == "A":
        if mesh_radii is not None:
            hit, ex = convex_hit(o, d, center, mesh_radii[0] * scale, mesh_radii[1] * scale)
            if mesh is not None:
                ex |= hit & mesh_edge_band(o, d, mesh[0], mesh[1])
        else:
            hit, _, ex = sphere_hit(o, d, center, scale)
        dist = kind_a(hit, ex, ALBEDO, sky)
    elif kind == "B":
        hit, cos_i, ex = sphere_hit(o, d, center, scale)
        dist = kind_b(hit, cos_i, ex, ALBEDO, param, sky, **wrong)
    elif kind == "C":
        hit, cos_i, ex = sphere_hit(o, d, center, scale)
        dist = kind_c(hit, cos_i, ex, param, max_depth, sky, **wrong)
    else:
        dist = kind_d(o, d, ground, emitter, GROUND_ALBEDO, EMISSION, sky, **wrong)
    jitter, rr_depth, clamp = sampling
    if rr_depth == 1 and max_depth >= 2:
        dist = with_roulette(dist, (1.0, 1.0, 1.0) if kind == "C" else GROUND_ALBEDO if kind == "D" else ALBEDO, max_depth)
    if clamp > 0:
        dist = with_clamp(dist, clamp)
    if sub > 1:
        dist = average(dist, sub * sub)
    return dist
