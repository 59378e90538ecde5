"""Float64 replay of light-sampled frames under clustered light selection (include/prt.h "Clustered light selection").

Built on tests/mesh_light_replay.py (and through it tests/lighting_replay.py) without editing either: their walker, visibility
test, comparison, tolerances, light records, point on the light and pdf_w are used as they are.  What this module restates,
from the written contract and the cluster tables a context reads back (prt_light_clusters, prt_light_cluster_members):

  * the cluster choice at a vertex in numpy FLOAT32, operation for operation (thresholds()): it has no transcendental, every
    numpy float32 operation rounds once and numpy never contracts, so it is the device's M_c bit for bit;
  * the member by integers: the smallest j with r3 < U_{c,j}, r3 the state after the light stream's fourth step, U the
    running sums of the read-back inner widths;
  * the light's pmf P_c pmf_in, and the same number in the weight of a scattered segment that meets a light, with P_c
    evaluated at the segment's origin.

Everything downstream is float64 as in mesh_light_replay.  The tables are read back exactly, so the clustered choice adds no
unstable band: cluster and member are compared for equality.

`clustered(tables)` is a context manager that puts these three restatements in the place of mesh_light_replay's light set,
sample_lights and hit_weight for the calls made inside it, so mesh_light_replay.replay and environment_replay.replay run
unchanged on top of them.  `wrong=` selects a deliberately wrong estimator (WRONG), used only to show the comparison tells
them apart."""
from __future__ import annotations

import contextlib

import numpy as np

import lighting_replay as lr
import mesh_light_replay as mlr
from lighting_replay import M32, SHADOW_EPS, pcg, rnd
from util import prt

TWO32 = 4294967296.0
TWO24 = 16777216
F = np.float32
WRONG = ("phi_for_P", "wb_power_pmf")


def read_tables(r):
    """The cluster tables of renderer `r` (host-only or not): light_clusters() plus cluster / inner_width per light."""
    t = dict(r.light_clusters())
    t["cluster"], t["inner_width"] = r.light_cluster_members()
    return t


def thresholds(t, x):
    """M [n, K] uint32 for points x [n, 3] (taken as float32): the contract's cluster choice, fp32 operation for operation."""
    x = np.ascontiguousarray(x, F).reshape(-1, 3)
    lo, hi, r2, phi = (np.asarray(t[k], F) for k in ("lo", "hi", "r2", "phi"))
    K, n = len(phi), len(x)
    zero = F(0.0)
    cw, cp = np.zeros((n, K), F), np.zeros((n, K), F)
    acc_w, acc_p = np.zeros(n, F), np.zeros(n, F)
    with np.errstate(all="ignore"):
        for c in range(K):
            d = []
            for k in range(3):
                a = lo[c, k] - x[:, k]
                b = x[:, k] - hi[c, k]
                dk = np.where(a > b, a, b)
                d.append(np.where(dk > zero, dk, zero))
            D2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            den = np.where(D2 > r2[c], D2, r2[c])
            acc_w = acc_w + phi[c] / den
            acc_p = acc_p + phi[c]
            cw[:, c], cp[:, c] = acc_w, acc_p
        fb = ~((acc_w > zero) & (acc_w < F(np.inf)))
        cum = np.where(fb[:, None], cp, cw)
        inv = F(1.0) / cum[:, -1]
        q = (cum * inv[:, None]) * F(16777216.0)
        below = q < F(16777216.0)
        M = np.where(below, np.where(below, q, zero).astype(np.uint32), np.uint32(TWO24)).astype(np.uint32)
    M[:, -1] = TWO24
    return M


def cluster_prob(M, c):
    """P_c = (M_c - M_{c-1}) 2^-24 (float64, exact) for one cluster per row."""
    M = M.astype(np.int64)
    rows = np.arange(len(M))
    prev = np.where(c > 0, M[rows, np.maximum(c - 1, 0)], 0)
    return np.maximum(M[rows, c] - prev, 0) / float(TWO24)


class ClusteredLightSet(mlr.MeshLightSet):
    """mesh_light_replay.MeshLightSet under "all" with the read-back cluster tables: `cluster` [n], `inner` (pmf_in, exact,
    float64) [n], and per cluster the members (set order = candidate order) with their thresholds U."""

    tables = None   # set by clustered()

    def __init__(self, scene, sources="all"):
        super().__init__(scene, sources)
        assert sources == "all", "clustered selection is active only with the MESH bit"
        t = self.tables
        self.t = t
        self.cluster = np.asarray(t["cluster"], np.int64)
        assert len(self.cluster) == self.n, (len(self.cluster), self.n)
        self.inner = np.asarray(t["inner_width"], np.float64) / TWO32
        self.K = len(t["phi"])
        self.members = [np.nonzero(self.cluster == c)[0] for c in range(self.K)]
        self.U = [np.cumsum(np.asarray(t["inner_width"], np.float64)[m]) for m in self.members]

    def env_factor(self):
        """(2^32 - T_e) / 2^32 as environment_replay multiplied it into the global pmf (1 without an environment)."""
        return float(self.pmf[0] / (self.width[0] / TWO32)) if self.n else 1.0


def light_draws4(keys):
    """(m, r3, u1, u2): u0's 24-bit integer, the 32-bit state after the light stream's fourth step, the second and third draws."""
    s = pcg((np.asarray(keys).astype(np.uint64) + lr.LIGHT_RNG) & M32)
    _, s = rnd(s)
    m = (s.astype(np.uint64) >> 8).astype(np.int64)
    u1, s = rnd(s)
    u2, s = rnd(s)
    r3 = pcg(s).astype(np.float64)
    return m, r3, u1, u2


def select(ls: ClusteredLightSet, x, keys):
    """-> (light [n] set index, cluster [n], P [n], pmf_in [n], M [n, K]) of the clustered choice at x with the keys' draws."""
    m, r3, _, _ = light_draws4(keys)
    M = thresholds(ls.t, x)
    cl = np.minimum((m[:, None] >= M.astype(np.int64)).sum(1), ls.K - 1)
    P = cluster_prob(M, cl)
    li = np.zeros(len(m), np.int64)
    for c in np.unique(cl):
        rows = np.nonzero(cl == c)[0]
        U, mem = ls.U[c], ls.members[c]
        li[rows] = mem[np.minimum(np.searchsorted(U, r3[rows], side="right"), len(mem) - 1)]
    return li, cl, P, ls.inner[li], M


def sample_lights(ls: ClusteredLightSet, x, n, keys, mode, wrong=None):
    """mesh_light_replay.sample_lights with the clustered choice in the place of the global thresholds: the same dict."""
    li, cl, P, pin, _ = select(ls, x, keys)
    if wrong == "phi_for_P":
        P = np.asarray(ls.t["phi"], np.float64)[cl]
    pmf = P * pin * ls.env_factor()
    # the point on the light, pdf_w and the weights: mesh_light_replay's, evaluated for the chosen light by handing it a
    # light set whose threshold search can only return li (one light per row is not what its search does, so the few lines
    # downstream of the choice are repeated from its text)
    _, _, u1, u2 = light_draws4(keys)
    kind = ls.kind[li]
    flat = kind != 0
    sq = np.sqrt(u1)
    pq = ls.c[li] + ls.u[li] * (u1 - 0.5)[:, None] + ls.v[li] * (u2 - 0.5)[:, None]
    pt = ls.c[li] + ls.u[li] * (sq * (1.0 - u2))[:, None] + ls.v[li] * (sq * u2)[:, None]
    p = np.where((kind == 2)[:, None], pt, pq)
    dv = p - x
    d2q = (dv * dv).sum(1)
    tq = np.sqrt(d2q)
    with np.errstate(divide="ignore", invalid="ignore"):
        wq = dv / tq[:, None]
    omc, cd, D2, band = ls.cone_omc(li, x)
    D = np.sqrt(D2)
    a = u1 * omc
    cos_t = 1.0 - a
    sin2 = a * (2.0 - a)
    sin_t = np.sqrt(sin2)
    phi = 2.0 * np.pi * u2
    with np.errstate(divide="ignore", invalid="ignore"):
        wc = cd / D[:, None]
        sg = np.copysign(1.0, wc[:, 2])
        ia = -1.0 / (sg + wc[:, 2])
        b = wc[:, 0] * wc[:, 1] * ia
        t1 = np.column_stack([1.0 + sg * wc[:, 0] ** 2 * ia, sg * b, -sg * wc[:, 0]])
        t2 = np.column_stack([b, sg + wc[:, 1] ** 2 * ia, -wc[:, 1]])
        ws = t1 * (sin_t * np.cos(phi))[:, None] + t2 * (sin_t * np.sin(phi))[:, None] + wc * cos_t[:, None]
        Rl = ls.R[li]
        ts = (D2 - Rl * Rl) / (D * cos_t + np.sqrt(np.maximum(Rl * Rl - D2 * sin2, 0.0)))
    w = np.where(flat[:, None], wq, ws)
    t_light = np.where(flat, tq, ts)
    pdf_w, cos_l, _ = ls.pdf_w(li, x, np.nan_to_num(w), d2q)
    pdf_l = pmf * pdf_w
    tmax = t_light * (1.0 - SHADOW_EPS)
    valid = (pdf_l > 0) & (pdf_l < 3.0e38) & (tmax > 0) & np.all(np.isfinite(w), axis=1)
    w = np.where(valid[:, None], w, 0.0)
    cos_n = (n * w).sum(1)
    pb = np.maximum(cos_n, 0.0) / np.pi
    wl = np.where(valid, lr.light_weight(mode, np.where(valid, pdf_l, 1.0), pb), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(valid & (cos_n > 0), pb * wl / pdf_l, 0.0)
    return dict(valid=valid, light=li, w=w, t_light=np.where(valid, t_light, 0.0), tmax=np.where(valid, tmax, 0.0),
                pdf_l=np.where(valid, pdf_l, 0.0), pb=pb, wl=wl, cos_n=cos_n, cos_l=np.where(flat, cos_l, 1.0), f=f,
                margin_band=np.where(flat, np.inf, band), sel_band=np.zeros(len(li), bool), quad=flat, cluster=cl, P=P)


def hit_weight(ls: ClusteredLightSet, prim, x, w, d2, pb, mode, wrong=None):
    """mesh_light_replay.hit_weight with pL = P_c(x) pmf_in pdf_w, x the segment's origin."""
    li = ls.prim_light[prim]
    inset = li >= 0
    lj = np.where(inset, li, 0)
    if ls.n == 0:
        one = np.ones(len(prim))
        return one, one, np.full(len(prim), np.inf), np.zeros(len(prim))
    pdf_w, cos_l, band = ls.pdf_w(lj, x, w, d2)
    if wrong == "wb_power_pmf":
        pmf = ls.pmf[lj]
    else:
        pmf = cluster_prob(thresholds(ls.t, x), ls.cluster[lj]) * ls.inner[lj] * ls.env_factor()
    pl = np.where(inset, pmf * pdf_w, 0.0)
    has = pl > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == "nee":
            wb = np.zeros(len(prim))
        else:
            wb = np.where(pb > 0, 1.0 / (1.0 + (pl / np.where(pb > 0, pb, 1.0)) ** 2), 0.0)
    return np.where(has, wb, 1.0), np.where(inset, cos_l, 1.0), np.where(inset, band, np.inf), pl


def light_set(scene, tables) -> ClusteredLightSet:
    """The clustered light set of `scene` over the read-back `tables`."""
    return type("ClusteredLightSetBound", (ClusteredLightSet,), {"tables": tables})(scene, "all")


@contextlib.contextmanager
def clustered(tables, wrong=None):
    """Inside: mesh_light_replay's light set, sample_lights and hit_weight are the clustered ones over `tables`."""
    assert wrong is None or wrong in WRONG, wrong
    saved = (mlr.MeshLightSet, mlr.sample_lights, mlr.hit_weight)
    cls = type("ClusteredLightSetBound", (ClusteredLightSet,), {"tables": tables})
    mlr.MeshLightSet = cls
    mlr.sample_lights = lambda ls, x, n, keys, mode, wrong_=None: sample_lights(ls, x, n, keys, mode, wrong)
    mlr.hit_weight = lambda ls, prim, x, w, d2, pb, mode, wrong_=None: hit_weight(ls, prim, x, w, d2, pb, mode, wrong)
    try:
        yield
    finally:
        mlr.MeshLightSet, mlr.sample_lights, mlr.hit_weight = saved


def replay_case(c, mode, tables, samples=mlr.SAMPLES, wrong=None, **kw):
    """mesh_light_replay.replay_case under clustered selection over `tables`."""
    with clustered(tables, wrong):
        return mlr.replay_case(c, mode, samples=samples, **kw)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def near_far(W=96, H=64):
    """NEAR_FAR: lighting_replay's 20 x 20 ground quad and two emissive refined icosahedra (80 triangles each, equal power)
    20 ground-widths apart: one above the ground in front of the camera, one 400 away along +x; black sky.
    -> mesh_light_replay.case's dict."""
    from parallelraytracing_amd import scenes

    def fill(sc):
        e = sc.AddEmissive((8.0, 8.0, 8.0))
        ico = prt.Mesh(scenes.asset("icosahedron.ply")).refine(80)
        assert ico.n_triangles == 80
        v, nr, idx = ico.GetVertices(), ico.GetNormals(), ico.GetIndices()
        for tx in (0.0, 400.0):
            sc.AddMesh(prt.Mesh(vertices=(v * np.float32(0.4) + np.array([tx, 0.5, 0.0], np.float32)).astype(np.float32), normals=nr,
                                indices=idx), e)
    sc, cam = lr._ground_and(fill, (1.5, 1.5, 4.5), W, H, sky=(0.0, 0.0, 0.0))
    return dict(name="NEAR_FAR", scene=sc, cam=cam, W=W, H=H, depth=2, sampling=(0, 0, 0.0), use_bvh=True)


def ground_pixels(c, seed=mlr.SEED):
    """The pixels of case `c` whose primary ray hits analytic primitive 0, the ground (no jitter: the same for every sample)."""
    from util import orc
    osc = orc.OracleScene(c["scene"].desc())
    pix = np.arange(c["W"] * c["H"])
    verts, _, _, _ = lr.walk(c["scene"], osc, c["cam"], c["W"], c["H"], 1, seed, pix, np.zeros(len(pix), np.int64), c["sampling"],
                             c["use_bvh"], None)
    v = verts[0]
    return np.sort(v["path"][v["hit"]["prim"] == 0])


def luminance(v):
    return 0.2126 * v[..., 0] + 0.7152 * v[..., 1] + 0.0722 * v[..., 2]


def variance_ratio(y_power, y_clustered, groups=8):
    """y_* [n_pix, n_samples] luminance of the same pixels under the two selections.  -> (R, se): R = the ratio of the
    pixel-summed per-pixel sample variances (clustered / power) over all samples, se = the standard error of the mean of
    the `groups` per-group ratios (consecutive samples form a group)."""
    def var_sum(y):
        return float(y.var(axis=1, ddof=1).sum())
    R = var_sum(y_clustered) / var_sum(y_power)
    per = y_power.shape[1] // groups
    rs = np.array([var_sum(y_clustered[:, g * per:(g + 1) * per]) / var_sum(y_power[:, g * per:(g + 1) * per]) for g in range(groups)])
    return R, float(rs.std(ddof=1) / np.sqrt(groups)), rs
