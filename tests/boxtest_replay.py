"""fp32-faithful replay of the 8-wide walk's box test (T8_BOXTEST in csrc/prt_kernels.hip) along the winner's path.

For a ray whose closest hit (the oracle's linear scan) is triangle p, the walk finds p only if every child box on the way
from the root to the leaf slot that holds p passes `tn <= tf` with the kernel's own fp32 expressions: the per-ray pad, the
clamped reciprocals, anx / afx, the cell products Ax, the node constants Bnx / Bfx, one fma per plane, and
tlimit = limit_from_d2(d2 of the winner, pad), the tightest bound the walk can hold while p has not been tested.

Every operation is evaluated as IEEE binary32: numpy float32 for +, *, sqrt, and fma(a, b, c) as the correctly rounded
exact a * b + c (float64 holds the product exactly and adds with one rounding; a result that sits on a rounding tie of
binary32, where the second rounding could go the other way, and every subnormal result are recomputed with
fractions.Fraction).  fmax / fmin follow IEEE fmaxf / fminf (the operand that is not NaN wins).  v_rcp_f32 is good to one
ulp: each reciprocal is taken as the correctly rounded one and its two binary32 neighbours, and the condition must hold
for every combination (the axes are independent: the largest near value and the smallest far value per axis decide)."""
import os
import re
from fractions import Fraction

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD_COEFF = F(2.0 ** -18)


def kernel_dir_min():
    """PRT_DIR_MIN of csrc/prt_kernels.h: the clamp the kernels are compiled with."""
    with open(os.path.join(ROOT, "parallelraytracing_amd", "csrc", "prt_kernels.h")) as f:
        m = re.search(r"#define\s+PRT_DIR_MIN\s+([0-9.eE+-]+)f", f.read())
    return F(float(m.group(1)))


def _round_fraction(x):
    """Fraction -> binary32, round to nearest even."""
    if x == 0:
        return F(0.0)
    f = F(float(x))  # within one ulp of the answer; pick among it and its neighbours exactly
    if not np.isfinite(f):
        return f
    cands = [np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf))]
    best = None
    for c in cands:
        if not np.isfinite(c):
            continue
        e = abs(Fraction(float(c)) - x)
        even = (int(np.array(c, F).view(np.uint32)) & 1) == 0
        if best is None or e < best[0] or (e == best[0] and even):
            best = (e, c)
    return best[1]


def fma32(a, b, c):
    """Correctly rounded a * b + c in binary32, elementwise."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)  # the product is exact, one rounding here
        r = s.astype(F)
    bits = s.view(np.uint64) if s.flags.c_contiguous else np.ascontiguousarray(s).view(np.uint64)
    tie = (bits & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)
    sub = (np.abs(s) < 2.0 ** -126) & (s != 0)
    redo = (tie | sub) & np.isfinite(s)
    r = r.copy()
    for i in zip(*np.nonzero(redo)):
        r[i] = _round_fraction(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return r


def limit_from_d2(d2, pad):
    d2, pad = np.asarray(d2, F), np.asarray(pad, F)
    with np.errstate(all="ignore"):
        return np.where(d2 < F(3.0e38), np.sqrt(d2) * F(1.0000153) + F(4.0) * pad, F(3.4e38)).astype(F)


def ray_pad(o, extent, coeff=PAD_COEFF):
    o = np.asarray(o, F)
    return (coeff * (((np.abs(o[..., 0]) + np.abs(o[..., 1])) + np.abs(o[..., 2])) + F(extent))).astype(F)


def normalize3(d):
    d = np.asarray(d, F)
    dot = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(F)
    with np.errstate(all="ignore"):
        return (d * (F(1.0) / np.sqrt(dot))[..., None]).astype(F)


def reciprocals(ld, dir_min):
    """[3 variants, n, 3]: the correctly rounded reciprocal of the clamped component and its two neighbours."""
    ld = np.asarray(ld, F)
    c = np.where(np.abs(ld) < dir_min, np.copysign(dir_min, ld), ld).astype(F)
    with np.errstate(all="ignore"):
        ix = (F(1.0) / c).astype(F)
    return np.stack([np.nextafter(ix, F(-np.inf)), ix, np.nextafter(ix, F(np.inf))])


def paths_to_slots(n8):
    """leaf slot -> [(node, child), ...] from the root's children down to the child that holds the slot."""
    nodes = len(n8)
    meta = np.stack([(n8[:, 6 + (i >> 2)] >> (8 * (i & 3))) & 0xFF for i in range(8)], axis=1).astype(np.int64)
    imask = (n8[:, 3] >> 24).astype(np.int64)
    parent = {}
    leaf = {}
    for n in range(nodes):
        rank = 0
        for i in range(8):
            m = int(meta[n, i])
            if m == 0:
                continue
            if (imask[n] >> i) & 1:
                parent[int(n8[n, 4]) + rank] = (n, i)
                rank += 1
            else:
                first = int(n8[n, 5]) + (m & 31)
                for t in range(bin(m >> 5).count("1")):
                    leaf[first + t] = (n, i)
    paths = {}
    for slot, (n, i) in leaf.items():
        p = [(n, i)]
        while n != 0:
            n, i = parent[n]
            p.append((n, i))
        paths[slot] = p[::-1]
    return paths


def boxtest_margin(n8, steps, ray, o, d, d2, extent, dir_min):
    """For the (node, child) pairs `steps` tested with rays o[ray], d[ray] whose winner lies at d2[ray]: (tn, tf), the
    largest tn and the smallest tf over the reciprocal variants, fp32.  The walk keeps the child iff tn <= tf."""
    o, d = np.asarray(o, F)[ray], np.asarray(d, F)[ray]
    node, child = steps[:, 0], steps[:, 1]
    pad = ray_pad(o, extent)
    ld = normalize3(d)
    tlimit = limit_from_d2(np.asarray(d2, F)[ray], pad)
    p = n8[node, 0:3].copy().view(F)                                         # [m, 3]
    eb = np.stack([(n8[node, 3] >> (8 * a)) & 0xFF for a in range(3)], axis=1).astype(np.uint32)
    cell = (eb << np.uint32(23)).view(F)                                      # 2^(e - 127); e = 0 -> 0.0
    w = n8[node]
    sh = (8 * (child & 3)).astype(np.uint32)
    hi_half = child >> 2

    def plane(word):  # byte `child` of the 8 bytes in words word, word + 1
        return ((w[np.arange(len(node)), word + hi_half] >> sh) & 0xFF).astype(F)
    qlo = np.stack([plane(8), plane(10), plane(12)], axis=1)
    qhi = np.stack([plane(14), plane(16), plane(18)], axis=1)
    tn_worst = np.full(len(node), F(0.0))
    tf_worst = tlimit.copy()
    with np.errstate(all="ignore"):
        for ix in reciprocals(ld, dir_min):
            neg = ix < 0
            an = (np.where(neg, o - pad[:, None], o + pad[:, None]).astype(F) * ix).astype(F)
            af = (np.where(neg, o + pad[:, None], o - pad[:, None]).astype(F) * ix).astype(F)
            A = (cell * ix).astype(F)
            Bn = fma32(p, ix, -an)
            Bf = fma32(p, ix, -af)
            tnq = fma32(np.where(neg, qhi, qlo), A, Bn)
            tfq = fma32(np.where(neg, qlo, qhi), A, Bf)
            tn = np.fmax(np.fmax(tnq[:, 0], tnq[:, 1]), np.fmax(tnq[:, 2], F(0.0)))
            tf = np.fmin(np.fmin(tfq[:, 0], tfq[:, 1]), np.fmin(tfq[:, 2], tlimit))
            # `tn <= tf` is false if either is NaN: a NaN that survives fmax / fmin must count as a failure
            tn_worst = np.where(np.isnan(tn) | np.isnan(tn_worst), F(np.nan), np.maximum(tn_worst, tn))
            tf_worst = np.where(np.isnan(tf) | np.isnan(tf_worst), F(np.nan), np.minimum(tf_worst, tf))
    return tn_worst, tf_worst


def culled_winners(n8, tris, o, d, want, extent, dir_min):
    """Indices of the rays whose oracle winner the box tests would cut off, with the first failing (node, child, tn, tf)."""
    prim_of_slot = tris[:, 3].view(np.uint32)
    slot_of_prim = {int(p): s for s, p in enumerate(prim_of_slot)}
    paths = paths_to_slots(n8)
    rays, steps = [], []
    for k in np.nonzero(want["prim"] >= 0)[0]:
        for st in paths[slot_of_prim[int(want["prim"][k])]]:
            rays.append(k)
            steps.append(st)
    if not rays:
        return [], 0
    rays, steps = np.array(rays), np.array(steps, np.int64)
    tn, tf = boxtest_margin(n8, steps, rays, o, d, want["d2"], extent, dir_min)
    bad = ~(tn <= tf)
    out = {}
    for j in np.nonzero(bad)[0]:
        out.setdefault(int(rays[j]), (int(steps[j, 0]), int(steps[j, 1]), float(tn[j]), float(tf[j])))
    return sorted(out.items()), len(rays)


# ---- the walk over the analytic primitives' world boxes (scan_analytic<ABVH> in csrc/prt_kernels.hip) ------------------
def prim_world_boxes(scene):
    """build_prim_bvh / prim_world_box of csrc/prt_scene.cpp restated: per primitive the padded fp32 world box, and the
    scene's extent and abvh_q as the walk gets them.  -> (mn [n, 3], mx [n, 3], extent, q [3]), or None where the library
    builds no tree over the primitives (16 or fewer, or a transform outside the similarity check's bounds)."""
    prims = scene.primitives
    if len(prims) <= 16:
        return None
    mn, mx = np.zeros((len(prims), 3), F), np.zeros((len(prims), 3), F)
    quad_pad = [0.0, 0.0, 0.0]
    for i, p in enumerate(prims):
        M = np.array(p.mat[:], F)
        g = [[sum(float(M[4 * a + k]) * float(M[4 * b + k]) for k in range(3)) for b in range(3)] for a in range(3)]
        s2 = g[0][0]
        if not (s2 > 1e-20 and np.isfinite(s2)) or any(abs(g[a][b] - (s2 if a == b else 0.0)) > 1e-4 * s2 for a in range(3) for b in range(3)):
            return None
        p0, p1 = F(p.shape_param[0]), F(p.shape_param[1])
        if p.shape_type == 0:  # sphere
            R = abs(float(p0)) * np.sqrt(s2)
            lo = np.array([F(float(M[12 + a]) - R) for a in range(3)], F)
            hi = np.array([F(float(M[12 + a]) + R) for a in range(3)], F)
            if R > 0.0:
                q, c1 = 1e-6 / R, sum(abs(float(M[12 + a])) for a in range(3))
                quad_pad = [max(quad_pad[0], q), max(quad_pad[1], 2.0 * q * c1), max(quad_pad[2], q * c1 * c1)]
        else:                  # quad in the local plane y = 0
            lo, hi = np.full(3, np.finfo(F).max, F), np.full(3, -np.finfo(F).max, F)
            for corner in range(4):
                lx = F(0.5 if corner & 1 else -0.5) * p0
                lz = F(0.5 if corner & 2 else -0.5) * p1
                for a in range(3):
                    wv = F(F(F(M[a] * lx) + F(M[4 + a] * F(0.0))) + F(F(M[8 + a] * lz) + M[12 + a]))
                    lo[a], hi[a] = min(lo[a], wv), max(hi[a], wv)
        mag = F(max(np.abs(lo).max(), np.abs(hi).max()))
        slack = F(F(F(1e-5) * F(mag + F(F(np.sqrt(s2)) * F(abs(p0) + abs(p1))))) + F(1e-30))
        mn[i], mx[i] = (lo - slack).astype(F), (hi + slack).astype(F)
    extent = F(max(np.abs(mn).max(), np.abs(mx).max()))
    for m, _ in scene.meshes:
        extent = max(extent, F(np.abs(m.GetVertices()).max()))
    return mn, mx, F(extent), np.array([F(v * 1.0000002) for v in quad_pad], F)


def analytic_slab_culled(scene, o, d, want, dir_min):
    """ABVH_CHILD's slab test in binary32 for every ray whose oracle winner is an analytic primitive, against that
    primitive's own world box and against the root (the union of all boxes; every node in between contains the first
    and lies inside the second): the rays for which `tn <= tf * 1.0000005f` fails, and the number of tests replayed."""
    boxes = prim_world_boxes(scene)
    assert boxes is not None
    mn, mx, extent, q = boxes
    k = np.nonzero((want["prim"] >= 0) & (want["prim"] < len(scene.primitives)))[0]
    oo, dd = np.asarray(o, F)[k], np.asarray(d, F)[k]
    ld = normalize3(dd)
    with np.errstate(all="ignore"):
        A1 = ((np.abs(oo[:, 0]) + np.abs(oo[:, 1])) + np.abs(oo[:, 2])).astype(F)
        pad = (PAD_COEFF * (A1 + extent) + ((q[0] * A1 + q[1]) * A1 + q[2])).astype(F)
        c = np.where(np.abs(ld) < dir_min, np.copysign(dir_min, ld), ld).astype(F)
        ix = (F(1.0) / c).astype(F)                                     # (an IEEE division in this walk)
        a_, b_ = ((oo + pad[:, None]) * ix).astype(F), ((oo - pad[:, None]) * ix).astype(F)
        tlimit = limit_from_d2(want["d2"][k], pad)
        bad = np.zeros(len(k), bool)
        for lo, hi in ((mn[want["prim"][k]], mx[want["prim"][k]]),
                       (np.broadcast_to(mn.min(axis=0), oo.shape), np.broadcast_to(mx.max(axis=0), oo.shape))):
            t0, t1 = fma32(lo, ix, -a_), fma32(hi, ix, -b_)
            near, far = np.fmin(t0, t1), np.fmax(t0, t1)
            tn = np.fmax(np.fmax(near[:, 0], near[:, 1]), np.fmax(near[:, 2], F(0.0)))
            tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), np.fmin(far[:, 2], tlimit))
            bad |= ~(tn <= (tf * F(1.0000005)).astype(F))
    return k[bad], 2 * len(k)
