"""numpy restatement of surface baking (include/prt.h "Surface baking"), written from the header text: coverage in
float64 on the UVs widened from fp32, everything after the barycentrics in float32 with every operation rounded once, the
RNG (pcg_hash, path_seed, Random, the rejection sampler of RandomUnitVector) in uint32 / float32.

  * surface(faces, W, H): owner, coverage, barycentrics, position and normal of every texel, and the counts.
  * rays(surf, sample, seed): origin, direction and advanced RNG state of one sample of every texel.
  * dilate(coverage, rgb, passes): the gutter fill.
  * the shapes the tests bake (square, cube with the PLY's overlapping UVs, cube with an atlas that leaves gutters), the
    map sizes, and the emitter of the form-factor test.
  * the shapes beyond toy maps (BIG_SHAPES: a grid whose vertices are texel centres, a 2,003-face soup, faces of magnitude
    2^20, near-collinear slivers, a 20 k-face scan and a placed copy under planar projections) with the maps they are baked
    on, and exact_owner: the owner in exact rational arithmetic.

No kernel code and no GPU is involved."""
from __future__ import annotations

import functools

import numpy as np

from util import prt

F = np.float32
NONE = 0xFFFFFFFF
SIZES = ((1, 1), (3, 5), (16, 16), (17, 33))   # (H, W): 1 x 1, 5 x 3, 16 x 16 and 33 x 17 maps
M32 = np.uint64(0xFFFFFFFF)


# ---- RNG (prt_device.h: pcg_hash, path_seed, rnd01, random_unit_vector) ----------------------------------------------------
def pcg_hash(v):
    v = np.asarray(v).astype(np.uint64) & M32
    state = (v * np.uint64(747796405) + np.uint64(2891336453)) & M32
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & M32
    return (((word >> np.uint64(22)) ^ word) & M32).astype(np.uint32)


def path_seed(pixel, sample, seed):
    pixel = np.asarray(pixel).astype(np.uint64)
    s = (np.uint64(int(sample) & 0xFFFFFFFF) * np.uint64(719393)) & M32
    k = np.uint64((int(seed) * 0x9E3779B9) & 0xFFFFFFFF)
    return pcg_hash(((pixel ^ s) + k) & M32)


def rnd01(state):
    """-> (the advanced states, u = (s >> 8) * 2^-24 in fp32)"""
    s = pcg_hash(state)
    return s, (s >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)


def random_unit_vector(state):
    """Rejection in [-1, 1]^3, draw order x, y, z; accepted when 1e-8f < |p|^2 <= 1; p / sqrt(|p|^2).  Vectorised: every
    state draws until its own point is accepted."""
    state = np.array(state, np.uint32)
    out = np.zeros((len(state), 3), F)
    todo = np.ones(len(state), bool)
    while todo.any():
        s = state[todo]
        s, ux = rnd01(s)
        s, uy = rnd01(s)
        s, uz = rnd01(s)
        x, y, z = F(-1.0) + F(2.0) * ux, F(-1.0) + F(2.0) * uy, F(-1.0) + F(2.0) * uz
        l2 = (x * x + y * y) + z * z
        ok = (F(1e-8) < l2) & (l2 <= F(1.0))
        state[todo] = s
        r = np.sqrt(l2[ok])
        idx = np.nonzero(todo)[0][ok]
        out[idx] = np.stack([x[ok] / r, y[ok] / r, z[ok] / r], 1)
        todo[idx] = False
    return state, out


def normalize3(v):
    """glm::normalize in fp32: v * (1 / sqrt((x*x + y*y) + z*z)), rows of an [n, 3] float32 array"""
    l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (v * (F(1.0) / np.sqrt(l2))[:, None]).astype(F)


def lambert_scatter(normal, state):
    """Material::Scatter of a Lambertian: dir = n + RandomUnitVector, n itself where every |component| < 1e-8, normalised."""
    state, u = random_unit_vector(state)
    d = (normal + u).astype(F)
    tiny = (np.abs(d).astype(np.float64) < 1e-8).all(axis=1)
    d[tiny] = normal[tiny]
    return state, normalize3(d)


# ---- transforms (prt_device.h: transform_point with Mat, transform_normal with Inv) ------------------------------------------
def dev12(m16):
    """Rows 0..2 of a column-major mat4 as the 12 floats the device keeps: m12[c * 3 + r] = m16[c * 4 + r]"""
    m16 = np.asarray(m16, F)
    return np.array([m16[c * 4 + r] for c in range(4) for r in range(3)], F)


def transform_point(m, p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(m[r] * x + m[3 + r] * y) + (m[6 + r] * z + m[9 + r] * F(1.0)) for r in range(3)], 1).astype(F)


def transform_normal(m, n):
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    return normalize3(np.stack([(m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z for r in range(3)], 1).astype(F))


# ---- 1. the surface of a texel --------------------------------------------------------------------------------------------
def mesh_faces(mesh, uvs=None):
    """(uv [F, 3, 2], position [F, 3, 3], normal [F, 3, 3]) of a prt.Mesh in face order; uvs: per vertex, default the mesh's own"""
    idx = mesh.GetIndices().astype(np.int64)
    uv = np.asarray(mesh.GetUVs() if uvs is None else uvs, F)
    return uv[idx], mesh.GetVertices().astype(F)[idx], mesh.GetNormals().astype(F)[idx]


def _edges(uv, px, py):
    """A2 of one face and E0, E1, E2 at the points, in double from the fp32 UVs, every operation rounded once"""
    (ax, ay), (bx, by), (cx, cy) = uv.astype(np.float64)
    A2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    E0 = (bx - px) * (cy - py) - (by - py) * (cx - px)
    E1 = (cx - px) * (ay - py) - (cy - py) * (ax - px)
    E2 = (ax - px) * (by - py) - (ay - py) * (bx - px)
    return A2, E0, E1, E2


def centres(W, H):
    """(px, py) of the W * H texels in map order, in double"""
    t = np.arange(W * H)
    return ((t % W).astype(np.float64) + 0.5) / float(W), 1.0 - ((t // W).astype(np.float64) + 0.5) / float(H)


def in_box(uv, px, py):
    """The centre lies in the face's closed UV box: double comparisons of the widened fp32 UVs with the centre"""
    x, y = uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)
    return (x.min() <= px) & (px <= x.max()) & (y.min() <= py) & (py <= y.max())


def covers(uv, px, py):
    """The coverage rule of one face at the points -> (bool per point, or None: the face is skipped; A2, E1, E2)"""
    with np.errstate(invalid="ignore", over="ignore"):
        A2, E0, E1, E2 = _edges(uv, px, py)
        if not np.isfinite(uv).all() or A2 == 0.0:
            return None, A2, E1, E2
        signs = ((E0 >= 0) & (E1 >= 0) & (E2 >= 0)) if A2 > 0 else ((E0 <= 0) & (E1 <= 0) & (E2 <= 0))
        return signs & in_box(uv, px, py), A2, E1, E2


def surface(faces, W, H, mat16=None, inv16=None):
    """faces = (uv, position, normal) as mesh_faces gives them; mat16 / inv16: a placed copy's column-major Mat and Inv.
    -> dict(owner [H, W] uint32, coverage [H, W] uint8, bary [H, W, 2], position, normal [H, W, 3], n_covered,
    n_degenerate, n_faces_skipped; coverers [H, W]: how many faces' rule covers the texel, face_texels [F]: how many texels
    each face's rule covers)."""
    uv, pos, nrm = (np.asarray(a, F) for a in faces)
    n = W * H
    px, py = centres(W, H)
    owner = np.full(n, NONE, np.uint32)
    b1, b2 = np.zeros(n, F), np.zeros(n, F)
    skipped = 0
    coverers, face_texels = np.zeros(n, np.int32), np.zeros(len(uv), np.int64)     # (of the rule alone: for the tests' conditions)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(len(uv)):
            cov, A2, E1, E2 = covers(uv[f], px, py)
            if cov is None:
                skipped += 1
                continue
            coverers += cov
            face_texels[f] = cov.sum()
            new = cov & (owner == NONE)          # faces in ascending order: the first to cover a texel is the lowest
            owner[new] = f
            b1[new] = (E1[new] / A2).astype(F)
            b2[new] = (E2[new] / A2).astype(F)
    own = owner != NONE
    fo = owner[own].astype(np.int64)
    w0 = (F(1.0) - b1[own] - b2[own])[:, None]
    c1, c2 = b1[own][:, None], b2[own][:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        p = ((w0 * pos[fo, 0] + c1 * pos[fo, 1]) + c2 * pos[fo, 2]).astype(F)
        ns = ((w0 * nrm[fo, 0] + c1 * nrm[fo, 1]) + c2 * nrm[fo, 2]).astype(F)
        l2 = (ns[:, 0] * ns[:, 0] + ns[:, 1] * ns[:, 1]) + ns[:, 2] * ns[:, 2]
        good = (l2 > 0) & (l2 < np.inf)
        nn = normalize3(ns)
        if mat16 is not None:
            p = transform_point(dev12(mat16), p)
            nn = transform_normal(dev12(inv16), nn)
    at = np.nonzero(own)[0]
    owner[at[~good]] = NONE
    position, normal, bary = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 2), F)
    position[at[good]] = p[good]
    normal[at[good]] = nn[good]
    bary[at[good], 0] = b1[own][good]
    bary[at[good], 1] = b2[own][good]
    return dict(owner=owner.reshape(H, W), coverage=(owner != NONE).astype(np.uint8).reshape(H, W), bary=bary.reshape(H, W, 2),
                position=position.reshape(H, W, 3), normal=normal.reshape(H, W, 3), n_covered=int(good.sum()),
                n_degenerate=int((~good).sum()), n_faces_skipped=skipped, coverers=coverers.reshape(H, W), face_texels=face_texels)


def interior(surf, margin=0.05):
    """[H, W] bool: covered texels whose three barycentrics are all >= margin (in fp32, w0 by the UV rule's line)"""
    b1, b2 = surf["bary"][..., 0], surf["bary"][..., 1]
    w0 = F(1.0) - b1 - b2
    return (surf["coverage"] != 0) & (np.minimum(np.minimum(w0, b1), b2) >= F(margin))


# ---- 2. the rays of a texel -----------------------------------------------------------------------------------------------
def rays(surf, sample, seed):
    """-> dict(o, d [H, W, 3], rng_state [H, W]) of sample `sample`: zero where uncovered"""
    H, W = surf["coverage"].shape
    cov = surf["coverage"].ravel() != 0
    t = np.nonzero(cov)[0]
    state = path_seed(t, sample, seed)
    nn = surf["normal"].reshape(-1, 3)[t]
    state, out_d = lambert_scatter(nn, state)
    o, d, s = np.zeros((H * W, 3), F), np.zeros((H * W, 3), F), np.zeros(H * W, np.uint32)
    o[t] = surf["position"].reshape(-1, 3)[t]
    d[t] = normalize3(out_d)
    s[t] = state
    return dict(o=o.reshape(H, W, 3), d=d.reshape(H, W, 3), rng_state=s.reshape(H, W))


# ---- 3. gutter fill -------------------------------------------------------------------------------------------------------
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def dilate(coverage, rgb, passes):
    """-> (coverage, rgb, n_filled) after `passes` double-buffered passes"""
    cov, val = np.array(coverage, np.uint8), np.array(rgb, F)
    H, W = cov.shape
    filled = 0
    for _ in range(passes):
        ncov, nval = cov.copy(), val.copy()
        for i in range(H):
            for j in range(W):
                if cov[i, j]:
                    continue
                acc, cnt = np.zeros(3, F), 0
                for di, dj in NEIGHBOURS:
                    ii, jj = i + di, j + dj
                    if 0 <= ii < H and 0 <= jj < W and cov[ii, jj]:
                        acc = (acc + val[ii, jj]).astype(F)
                        cnt += 1
                if cnt:
                    nval[i, j] = acc / F(cnt)
                    ncov[i, j] = 2
                    filled += 1
        cov, val = ncov, nval
    return cov, val, filled


# ---- the shapes the tests bake ----------------------------------------------------------------------------------------------
def square_mesh(size=2.0, y=0.0):
    """Two triangles over [-size/2, size/2]^2 in the plane y, normal +y, UVs the unit square; the diagonal runs from
    uv (0, 0) to (1, 1) and is shared by both faces."""
    h = size / 2.0
    v = np.array([[-h, y, h], [h, y, h], [h, y, -h], [-h, y, -h]], F)       # uv (0,0) (1,0) (1,1) (0,1)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)
    n = np.tile(np.array([[0.0, 1.0, 0.0]], F), (4, 1))
    return prt.Mesh(vertices=v, normals=n, indices=np.array([[0, 1, 2], [0, 2, 3]], np.uint32), uvs=uv)


def cube_mesh():
    return prt.Mesh(prt.scenes.asset("cube_uv.ply"))


def cube_atlas_uvs(mesh):
    """A lightmap layout for cube_uv.ply: the quad of side k (4 vertices, the PLY's own unit-square UVs) goes into cell
    (k % 3, k // 3) of a 3 x 2 grid, shrunk to half the cell: gutters several texels wide between the charts and along the border."""
    uv = mesh.GetUVs().astype(np.float64)
    out = np.empty_like(uv)
    for k in range(6):
        cx, cy = k % 3, k // 3
        sl = slice(4 * k, 4 * k + 4)
        out[sl, 0] = (cx + 0.25 + 0.5 * uv[sl, 0]) / 3.0
        out[sl, 1] = (cy + 0.25 + 0.5 * uv[sl, 1]) / 2.0
    return out.astype(F)


COPY_SRT = (1.7, (20.0, 35.0, -10.0), (0.4, 1.1, -0.3))   # the placed copy: scale 1.7, a rotation, an offset
SHAPES = ("square", "cube", "cube_atlas", "copy", "copy_atlas")


# ---- shapes beyond toy maps: many faces, maps of several compaction trips (1024 texels each) ----------------------------------
BIG_SIZES = ((80, 96), (33, 129), (128, 128))       # (H, W): 7.5 trips, 4.2 trips, 16 whole trips
STRIPS = ((1, 2049), (2049, 1))
DYADIC = ((16, 16), (32, 32), (16, 64))             # the grid's rule is exact on these
SLIVER_SIZES = ((16, 16), (17, 17), (12, 12))
BIG_SHAPES = ("grid", "soup", "huge", "slivers", "bunny", "ico_copy")
SHAPE_SIZES = dict(grid=BIG_SIZES + STRIPS + DYADIC, soup=BIG_SIZES + STRIPS, huge=BIG_SIZES, slivers=BIG_SIZES + SLIVER_SIZES,
                   bunny=BIG_SIZES, ico_copy=BIG_SIZES)
SOUP_FACES = 2003
SOUP_TWINS = (700, 1500)                            # two faces of the soup with identical UVs
SLIVER_0 = ((0.0, 0.0), (0.5, 0.5), (1e-30, 2e-30))   # rounded E0 = E1 = E2 = 0 at every point of the diagonal of the map


def soup_mesh(uv, seed):
    """Three vertices of their own per face [F, 3, 2]: small random triangles in [-1, 1]^3, random unit vertex normals"""
    rng = np.random.default_rng(seed)
    n = len(uv)
    pos = (rng.uniform(-1.0, 1.0, (n, 1, 3)) + rng.uniform(-0.1, 0.1, (n, 3, 3))).astype(F)
    nrm = rng.normal(size=(n, 3, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(F)
    return prt.Mesh(vertices=pos.reshape(-1, 3), normals=nrm.reshape(-1, 3), indices=np.arange(3 * n, dtype=np.uint32).reshape(n, 3),
                    uvs=np.asarray(uv, F).reshape(-1, 2))


def grid_mesh():
    """An 8 x 8 vertex grid, 98 faces: UV vertices at (4k + 1) / 32, texel centres of a 16-wide map; the diagonal alternates
    per cell; about a third of the faces are wound clockwise.  Positions and normals are the square's."""
    rng = np.random.default_rng(21)
    k = (4.0 * np.arange(8) + 1.0) / 32.0
    uv = np.array([[k[c], k[r]] for r in range(8) for c in range(8)], F)
    idx = []
    for r in range(7):
        for c in range(7):
            v00, v10, v01, v11 = r * 8 + c, r * 8 + c + 1, (r + 1) * 8 + c, (r + 1) * 8 + c + 1
            idx += [[v00, v10, v11], [v00, v11, v01]] if (r + c) % 2 == 0 else [[v00, v10, v01], [v10, v11, v01]]
    idx = np.array(idx, np.uint32)
    flip = rng.random(len(idx)) < 1.0 / 3.0
    idx[flip] = idx[flip][:, [0, 2, 1]]
    pos = np.stack([2.0 * uv[:, 0] - 1.0, np.zeros(64), 1.0 - 2.0 * uv[:, 1]], 1).astype(F)
    return prt.Mesh(vertices=pos, normals=np.tile(np.array([[0.0, 1.0, 0.0]], F), (64, 1)), indices=idx, uvs=uv)


def soup_uvs():
    """SOUP_FACES random triangles: centres uniform in [-0.1, 1.1]^2, vertices within +-size of the centre, size log-uniform
    in 2e-3 .. 0.12 (from well below a texel of every map used to a dozen texels across; the upper end is what brings the
    covered share of 2,003 faces above 30 % on every map, the strips included), random winding, one pair of identical faces"""
    rng = np.random.default_rng(31)
    n = SOUP_FACES
    centre = rng.uniform(-0.1, 1.1, (n, 1, 2))
    size = np.exp(rng.uniform(np.log(2e-3), np.log(0.12), (n, 1, 1)))
    uv = (centre + size * rng.uniform(-1.0, 1.0, (n, 3, 2))).astype(F)
    uv[SOUP_TWINS[1]] = uv[SOUP_TWINS[0]]
    return uv


def huge_uvs():
    """Three small faces first, which keep their texels; then a face over the whole map, one of magnitude 2^20 over it too,
    and one of magnitude 2^20 wholly outside"""
    B = 2.0 ** 20
    return np.array([[[0.1, 0.1], [0.4, 0.15], [0.2, 0.45]], [[0.9, 0.9], [0.6, 0.8], [0.85, 0.55]], [[0.3, 0.7], [0.5, 0.6], [0.45, 0.95]],
                     [[-1, -1], [3, -1], [-1, 3]], [[-B, -B], [B, -B], [0, B]], [[B, B], [B / 2, B], [B, B / 2]]], F)


def sliver_uvs():
    """A few dozen near-collinear faces with area (A2 != 0): SLIVER_0; along diagonals and anti-diagonals, short, so that
    their lines cross texel centres far outside their boxes; along axis-aligned lines, c one fp32 ulp off the line a-b;
    along arbitrary directions, c the fp32 rounding of a point of a-b, or an ulp from it; third vertices down to 1e-30 and
    to subnormals."""
    rng = np.random.default_rng(41)
    up = lambda v: np.nextafter(F(v), F(np.inf))
    f = [SLIVER_0]
    for tiny in (1e-30, 3e-39, 1.4e-45):                 # (the last two are subnormal in fp32)
        f.append(((0.0, 0.0), (0.25, 0.25), (tiny, 2 * tiny)))
        f.append(((0.0, 0.0), (2 * tiny, tiny), (0.3125, 0.3125)))
        f.append(((0.0, 0.0), (0.375, 0.0), (0.1, tiny)))            # along v = 0
        f.append(((0.0, 0.0), (tiny, 0.2), (0.0, 0.625)))            # along u = 0
    for lo, hi in ((0.125, 0.375), (0.53125, 0.59375), (0.25, 0.28125)):
        f.append(((lo, lo), (hi, hi), (up(lo), lo)))                                  # diagonal, an ulp off at a
        f.append(((lo, 1.0 - lo), (hi, 1.0 - hi), (up((lo + hi) / 2), 1.0 - (lo + hi) / 2)))      # anti-diagonal
    for v in (0.3, 0.53125, 0.96875):
        f.append(((0.1, v), (0.9, v), (0.5, up(v))))                                  # horizontal, c an ulp above
        f.append(((v, 0.2), (up(v), 0.55), (v, 0.7)))                                 # vertical, b an ulp right
    while len(f) < 40:                                   # arbitrary directions
        a, b = rng.uniform(0.0, 1.0, 2).astype(F), rng.uniform(0.0, 1.0, 2).astype(F)
        s = rng.uniform(0.2, 0.8)
        c = (a.astype(np.float64) * (1.0 - s) + b.astype(np.float64) * s).astype(F)
        if len(f) % 2:
            c[0] = up(c[0])
        f.append((a, b, c))
    return np.array(f, F)


@functools.lru_cache(maxsize=None)
def shape(name):
    """dict(mesh, uvs (per call, or None: the mesh's own), placed) of a shape; computed once, shared"""
    if name == "square":
        return dict(mesh=square_mesh(), uvs=None, placed=False)
    if name == "grid":
        return dict(mesh=grid_mesh(), uvs=None, placed=False)
    if name in ("soup", "huge", "slivers"):
        uv, seed = dict(soup=(soup_uvs, 32), huge=(huge_uvs, 33), slivers=(sliver_uvs, 34))[name]
        return dict(mesh=soup_mesh(uv(), seed), uvs=None, placed=False)
    if name in ("bunny", "ico_copy"):
        m = prt.scenes.refined("bunny.ply", 20_000) if name == "bunny" else prt.scenes.refined("icosahedron.ply", 2000)
        return dict(mesh=m, uvs=prt.scenes.planar_uvs(m, axes=(0, 1)), placed=name == "ico_copy")
    m = cube_mesh()
    return dict(mesh=m, uvs=cube_atlas_uvs(m) if name.endswith("atlas") else None, placed=name.startswith("copy"))


def exact_owner(uv, W, H):
    """The lowest face whose closed triangle holds the texel centre, in exact rational arithmetic -> (owner [H, W] uint32,
    number of exact coverers [H, W]).  fractions.Fraction turns the fp32 UVs and the centres (2j + 1) / (2W),
    1 - (2i + 1) / (2H) into integers over one common denominator; the edge functions are then integer arithmetic."""
    from fractions import Fraction
    from math import lcm
    q = [[Fraction(float(v)) for v in face.ravel()] for face in np.asarray(uv, F)]
    cx = [Fraction(2 * j + 1, 2 * W) for j in range(W)]
    cy = [1 - Fraction(2 * i + 1, 2 * H) for i in range(H)]
    D = lcm(*(v.denominator for face in q for v in face), *(v.denominator for v in cx + cy))
    whole = lambda v: int(v * D)
    assert all((v * D).denominator == 1 for face in q for v in face)
    px = np.tile(np.array([whole(v) for v in cx], object), H)
    py = np.repeat(np.array([whole(v) for v in cy], object), W)
    owner = np.full(W * H, NONE, np.uint32)
    count = np.zeros(W * H, np.int64)
    for f, face in enumerate(q):
        ax, ay, bx, by, cx_, cy_ = (whole(v) for v in face)
        A2 = (bx - ax) * (cy_ - ay) - (by - ay) * (cx_ - ax)
        if A2 == 0:
            continue
        s = 1 if A2 > 0 else -1
        E0 = ((bx - px) * (cy_ - py) - (by - py) * (cx_ - px)) * s
        E1 = ((cx_ - px) * (ay - py) - (cy_ - py) * (ax - px)) * s
        E2 = ((ax - px) * (by - py) - (ay - py) * (bx - px)) * s
        cov = ((E0 >= 0) & (E1 >= 0) & (E2 >= 0)).astype(bool)
        owner[cov & (owner == NONE)] = f
        count += cov
    return owner.reshape(H, W), count.reshape(H, W)


@functools.lru_cache(maxsize=None)
def reference(name, H, W):
    """The replay's surface of a shape on an H x W map; computed once, shared, never written to"""
    s = shape(name)
    mat = inv = None
    if s["placed"]:
        mat, inv = prt.make_transform((COPY_SRT[0],) * 3, COPY_SRT[1], COPY_SRT[2])
    surf = surface(mesh_faces(s["mesh"], s["uvs"]), W, H, mat, inv)
    for a in surf.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return surf


# ---- the form-factor case: the square under an emissive quad ----------------------------------------------------------------
FF_MAP = (8, 8)
FF_SAMPLES = 256
FF_EMISSION = (3.0, 2.0, 1.0)
FF_QUAD = dict(width=3.0, height=3.0, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 1.2, 0.0))   # faces down, above the square


def ff_scene():
    """The 2 x 2 square at y = 0 under a black sky and the emissive quad; -> (scene, the quad's column-major Mat)"""
    sc = prt.Scene(preset=None, sky=(0.0, 0.0, 0.0))
    body = sc.AddLambertian((0.5, 0.5, 0.5))
    light = sc.AddEmissive(FF_EMISSION)
    sc.AddQuad(FF_QUAD["width"], FF_QUAD["height"], light, euler_deg=FF_QUAD["euler_deg"], translation=FF_QUAD["translation"])
    sc.AddMesh(square_mesh(), body)
    return sc, np.array(sc.primitives[0].mat[:], F)
