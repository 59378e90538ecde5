"""numpy-float32 restatement of image textures (include/prt.h "Image textures"): the UV of a hit, the lookup, and a path
walker that puts the looked-up colour where the material's rgb stood as albedo.

Everything the kernels compute for a texture is a handful of fp32 operations in a written order, built without contraction,
so this module restates them operation for operation in numpy float32 (one rounding per operation, no FMA) and expects the
device to agree BIT FOR BIT:

  * Triangle::Intersect in glm's operation order, as oracle/prt_oracle.cpp has it (S, E1, E2, S1, S2, divisor, t, b1, b2, the
    position), with the local ray of a placed copy (TransformPoint(Inv, o), TransformNormal(Mat, d)); Quad::Intersect's local
    point; the UV rules; wrap, nearest and bilinear lookup.
  * hit_uv() is trusted only through its gate (tests/test_texture_replay.py): on every hit of every test scene the position it
    restates equals OracleScene.closest_hit's position bit for bit.  A restatement that does not is wrong; there is no
    tolerance anywhere in this file.
  * walk() is lighting_replay.walk (same signature, same record) with the looked-up colour as attenuation and `albedo` of
    every vertex whose material is textured; with monkeypatch.setattr(<replay module>, "walk", texture_replay.walk) the
    float64 replays of the lighting modes replay textured frames with their own tolerances.

No kernel code and no GPU is involved."""
from __future__ import annotations

import numpy as np

import lighting_replay as lr
from util import orc, prt

capi = prt.capi
F = np.float32
NONE = capi.TEXTURE_NONE


# ---- glm-order fp32 helpers (rows of [n, 3] float32 arrays) ------------------------------------------------------------------
def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2], x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0],
                     x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], axis=1)


def normalize(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (v * (F(1.0) / np.sqrt(dot(v, v)))[:, None]).astype(F)


def transform_point(m, p):
    """TransformPoint with glm's mat4 * vec4 grouping; m: 16 floats, column-major."""
    m = np.asarray(m, F)
    return np.stack([(m[r] * p[:, 0] + m[4 + r] * p[:, 1]) + (m[8 + r] * p[:, 2] + m[12 + r] * F(1.0)) for r in range(3)], axis=1)


def transform_normal(m, n):
    """TransformNormal: normalize(mat3(transpose(M)) * n)."""
    m = np.asarray(m, F)
    return normalize(np.stack([m[4 * r] * n[:, 0] + m[4 * r + 1] * n[:, 1] + m[4 * r + 2] * n[:, 2] for r in range(3)], axis=1))


def triangle_intersect(P, o, d):
    """Triangle::Intersect for rays (o, d) against their own triangles P [n, 3, 3] -> (position, b1, b2), all float32."""
    P0, P1, P2 = P[:, 0], P[:, 1], P[:, 2]
    S = o - P0
    E1 = P1 - P0
    E2 = P2 - P0
    S1 = cross(d, E2)
    S2 = cross(S, E1)
    with np.errstate(divide="ignore", invalid="ignore"):
        divisor = dot(S1, E1)
        b1 = dot(S1, S) / divisor
        b2 = dot(S2, d) / divisor
    w0 = F(1.0) - b1 - b2
    pos = w0[:, None] * P0 + b1[:, None] * P1 + b2[:, None] * P2
    return pos.astype(F), b1.astype(F), b2.astype(F)


# ---- the lookup --------------------------------------------------------------------------------------------------------------
def wrap(u, clamp):
    u = np.asarray(u, F)
    return np.minimum(np.maximum(u, F(0.0)), F(1.0)) if clamp else (u - np.floor(u)).astype(F)


def wrap_index(k, N, clamp):
    return np.minimum(np.maximum(k, 0), N - 1) if clamp else ((k % N) + N) % N


def lookup(img, filt, wrp, u, v):
    """Texel colour [n, 3] float32 of (u, v) in img [H, W, 3] (row 0 = top; v = 0 is the bottom row)."""
    img = np.asarray(img, F)
    H, W = img.shape[:2]
    a, b = wrap(u, wrp), wrap(v, wrp)
    X = a * F(W)
    Y = (F(1.0) - b) * F(H)
    if filt == 0:
        j = np.minimum(W - 1, np.floor(X).astype(np.int64))
        i = np.minimum(H - 1, np.floor(Y).astype(np.int64))
        return img[i, j]
    x, y = X - F(0.5), Y - F(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0).astype(F), (y - y0).astype(F)
    kx, ky = x0.astype(np.int64), y0.astype(np.int64)
    j0, j1 = wrap_index(kx, W, wrp), wrap_index(kx + 1, W, wrp)
    i0, i1 = wrap_index(ky, H, wrp), wrap_index(ky + 1, H, wrp)
    gx, gy = (F(1.0) - fx)[:, None], (F(1.0) - fy)[:, None]
    fx, fy = fx[:, None], fy[:, None]
    return ((img[i0, j0] * gx + img[i0, j1] * fx) * gy + (img[i1, j0] * gx + img[i1, j1] * fx) * fy).astype(F)


# ---- a scene's geometry as the UV rule needs it ------------------------------------------------------------------------------
class TexScene:
    """Primitive index -> what it is (analytic / face of a world-space mesh / face of a placed copy), the faces' vertices and
    UVs in index order, the textures and the texture of every material, all from the Python description."""

    def __init__(self, scene):
        self.scene = scene
        self.n_prims = len(scene.primitives)
        P, UV = [np.zeros((0, 3, 3), F)], [np.zeros((0, 3, 2), F)]
        for m, _ in scene.meshes:
            idx = m.GetIndices().astype(np.int64)
            uv = m.GetUVs()
            P.append(m.GetVertices()[idx])
            UV.append(np.zeros((len(idx), 3, 2), F) if uv is None else uv[idx])
        self.wP, self.wUV = np.concatenate(P).astype(F), np.concatenate(UV).astype(F)
        self.n_world = len(self.wP)
        self.mP, self.mUV = [], []
        for m in scene.instanced_meshes:
            idx = m.GetIndices().astype(np.int64)
            uv = m.GetUVs()
            self.mP.append(m.GetVertices()[idx].astype(F))
            self.mUV.append(np.zeros((len(idx), 3, 2), F) if uv is None else uv[idx].astype(F))
        self.inst = []   # (first primitive, triangles, mesh, mat, inv)
        base = self.n_prims + self.n_world
        for it in scene.instances:
            nt = len(self.mP[it.mesh])
            self.inst.append((base, nt, it.mesh, np.array(it.mat[:], F), np.array(it.inv[:], F)))
            base += nt
        self.mat_tex = np.array([scene.material_texture.get(m, NONE) for m in range(len(scene.materials))], np.int64)
        self.mat_rgb = np.array([list(m.rgb) for m in scene.materials], F).reshape(-1, 3)

    def hit_uv(self, o, d, hits):
        """(uv [n, 2], restated position [n, 3]) of closest-hit records `hits` of rays (o, d); float32.  Misses and spheres:
        uv 0 and the record's own position (nothing is restated for them)."""
        o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
        n = len(o)
        uv = np.zeros((n, 2), F)
        pos = np.array(hits["position"], F).reshape(-1, 3).copy()
        prim = hits["prim"].astype(np.int64)
        # analytic quads: the local hit point p of Quad::Intersect, u = p.x / w + 0.5, v = p.z / h + 0.5
        for q, pr in enumerate(self.scene.primitives):
            if pr.shape_type != capi.SHAPE_QUAD:
                continue
            s = np.nonzero(prim == q)[0]
            if not len(s):
                continue
            lo = transform_point(pr.inv[:], o[s])
            ld = transform_normal(pr.mat[:], d[s])
            t = -lo[:, 1] / ld[:, 1]
            p = (lo + ld * t[:, None]).astype(F)
            uv[s, 0] = p[:, 0] / F(pr.shape_param[0]) + F(0.5)
            uv[s, 1] = p[:, 2] / F(pr.shape_param[1]) + F(0.5)
            pos[s] = transform_point(pr.mat[:], p)
        # faces of world-space meshes: identity Transform, local direction = normalize(d)
        s = np.nonzero((prim >= self.n_prims) & (prim < self.n_prims + self.n_world))[0]
        if len(s):
            f = prim[s] - self.n_prims
            p, b1, b2 = triangle_intersect(self.wP[f], o[s], normalize(d[s]))
            uv[s] = self._tri_uv(self.wUV[f], b1, b2)
            pos[s] = p
        # faces of placed copies: Triangle::Intersect in the mesh's space from the local ray, position back through Mat
        for base, nt, mesh, mat, inv in self.inst:
            s = np.nonzero((prim >= base) & (prim < base + nt))[0]
            if not len(s):
                continue
            f = prim[s] - base
            lo = transform_point(inv, o[s])
            ld = transform_normal(mat, d[s])
            p, b1, b2 = triangle_intersect(self.mP[mesh][f], lo, ld)
            uv[s] = self._tri_uv(self.mUV[mesh][f], b1, b2)
            pos[s] = transform_point(mat, p)
        return uv, pos

    @staticmethod
    def _tri_uv(T, b1, b2):
        w0 = F(1.0) - b1 - b2
        return ((w0[:, None] * T[:, 0] + b1[:, None] * T[:, 1]) + b2[:, None] * T[:, 2]).astype(F)

    def albedo(self, hits, uv):
        """rgb [n, 3] float32 the shade kernels use as albedo at the hits: the lookup where the material is textured, else
        the material's rgb; zeros for a miss."""
        n = len(hits)
        out = np.zeros((n, 3), F)
        hit = hits["prim"] >= 0
        mid = np.where(hit, hits["material_id"].astype(np.int64), 0)
        out[hit] = self.mat_rgb[mid[hit]]
        tex = np.where(hit, self.mat_tex[mid], NONE)
        for t, (img, filt, wrp) in enumerate(self.scene.textures):
            s = np.nonzero(tex == t)[0]
            if len(s):
                out[s] = lookup(img, filt, wrp, uv[s, 0], uv[s, 1])
        return out

    def textured(self, hits):
        hit = hits["prim"] >= 0
        mid = np.where(hit, hits["material_id"].astype(np.int64), 0)
        return hit & (self.mat_tex[mid] != NONE)


# ---- the walker: lighting_replay.walk with the looked-up colour as albedo ----------------------------------------------------
MISS_RGB = None   # lighting off under an environment image: a function of the missing rays' directions [m, 3] -> rgb [m, 3]
#                   float32 in the sky's place (a GPU test hands in the device's own lookup, prt_environment_eval, which
#                   tests/test_gpu_environment.py holds to the float64 mapping: a float64 lookup cannot settle a direction on a
#                   texel edge, and a frame compared bit for bit needs every miss)


def walk(scene, osc, cam, W, H, max_depth, seed, pix, samp, sampling=(0, 0, 0.0), use_bvh=False, n_threads=None, start=None):
    """lighting_replay.walk (its `start` too) of a scene with textures (Scene.AddTexture / SetMaterialTexture): the same record; at a vertex whose
    material is textured the attenuation and the `albedo` entry are the looked-up colour.  Every record also carries `uv`."""
    ts = TexScene(scene)
    jitter, rr_depth, clamp = int(sampling[0]), int(sampling[1]), float(sampling[2])
    nt = n_threads or lr.n_threads_default()
    cd = cam.desc()
    pix = np.asarray(pix, np.int64)
    n = len(pix)
    if start is not None:
        o, d, rng = lr.start_rays(start, pix, samp, seed)
    else:
        rng = lr._path_seeds(pix, samp, seed)
        o, d, rng = lr.primary_rays(cd, W, pix, rng, jitter)
    thr = np.ones((n, 3), F)
    path = np.arange(n)
    delivered = np.zeros((n, 3), F)
    last = np.zeros(n, np.int64)
    sky = np.asarray(scene.sky, F)
    mats = scene.materials
    mtypes = np.array([m.type for m in mats], np.int64)
    verts = []
    segs = 0
    for k in range(max_depth):
        if len(path) == 0:
            break
        hits = osc.closest_hit(o, d, use_bvh=use_bvh, n_threads=nt)
        segs += len(path)
        last[path] = k
        hit = hits["prim"] >= 0
        m = len(path)
        uv, _ = ts.hit_uv(o, d, hits)
        colour = ts.albedo(hits, uv)
        is_tex = ts.textured(hits)
        term = np.zeros((m, 3), F)
        term[~hit] = thr[~hit] * (sky if MISS_RGB is None else np.asarray(MISS_RGB(d[~hit]), F).reshape(-1, 3))
        mtype = np.zeros(m, np.int64)
        albedo = np.zeros((m, 3), F)
        scattered = np.zeros(m, bool)
        d_out = np.zeros((m, 3), F)
        o_out = np.zeros((m, 3), F)
        rr_p = np.ones(m, F)
        killed = np.zeros(m, bool)
        thr_out = thr.copy()
        rng_out = rng.copy()
        hi = np.nonzero(hit)[0]
        if len(hi):
            sc, att, em, oo, od, r2 = orc.scatter_batch(mats, d[hi], hits[hi], rng[hi])
            mid = hits["material_id"][hi].astype(np.int64)
            mtype[hi] = mtypes[mid]
            albedo[hi] = colour[hi]
            att = np.where(is_tex[hi][:, None], colour[hi], att).astype(F)   # (textured materials are Lambertian or Metal)
            sc = sc & (k + 1 < max_depth)
            scattered[hi] = sc
            term[hi[~sc]] = thr[hi[~sc]] * em[~sc]
            s_i = hi[sc]
            thr_out[s_i] = thr[s_i] * att[sc]
            o_out[s_i] = oo[sc]
            d_out[s_i] = lr.normalize_rows_f32(od[sc])
            rng_out[s_i] = r2[sc]
            if rr_depth and k + 1 >= rr_depth and len(s_i):
                t = thr_out[s_i]
                p = np.clip(t.max(1), F(0.05), F(1.0)).astype(F)
                u, r3 = lr.rnd(rng_out[s_i])
                rng_out[s_i] = r3
                alive = u.astype(F) < p
                rr_p[s_i] = p
                killed[s_i[~alive]] = True
                thr_out[s_i] = (t / p[:, None]).astype(F)
        ends = ~scattered | killed
        delivered[path[ends]] = lr._clamp32(term[ends], clamp)
        verts.append(dict(path=path, hit=hits, o=o, d=d, thr=thr, key=rng, mtype=mtype, albedo=albedo, scattered=scattered,
                          d_out=d_out, rr_p=rr_p, killed=killed, term=term, uv=uv))
        go = ~ends
        path, o, d, thr, rng = path[go], o_out[go], d_out[go], thr_out[go], rng_out[go]
    return verts, delivered, last, segs


def frame(scene, osc, cam, W, H, max_depth, seed, first_sample, spp, sampling=(0, 0, 0.0), use_bvh=True):
    """Lighting off: (film sums [H, W, 3] float32 = the per-pixel fp32 sum of the delivered terms in sample order, weights,
    segments per depth [max_depth]) of samples first_sample .. first_sample + spp - 1."""
    pix = np.arange(W * H)
    apix = np.tile(pix, spp)
    asamp = np.repeat(np.arange(first_sample, first_sample + spp), len(pix))
    verts, delivered, last, _ = walk(scene, osc, cam, W, H, max_depth, seed, apix, asamp, sampling, use_bvh)
    acc, wts = lr.film_from_delivered(delivered, apix, asamp, W, H)
    per_depth = np.zeros(max_depth, np.int64)
    for k, v in enumerate(verts):
        per_depth[k] = len(v["path"])
    return acc, wts, per_depth


# ---- the test scenes (shared by the CPU and the GPU tests) -------------------------------------------------------------------
SEED = 7


def _random_image(h, w, seed):
    return np.random.default_rng(seed).uniform(0.05, 0.95, size=(h, w, 3)).astype(F)


def scene_a(mode="full"):
    """A: cube_uv.ply (12 triangles, a world-space mesh) and a metal placed copy of it stand on a ground quad under an emissive
    quad.  Textures ("full"): a 4 x 4 checker (nearest, repeat) on the ground, a 3 x 5 random image (bilinear, clamp) on the
    cube, whose UVs are scaled to reach -0.5 .. 1.5, and a 1 x 1 image on the metal copy.  48 x 36, depth 4.
    mode "flat": every one of the three materials gets a 1 x 1 image of its own rgb instead, nearest (the 1 x 1 laws); "none": no
    texture at all (the scene the untextured routes render)."""
    from parallelraytracing_amd import scenes
    W, H = 48, 36
    rgb = {"ground": (0.5, 0.6, 0.7), "body": (0.8, 0.7, 0.6), "metal": (0.9, 0.8, 0.6)}
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian(rgb["ground"])
    light = sc.AddEmissive((15.0, 12.0, 9.0))
    body = sc.AddLambertian(rgb["body"])
    metal = sc.AddMetal(rgb["metal"], 0.1)
    sc.AddQuad(12.0, 10.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    cube = prt.Mesh(scenes.asset("cube_uv.ply"))
    cube.SetUVs(cube.GetUVs() * F(2.0) - F(0.5))
    mat, inv = prt.make_transform((0.6, 0.6, 0.6), (0.0, 20.0, 0.0), (-1.3, -0.39, 0.2))
    cube.transform(mat, inv)
    sc.AddMesh(cube, body)
    sc.AddInstance(prt.Mesh(scenes.asset("cube_uv.ply")), metal, scale=0.5, euler_deg=(0.0, 35.0, 0.0), translation=(1.2, -0.49, 0.4))
    if mode == "full":
        sc.SetMaterialTexture(ground, sc.AddTexture(scenes.checker(4, (0.9, 0.85, 0.8), (0.15, 0.2, 0.1)), "nearest", "repeat"))
        sc.SetMaterialTexture(body, sc.AddTexture(_random_image(5, 3, 1), "bilinear", "clamp"))
        sc.SetMaterialTexture(metal, sc.AddTexture(np.array([[[0.7, 0.9, 0.5]]], F), "nearest", "clamp"))
    elif mode == "flat":
        # (nearest: the bilinear blend (c gx + c fx) gy + (c gx + c fx) fy of four equal texels rounds, and is not c exactly)
        for m, name, wrp in ((ground, "ground", "repeat"), (body, "body", "clamp"), (metal, "metal", "repeat")):
            sc.SetMaterialTexture(m, sc.AddTexture(np.asarray(rgb[name], F).reshape(1, 1, 3), "nearest", wrp))
    else:
        assert mode == "none", mode
    cam = prt.Camera((0.5, 2.5, 6.0), width=W, height=H)
    return dict(name="A_" + mode, scene=sc, cam=cam, W=W, H=H, depth=4, sampling=(0, 0, 0.0), use_bvh=True)


def _small_emissive_cube(at, scale):
    """cube_uv.ply as a world-space mesh of 12 triangles, `scale` of its size around `at` (for a scene without placed copies)."""
    from parallelraytracing_amd import scenes
    cube = prt.Mesh(scenes.asset("cube_uv.ply"))
    mat, inv = prt.make_transform((scale, scale, scale), (0.0, 10.0, 0.0), at)
    cube.transform(mat, inv)
    return cube


def scene_b(emissive_copy=False, copies=True, emissive_sphere=False, emissive_mesh=False, textured=True):
    """B: a 10,000-triangle bunny with planar UVs (a world-space mesh; 16 x 16 random image, bilinear, repeat) and two placed
    copies of the cube at different scale and rotation that share one UV array (8 x 8 checker, nearest, repeat; 3 x 5 random
    image, bilinear, repeat) on an untextured ground under an emissive quad.  40 x 30, depth 4.  emissive_copy: a third, small
    emissive copy (a triangle light for the MESH light sources); copies = False: the bunny alone (a scene that can be refitted).
    emissive_sphere: a third analytic primitive, a floating sphere light; emissive_mesh: the small emissive cube as a world-space
    mesh (a triangle light in a scene without placed copies).  textured = False: the same geometry, materials and UVs with no
    material bound to a texture (the scene the untextured instances render: tests/test_gpu_batch_instances.py)."""
    from parallelraytracing_amd import scenes
    W, H = 40, 30
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.5, 0.5, 0.5))
    light = sc.AddEmissive((15.0, 15.0, 15.0))
    fur = sc.AddLambertian((0.8, 0.7, 0.6))
    c1 = sc.AddLambertian((0.6, 0.6, 0.6))
    c2 = sc.AddMetal((0.9, 0.9, 0.9), 0.3)
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    if emissive_sphere:
        sc.AddCircle(0.25, sc.AddEmissive((6.0, 8.0, 12.0)), translation=(-1.6, 0.9, 1.6))
    bunny = prt.Mesh(scenes.asset("bunny.ply"))
    bunny.SetUVs(scenes.planar_uvs(bunny, (0, 1)) * F(3.0))
    sc.AddMesh(bunny, fur)
    if emissive_mesh:
        sc.AddMesh(_small_emissive_cube((0.2, 1.6, 1.5), 0.15), sc.AddEmissive((40.0, 30.0, 20.0)))
    cube = prt.Mesh(scenes.asset("cube_uv.ply"))
    if copies:
        sc.AddInstance(cube, c1, scale=0.45, euler_deg=(15.0, 30.0, 0.0), translation=(-1.6, -0.3, 0.6))
        sc.AddInstance(cube, c2, scale=0.3, euler_deg=(0.0, 65.0, 20.0), translation=(1.5, -0.4, 0.8))
    if emissive_copy:
        sc.AddInstance(cube, sc.AddEmissive((4.0, 3.0, 2.0)), scale=0.15, euler_deg=(0.0, 10.0, 0.0), translation=(0.2, 1.6, 1.5))
    if textured:
        sc.SetMaterialTexture(fur, sc.AddTexture(_random_image(16, 16, 2), "bilinear", "repeat"))
        sc.SetMaterialTexture(c1, sc.AddTexture(scenes.checker(8), "nearest", "repeat"))
        sc.SetMaterialTexture(c2, sc.AddTexture(_random_image(5, 3, 3), "bilinear", "repeat"))
    cam = prt.Camera((0.6, 1.2, 4.5), width=W, height=H)
    return dict(name="B", scene=sc, cam=cam, W=W, H=H, depth=4, sampling=(0, 0, 0.0), use_bvh=True)


def scene_e(emissive_mesh=False, textured=True):
    """E: scene B's bunny alone (no placed copies; two quads and a sphere, so no primitive BVH) under the emissive quad and a
    floating sphere light; emissive_mesh: plus the small emissive cube as a world-space mesh."""
    return dict(scene_b(copies=False, emissive_sphere=True, emissive_mesh=emissive_mesh, textured=textured), name="E")


# the textured quads of scenes C, D and Q: (width, height, scale, euler_deg, translation, texture).  Non-square, turned about one,
# two and three axes, one scaled; the upright pair faces the camera with opposite faces and the fourth lies face down, so that
# quads are hit on their back faces; textures 0 .. 3 are the four filter x wrap combinations.
_QUADS = (
    (9.0, 4.0, 1.0, (90.0, 0.0, 0.0), (0.0, 1.0, -2.5), 1),        # the back wall
    (1.6, 1.0, 1.0, (35.0, 40.0, 0.0), (-2.2, 0.0, 0.8), 2),
    (1.2, 1.8, 1.0, (200.0, 30.0, 15.0), (2.3, 0.1, 0.6), 3),       # face down
    (1.0, 0.6, 1.7, (50.0, -30.0, 10.0), (-0.9, -0.2, 2.2), 1),     # scaled
    (0.9, 1.3, 1.0, (90.0, 0.0, 0.0), (1.2, -0.3, 2.0), 0),         # upright
    (0.9, 1.3, 1.0, (-90.0, 20.0, 0.0), (-2.4, -0.3, 2.4), 2),      # upright, the other face toward the camera
)


def _textured_quads(sc, extra=0, textured=True):
    """The ground (8 x 8 checker, nearest, repeat), _QUADS and `extra` small tilted quads on a ring, each with a material of its
    own bound to one of four textures (nearest / bilinear x repeat / clamp), under the emissive quad.  -> indices of the quads
    that are turned about at least two axes."""
    from parallelraytracing_amd import scenes
    tex = [sc.AddTexture(scenes.checker(8), "nearest", "repeat"), sc.AddTexture(_random_image(5, 3, 5), "bilinear", "clamp"),
           sc.AddTexture(_random_image(4, 4, 6), "nearest", "clamp"), sc.AddTexture(scenes.checker(4, (0.9, 0.8, 0.3), (0.2, 0.3, 0.6)), "bilinear", "repeat")]

    def quad(w, h, scale, euler, at, t, metal=False):
        m = sc.AddMetal((0.8, 0.8, 0.8), 0.2) if metal else sc.AddLambertian((0.7, 0.7, 0.7))
        if textured:
            sc.SetMaterialTexture(m, tex[t])
        sc.AddQuad(w, h, m, scale=(scale, scale, scale), euler_deg=euler, translation=at)
        return len(sc.primitives) - 1

    quad(20.0, 20.0, 1.0, (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), 0)
    sc.AddQuad(4.0, 4.0, sc.AddEmissive((15.0, 15.0, 15.0)), euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    rotated = []
    for k, (w, h, s, e, at, t) in enumerate(_QUADS):
        q = quad(w, h, s, e, at, t, metal=k == 2)
        if sum(a % 180.0 != 0.0 for a in e) >= 2:
            rotated.append(q)
    for k in range(extra):
        a = 2.0 * np.pi * (k + 0.5) / extra
        rotated.append(quad(0.6, 0.4, 1.0 + 0.1 * (k % 3), (25.0 + 11.0 * k, 30.0 * k, 7.0 * k), (3.3 * np.cos(a), -0.6, 3.3 * np.sin(a)), k % 4))
    return rotated


def scene_c(emissive_mesh=False, copies=False, emissive_copy=False, textured=True):
    """C: 22 analytic primitives, every one placed by rotation + uniform scale + translation, so the primitive BVH is built, and
    no placed copy: the ground, the emissive quad, the six textured quads of _QUADS, a metal sphere, a floating sphere light and
    twelve small Lambertian spheres on a ring, around scene B's 10,000-triangle bunny, whose planar UVs reach -1 .. 2 under a
    bilinear, clamped image.  40 x 30, depth 4.  emissive_mesh: the small emissive cube as a world-space mesh.
    D (copies = True): plus two textured placed copies of the cube, whose shared UVs reach -0.5 .. 1.5, and with emissive_copy a
    third, small emissive one.  textured = False: no material is bound to a texture (scene_b)."""
    from parallelraytracing_amd import scenes
    W, H = 40, 30
    sc = prt.Scene(preset=None)
    rotated = _textured_quads(sc, textured=textured)
    sc.AddCircle(0.45, sc.AddMetal((0.9, 0.8, 0.6), 0.1), translation=(2.6, -0.5, 2.2))
    sc.AddCircle(0.25, sc.AddEmissive((6.0, 8.0, 12.0)), translation=(-1.5, 0.9, 1.8))
    for k in range(12):
        a = 2.0 * np.pi * k / 12.0
        sc.AddCircle(0.1, sc.AddLambertian((0.3 + 0.05 * k, 0.8 - 0.04 * k, 0.5)), scale=(1.2, 1.2, 1.2), euler_deg=(0.0, 30.0 * k, 0.0),
                     translation=(3.1 * np.cos(a), -0.85, 3.1 * np.sin(a)))
    assert len(sc.primitives) >= 20
    fur = sc.AddLambertian((0.8, 0.7, 0.6))
    bunny = prt.Mesh(scenes.asset("bunny.ply"))
    bunny.SetUVs(scenes.planar_uvs(bunny, (0, 1)) * F(3.0) - F(1.0))
    sc.AddMesh(bunny, fur)
    if textured:
        sc.SetMaterialTexture(fur, sc.AddTexture(_random_image(16, 16, 2), "bilinear", "clamp"))
    if emissive_mesh:
        sc.AddMesh(_small_emissive_cube((0.4, 1.5, 2.0), 0.12), sc.AddEmissive((40.0, 30.0, 20.0)))
    if copies:
        cube = prt.Mesh(scenes.asset("cube_uv.ply"))
        cube.SetUVs(cube.GetUVs() * F(2.0) - F(0.5))
        c1, c2 = sc.AddLambertian((0.6, 0.6, 0.6)), sc.AddMetal((0.9, 0.9, 0.9), 0.3)
        sc.AddInstance(cube, c1, scale=0.3, euler_deg=(15.0, 30.0, 0.0), translation=(0.2, -0.5, 2.6))
        sc.AddInstance(cube, c2, scale=0.25, euler_deg=(0.0, 65.0, 20.0), translation=(1.9, -0.5, 3.0))
        if emissive_copy:
            sc.AddInstance(cube, sc.AddEmissive((40.0, 30.0, 20.0)), scale=0.12, euler_deg=(0.0, 10.0, 0.0), translation=(0.4, 1.5, 2.0))
        if textured:
            sc.SetMaterialTexture(c1, sc.AddTexture(scenes.checker(8), "nearest", "repeat"))
            sc.SetMaterialTexture(c2, sc.AddTexture(_random_image(5, 3, 3), "bilinear", "repeat"))
    cam = prt.Camera((0.6, 1.6, 5.5), width=W, height=H)
    return dict(name="D" if copies else "C", scene=sc, cam=cam, W=W, H=H, depth=4, sampling=(0, 0, 0.0), use_bvh=True, rotated_quads=rotated)


def scene_d(emissive_copy=False, textured=True):
    return scene_c(copies=True, emissive_copy=emissive_copy, textured=textured)


def scene_q(big=False):
    """Q: quads only, no triangle at all (no tree: a batch launches no traversal).  The ground, the emissive quad and _QUADS, every
    one but the emitter textured: 8 primitives, scanned linearly; big: plus 12 small tilted quads on a ring, 20 primitives, walked
    through the primitive BVH.  40 x 30, depth 4."""
    W, H = 40, 30
    sc = prt.Scene(preset=None)
    rotated = _textured_quads(sc, extra=12 if big else 0)
    assert len(sc.primitives) == (20 if big else 8)
    cam = prt.Camera((0.6, 1.6, 5.5), width=W, height=H)
    return dict(name="Q_big" if big else "Q_small", scene=sc, cam=cam, W=W, H=H, depth=4, sampling=(0, 0, 0.0), use_bvh=True, rotated_quads=rotated)


def primary_and_random_rays(c, n_random=2000, seed=3):
    """The primary rays of every pixel centre of case c plus random rays toward the scene."""
    import util
    W, H = c["W"], c["H"]
    pix = np.arange(W * H)
    o, d = orc.camera_rays(c["cam"].desc(), (pix % W).astype(F) + F(0.5), (pix // W).astype(F) + F(0.5))
    o2, d2 = util.random_rays(np.random.default_rng(seed), n_random, center=(0.0, 0.0, 0.0), radius=6.0, spread=2.0)
    return np.concatenate([o, o2]).astype(F), np.concatenate([d, d2]).astype(F)


def eval_grid(W, H):
    """UVs for the lookup tests: 0, 1, every texel edge and centre, values just beside them, negative values and values above 1."""
    e = [k / W for k in range(W + 1)] + [(k + 0.5) / W for k in range(W)]
    f = [k / H for k in range(H + 1)] + [(k + 0.5) / H for k in range(H)]
    extra = [-2.25, -1.0, -0.5, -1e-9, 1e-9, 0.999999, 1.000001, 1.5, 2.0, 3.75]
    us = np.array(sorted(set(e + extra)), F)
    vs = np.array(sorted(set(f + extra)), F)
    us = np.unique(np.concatenate([us, np.nextafter(us, F(-np.inf)), np.nextafter(us, F(np.inf))]))
    vs = np.unique(np.concatenate([vs, np.nextafter(vs, F(-np.inf)), np.nextafter(vs, F(np.inf))]))
    uu, vv = np.meshgrid(us, vs)
    return np.stack([uu.ravel(), vv.ravel()], axis=1).astype(F)


# ---- the lighting cases: textured frames through the existing float64 replays ------------------------------------------------
LIGHTING_CASES = ("A_mis_analytic", "B_nee_analytic", "B_mis_mesh", "A_mis_env", "B_nee_mesh_env")
# the cases of tests/test_gpu_texture_instances.py: scenes C (primitive BVH), D (primitive BVH and placed copies) and E (neither)
INSTANCE_LIGHTING_CASES = ("C_mis_analytic", "C_nee_mesh", "C_mis_env", "C_nee_mesh_env", "D_nee_analytic", "D_mis_mesh", "D_nee_analytic_env",
                           "D_mis_mesh_env", "E_mis_analytic", "E_nee_mesh", "E_mis_env", "E_nee_mesh_env")


def patch_walk(monkeypatch):
    """The replays of the lighting modes walk textured paths: every module that holds lighting_replay's walker gets this one."""
    import environment_replay as er
    import mesh_light_replay as mr
    for mod in (lr, mr, er):
        monkeypatch.setattr(mod, "walk", walk)


def lighting_case(name, textured=True):
    """-> (case, mode, replay function of (case, osc)): mis and nee, analytic and mesh light sources, with and without an
    environment image; shared by the CPU test of the undecidable share and the GPU test.  textured = False: the untextured
    scenes B .. E (the replays then need no patch_walk)."""
    import environment_replay as er
    import mesh_light_replay as mr
    scene, mode, sources = name.split("_")[0], name.split("_")[1], ("all" if "mesh" in name else "analytic")
    mesh = sources == "all"
    c = {"A": lambda: scene_a("full" if textured else "none"), "B": lambda: scene_b(emissive_copy=mesh, textured=textured),
         "C": lambda: scene_c(emissive_mesh=mesh, textured=textured), "D": lambda: scene_d(emissive_copy=mesh, textured=textured),
         "E": lambda: scene_e(emissive_mesh=mesh, textured=textured)}[scene]()
    c = dict(c, sources=sources, env="sun", light_share=0.5)
    if name.endswith("_env"):
        return c, mode, lambda c, osc: er.replay_case(c, mode, osc=osc)
    if sources == "all":
        return c, mode, lambda c, osc: mr.replay_case(c, mode, osc=osc, sources="all")
    return c, mode, lambda c, osc: lr.replay_case(c, mode, osc=osc)
