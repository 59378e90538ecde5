"""Coordinate scale / offset cases: a scene transformer, ray families and the case table shared by test_scale_host.py,
test_gpu_scale.py and fuzz_parity.py --scale.

Tree-independence (DESIGN.md sections 0b and 3) rests on quantities that are meant to scale with the data: the per-ray
culling pad 2^-18 (|o|_1 + extent), limit_from_d2, the quantization grid of the 8-wide tree, the clamp on direction
components and the world <-> local conversions of the two-level walk.  Everything here moves a whole scene by a uniform
scale s (a power of two) and a translation T, so that those quantities are exercised away from 1.0."""
import numpy as np

from util import prt  # (util puts the repository root on sys.path)

# (name, s, T, base scene, extreme)
CASES = [
    ("s2^-20", 2.0 ** -20, (0.0, 0.0, 0.0), "bunny", False),
    ("s2^-10", 2.0 ** -10, (0.0, 0.0, 0.0), "bunny", False),
    ("s1", 1.0, (0.0, 0.0, 0.0), "bunny", False),
    ("s2^10", 2.0 ** 10, (0.0, 0.0, 0.0), "bunny", False),
    ("s2^20", 2.0 ** 20, (0.0, 0.0, 0.0), "bunny", False),
    ("T1e3", 1.0, (1e3, 1e3, 1e3), "bunny", False),
    ("T1e4x", 1.0, (1e4, 0.0, 0.0), "bunny", False),
    ("T1e5", 1.0, (1e5, -1e5, 1e5), "bunny", False),
    ("s2^-10_T1e3", 2.0 ** -10, (1e3, 1e3, 1e3), "bunny", False),   # about half of the triangles collapse to zero area
    ("wide", 1.0, (0.0, 0.0, 0.0), "wide", False),                  # bunny at 2^-10 by the origin + icosahedron at 2^10, 1e4 away
    ("s2^-40", 2.0 ** -40, (0.0, 0.0, 0.0), "bunny", True),
    ("s2^30", 2.0 ** 30, (0.0, 0.0, 0.0), "bunny", True),
    ("s2^40", 2.0 ** 40, (0.0, 0.0, 0.0), "bunny", True),
]
NAMES = [c[0] for c in CASES]
NON_EXTREME = [c for c in CASES if not c[4]]
FAMILIES = ("random", "axis", "tiny", "far", "vertex", "lattice")
TINY = (1e-38, -1e-38, 1e-31, -1e-31, 1e-29, -1e-29, 1e-20, -1e-20)
MIN_HIT_SHARE = 0.10
# The reference accepts a hit only at a ray parameter t >= 1e-3 (kShapeRayTMin, an absolute length), so a scene smaller than
# that cannot be hit from inside or from nearby: origins keep at least REACH_MIN from their targets, and a case whose mesh is
# smaller than NEEDS_TARGET gets a second small mesh TARGET_GAP away for the rays that must start ON the first one.
TMIN = 1e-3
REACH_MIN = 4 * TMIN
NEEDS_TARGET = 8 * TMIN
TARGET_GAP = 16 * TMIN


def case(name):
    return CASES[NAMES.index(name)]


# ---- the transformer --------------------------------------------------------------------------------------------------
def move_points(p, s, T):
    """p * s + T in float64, rounded once to fp32."""
    return (np.asarray(p, np.float64) * float(s) + np.asarray(T, np.float64)).astype(np.float32)


def move_mesh(mesh, s, T):
    return prt.Mesh(vertices=move_points(mesh.GetVertices(), s, T), normals=mesh.GetNormals(), indices=mesh.GetIndices())


def _srt(rec):
    """(scale, euler_deg, translation) a primitive / instance was made from: recorded by Scene.Add*; for records that came
    from a preset (no rotation, uniform scale) read back from the matrix."""
    srt = getattr(rec, "srt", None)
    if srt is not None:
        return srt
    m = np.array(rec.mat[:], np.float32).reshape(4, 4)  # column-major: m[c] is column c
    off = m[:3, :3] - np.diag(np.diag(m[:3, :3]))
    if np.any(off != 0) or not (m[0, 0] == m[1, 1] == m[2, 2]):
        raise ValueError("transform with a rotation and no recorded (scale, euler, translation)")
    return (float(m[0, 0]),) * 3, (0.0, 0.0, 0.0), tuple(float(v) for v in m[3, :3])


def move_scene(scene, s, T):
    """The same content under x -> x * s + T: world meshes get new vertices, analytic primitives and placed copies a new
    transform through prt_make_transform (scale * s, translation mapped like a point)."""
    out = prt.Scene(preset=None, sky=scene.sky)
    out.materials = list(scene.materials)
    for p in scene.primitives:
        sc, eu, tr = _srt(p)
        # shape parameters are lengths in the primitive's own space: the transform's scale carries s
        out._add_prim(p.shape_type, p.shape_param[0], p.shape_param[1], p.material_id,
                      tuple(float(np.float32(v) * np.float32(s)) for v in sc), eu, tuple(float(v) for v in move_points(tr, s, T)))
    for m, mat in scene.meshes:
        out.AddMesh(move_mesh(m, s, T), mat)
    for inst in scene.instances:
        sc, eu, tr = _srt(inst)
        out.AddInstance(scene.instanced_meshes[inst.mesh], inst.material_id, scale=tuple(float(np.float32(v) * np.float32(s)) for v in sc),
                        euler_deg=eu, translation=tuple(float(v) for v in move_points(tr, s, T)))
    return out


def move_camera(cam, s, T):
    return prt.Camera(position=tuple(float(v) for v in move_points(cam.position, s, T)), front=cam.front, width=cam.width,
                      height=cam.height)


def move_rays(o, d, s, T):
    return move_points(o, s, T), np.asarray(d, np.float32)


# ---- base scenes --------------------------------------------------------------------------------------------------------
_MESH = {}


def asset_mesh(name, tris=0):
    if (name, tris) not in _MESH:
        m = prt.Mesh(prt.scenes.asset(name))
        _MESH[(name, tris)] = m.refine(tris) if tris else m
    return _MESH[(name, tris)]


def base_scene(kind):
    sc = prt.Scene(preset=None)
    body = sc.AddLambertian((0.8, 0.8, 0.8))
    if kind == "bunny":
        sc.AddMesh(asset_mesh("bunny.ply"), body)
    elif kind == "wide":  # eleven binary orders of magnitude between the two meshes' sizes, twenty in one root box
        sc.AddMesh(move_mesh(asset_mesh("bunny.ply"), 2.0 ** -10, (0.0, 0.0, 0.0)), body)
        sc.AddMesh(move_mesh(asset_mesh("icosahedron.ply", 300), 2.0 ** 10, (1e4, 0.0, 0.0)), sc.AddMetal((0.9, 0.9, 0.9), 0.0))
    else:
        raise ValueError(kind)
    return sc


def case_scene(c):
    """The scene of a case (meshes only: no analytic primitive competes with the tree)."""
    _, s, T, kind, _ = c
    sc = move_scene(base_scene(kind), s, T)
    lo, hi = world_box(sc)
    if float(np.linalg.norm(hi - lo)) < NEEDS_TARGET:  # something beyond tmin for the rays that start on the mesh
        at = np.asarray(T, np.float64) + np.array([0.0, 0.0, TARGET_GAP])
        sc.AddMesh(move_mesh(asset_mesh("icosahedron.ply", 300), 0.5 * s, at), 0)
    return sc


def lit_scene(c):
    """The case's meshes on a ground quad under an emissive quad and a few spheres (frames need light), moved as a whole."""
    _, s, T, kind, _ = c
    sc = base_scene(kind)
    lo, hi = world_box(sc)
    ext = float((hi - lo).max())
    cx, cy, cz = ((lo + hi) / 2).tolist()
    sc.AddQuad(20 * ext, 20 * ext, sc.AddLambertian((0.5, 0.5, 0.5)), translation=(cx, float(lo[1]), cz))
    sc.AddQuad(2 * ext, 2 * ext, sc.AddEmissive((15.0, 15.0, 15.0)), euler_deg=(180.0, 0.0, 0.0), translation=(cx, float(hi[1]) + 2 * ext, cz))
    sc.AddCircle(0.3 * ext, sc.AddDielectric(1.5), translation=(cx + ext, float(lo[1]) + 0.3 * ext, cz))
    sc.AddCircle(0.2 * ext, sc.AddMetal((0.8, 0.8, 0.8), 0.05), translation=(cx - ext, float(lo[1]) + 0.2 * ext, cz + 0.5 * ext))
    ext = max(ext, REACH_MIN / s)  # (a camera closer than the reference's tmin sees nothing)
    cam = prt.Camera(position=(cx + 1.2 * ext, cy + 0.6 * ext, cz + 1.9 * ext),
                     front=tuple(float(v) for v in prt.glm_normalize(np.array([-1.2, -0.6, -1.9], np.float32))), width=64, height=36)
    return move_scene(sc, s, T), move_camera(cam, s, T)


def placed_scene(scale, seed=3):
    """A world mesh, copies of an icosphere at `scale` x {0.5 .. 2}, translations up to 1e4 x scale-free spread, and more
    than 16 analytic primitives (so the walk over their boxes runs as well)."""
    rng = np.random.default_rng([seed, int(np.log2(scale)) + 100])
    s = prt.Scene(preset=None)
    mats = [s.AddLambertian((0.7, 0.6, 0.5)), s.AddMetal((0.9, 0.9, 0.9), 0.05), s.AddEmissive((6.0, 6.0, 6.0))]
    ico = asset_mesh("icosahedron.ply", 1200)
    span = 4.0 * scale                      # the copies sit within a few of their own sizes of each other ...
    far = (1e4, 0.0, -1e4)                  # ... around the origin and around a point 1e4 away
    s.AddMesh(move_mesh(asset_mesh("bunny.ply"), 8.0 * scale, (0.0, 0.0, 0.0)), mats[0])
    for k in range(8):
        base = np.zeros(3) if k < 5 else np.array(far)
        s.AddInstance(ico, mats[k % 2], scale=float(scale * rng.uniform(0.5, 2.0)),
                      euler_deg=tuple(float(v) for v in rng.uniform(-180, 180, 3)),
                      translation=tuple(float(v) for v in base + rng.uniform(-span, span, 3)))
    s.AddQuad(40 * scale, 40 * scale, mats[0], translation=(0.0, -3.0 * scale, 0.0))
    s.AddQuad(4 * scale, 4 * scale, mats[2], euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 8.0 * scale, 0.0))
    for _ in range(20):
        s.AddCircle(float(rng.uniform(0.2, 0.8)), mats[int(rng.integers(0, 2))], scale=(scale,) * 3,
                    translation=tuple(float(v) for v in rng.uniform(-span, span, 3)))
    return s


# ---- geometry of a scene, as the kernels see it (fp32 vertices in world space) -----------------------------------------
def world_triangles(scene):
    """[nt, 3, 3] float64: the triangles of the world meshes and of every placed copy (vertices through the copy's fp32
    matrix, in float64)."""
    out = []
    for m, _ in scene.meshes:
        out.append(m.GetVertices().astype(np.float64)[m.GetIndices()])
    for inst in scene.instances:
        m = scene.instanced_meshes[inst.mesh]
        M = np.array(inst.mat[:], np.float64).reshape(4, 4).T  # column-major -> row-major
        v = m.GetVertices().astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        out.append(v[m.GetIndices()])
    return np.concatenate(out) if out else np.zeros((0, 3, 3))


def world_box(scene):
    t = world_triangles(scene).reshape(-1, 3)
    return t.min(axis=0), t.max(axis=0)


def _norm(d):
    return np.stack([prt.glm_normalize(v) for v in np.asarray(d, np.float32)]).astype(np.float32)


# ---- ray families -------------------------------------------------------------------------------------------------------
def ray_families(scene, rng, n=256):
    """name -> (o, d), fp32, directions normalised as the fuzzer does.  Built from the scene as it stands (after the
    move), with every length relative to the scene's own box, so that a family keeps its meaning at any scale."""
    tris = world_triangles(scene)
    lo, hi = tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)
    diam = float(np.linalg.norm(hi - lo))
    reach = max(diam, REACH_MIN)
    ctr = (lo + hi) / 2
    # targets: centroids of triangles with area (a zero-area triangle cannot be hit), chosen per ray
    area = np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1)
    solid = np.nonzero(area > 0)[0]
    cen = tris[solid].mean(axis=1)

    def targets(k):
        return cen[rng.integers(0, len(cen), k)]

    def unit(k):
        u = rng.normal(size=(k, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True)

    fam = {}
    # random origins around the scene, aimed into it
    o = (ctr + unit(n) * rng.uniform(1.0, 4.0, (n, 1)) * reach).astype(np.float32)
    fam["random"] = (o, _norm(targets(n) - o.astype(np.float64)))
    # axis-parallel, exactly zero components; on the zero axes the origin lies inside the scene's box
    tg = targets(n)
    ax = rng.integers(0, 3, n)
    sg = rng.choice([-1.0, 1.0], n)
    d = np.zeros((n, 3), np.float32)
    d[np.arange(n), ax] = sg
    o = tg.copy()
    o[np.arange(n), ax] -= sg * rng.uniform(1.0, 3.0, n) * reach
    o = o.astype(np.float32)
    inside = np.ones((n, 3), bool)
    inside[np.arange(n), ax] = False
    lo32, hi32 = np.nextafter(lo.astype(np.float32), np.float32(-np.inf)), np.nextafter(hi.astype(np.float32), np.float32(np.inf))
    assert np.all(((o >= lo32) & (o <= hi32))[inside])  # (inside the box up to the rounding of the box itself)
    fam["axis"] = (o, d)
    # one direction component tiny (below, at and above the kernels' clamp), the ray otherwise in a coordinate plane
    tg = targets(n)
    ax = rng.integers(0, 3, n)
    d = unit(n)
    d[np.arange(n), ax] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (tg - d * rng.uniform(1.0, 3.0, (n, 1)) * reach).astype(np.float32)
    d = d.astype(np.float32)
    d[np.arange(n), ax] = np.array(TINY, np.float32)[np.arange(n) % len(TINY)]
    d = _norm(d)
    assert np.all(np.abs(d[np.arange(n), ax]) <= np.float32(1.0000001e-20)) and np.all(d[np.arange(n), ax] != 0)
    fam["tiny"] = (o, d)
    # 10^3 scene diameters away (more where that is still closer than the reference's tmin)
    o = (ctr + unit(n) * max(1e3 * diam, REACH_MIN)).astype(np.float32)
    fam["far"] = (o, _norm(targets(n) - o.astype(np.float64)))
    # origins exactly on mesh vertices, aimed at a triangle farther than tmin from them (through the mesh, or at another)
    verts = tris.reshape(-1, 3)
    o = verts[rng.integers(0, len(verts), n)].astype(np.float32)
    tg = targets(n)
    for _ in range(64):
        near = np.linalg.norm(tg - o, axis=1) < 2 * TMIN
        if not near.any():
            break
        tg[near] = targets(int(near.sum()))
    fam["vertex"] = (o, _norm(tg - o.astype(np.float64)))
    # origins on the fp32 lattice points nearest to the root's box planes (on the plane and one step to either side),
    # anywhere on those planes around the scene
    o = (ctr + unit(n) * rng.uniform(1.0, 3.0, (n, 1)) * reach).astype(np.float32)
    ax = rng.integers(0, 3, n)
    plane = np.where(rng.random(n) < 0.5, lo[ax], hi[ax]).astype(np.float32)
    step = rng.integers(-1, 2, n)
    plane = np.where(step < 0, np.nextafter(plane, np.float32(-np.inf)), np.where(step > 0, np.nextafter(plane, np.float32(np.inf)), plane))
    o[np.arange(n), ax] = plane
    d = targets(n) - o.astype(np.float64)
    slide = rng.random(n) < 0.25   # a quarter of them travel inside the plane
    d[slide, ax[slide]] = 0.0
    fam["lattice"] = (o, _norm(d))
    assert tuple(fam) == FAMILIES
    return fam


def all_rays(fam):
    return np.concatenate([fam[f][0] for f in fam]), np.concatenate([fam[f][1] for f in fam])


def hit_shares(fam, want):
    """Share of oracle hits per family (`want`: the oracle's closest hits of all_rays(fam)); the caller asserts the floor."""
    shares, k = {}, 0
    for f in fam:
        n = len(fam[f][0])
        shares[f] = float((want["prim"][k:k + n] >= 0).mean())
        k += n
    return shares


def draw(rng):
    """A non-extreme (s, T) that moves the scene, for the fuzzer ("s1" and "wide" are the identity on a scene that is not theirs)."""
    moving = [c for c in NON_EXTREME if c[1] != 1.0 or any(c[2])]
    c = moving[int(rng.integers(0, len(moving)))]
    return c[0], c[1], c[2]


# ---- hits of the reference that no box can follow ---------------------------------------------------------------------
def phantom_winners(scene, o, d, want, coeff=2.0 ** -18):
    """Rays whose winner in the reference's arithmetic is reported at a position the ray does not come near: in float64 the
    ray (as fp32 data) passes farther from the REPORTED hit position than the walk's per-ray pad coeff * (|o|_1 + extent).
    The reference's barycentrics are then rounding noise (a sliver of area A and length L seen from D away: numerators of
    size u D L against a divisor of 2 A cos, i.e. a reach of u D L^2 / (2 A cos) along the sliver), and no box of the
    triangle, however padded in proportion to the coordinates, is entered before the bound that the reported distance sets:
    DESIGN.md section 0.  Conversely a winner reported within the pad of the ray is inside its padded leaf box at a
    parameter within the pad of the reported distance, which limit_from_d2 admits: the walk owes those.  A rule on the
    oracle's output alone.  World-space meshes only."""
    assert not scene.instances
    n_prims = len(scene.primitives)
    hit = np.nonzero(want["prim"] >= n_prims)[0]
    out = np.zeros(len(o), bool)
    if not len(hit):
        return out
    oo, dd = o[hit].astype(np.float64), d[hit].astype(np.float64)
    dd = dd / np.linalg.norm(dd, axis=1, keepdims=True)
    w = want["position"][hit].astype(np.float64) - oo
    t = np.maximum((w * dd).sum(1), 0.0)
    dist = np.linalg.norm(w - t[:, None] * dd, axis=1)
    extent = np.abs(world_triangles(scene)).max()
    out[hit] = dist > coeff * (np.abs(oo).sum(1) + extent)
    return out


# ---- many analytic primitives: the walk over their world boxes -------------------------------------------------------
def balls_scene(c):
    """RANDOM_BALLS_MEDIUM (a ground quad and 408 spheres, 80 units across) moved by the case's (s, T)."""
    return move_scene(prt.Scene("RANDOM_BALLS_MEDIUM"), c[1], c[2])


def ball_rays(scene, rng, n=256):
    """name -> (o, d) aimed at the spheres of a scene of analytic primitives: random, axis-parallel (exactly zero
    components, through a sphere), one component tiny, and from 10^3 scene diameters away."""
    sph = [p for p in scene.primitives if p.shape_type == 0]
    C = np.array([[p.mat[12], p.mat[13], p.mat[14]] for p in sph], np.float64)
    R = np.array([abs(p.shape_param[0]) * abs(p.mat[0]) for p in sph], np.float64)
    diam = float(np.linalg.norm(C.max(axis=0) - C.min(axis=0)))

    def unit(k):
        u = rng.normal(size=(k, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True)
    fam = {}
    i = rng.integers(0, len(sph), n)
    o = (C[i] + unit(n) * (rng.uniform(3.0, 60.0, (n, 1)) * R[i, None])).astype(np.float32)
    fam["random"] = (o, _norm(C[i] + 0.5 * R[i, None] * unit(n) - o.astype(np.float64)))
    i = rng.integers(0, len(sph), n)
    ax, sg = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
    d = np.zeros((n, 3), np.float32)
    d[np.arange(n), ax] = sg
    o = C[i] + 0.5 * R[i, None] * unit(n)
    o[np.arange(n), ax] -= sg * rng.uniform(3.0, 60.0, n) * R[i]
    fam["axis"] = (o.astype(np.float32), d)
    i = rng.integers(0, len(sph), n)
    ax = rng.integers(0, 3, n)
    d = unit(n)
    d[np.arange(n), ax] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (C[i] - d * (rng.uniform(3.0, 60.0, (n, 1)) * R[i, None])).astype(np.float32)
    d = d.astype(np.float32)
    d[np.arange(n), ax] = np.array(TINY, np.float32)[np.arange(n) % len(TINY)]
    fam["tiny"] = (o, _norm(d))
    i = rng.integers(0, len(sph), n)
    o = (C.mean(axis=0) + unit(n) * 1e3 * diam).astype(np.float32)
    fam["far"] = (o, _norm(C[i] - o.astype(np.float64)))
    return fam
