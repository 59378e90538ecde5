"""Deep trees: meshes whose host-built 8-wide tree has 9 .. 19 levels with a few hundred triangles, rays that walk them to
the bottom, and numpy emulations of the 8-wide and 4-wide walks that say how many stack entries a ray needs.  Shared by
test_deep_trees_host.py (the gate: the depths, and that the rays really need the upper stack rows),
test_gpu_deep_trees.py (every traversal instance against the linear scan) and test_host_logic.py (the emulation).

A telescope is a comb of levels i = 0 .. n-1 of size s = ratio^-i along the x axis: `per` thin triangles per level at
x = s, spread over 0.3 s (k - per / 2) in y, each 0.4 s x 0.25 s with a tilt of up to 0.1 s in z.  Every level sits in
the corner of the box of all larger ones, so the builder's splits peel the levels off one by one and the tree is a chain:
its depth grows with the number of levels, not with the number of triangles."""
import functools

import numpy as np

import boxtest_replay as bx
import scale_cases as sc
import util
from util import prt

MIN_SIZE = 2.0 ** -36   # the smallest level against the largest (the range tests/scale_cases.py holds)
F = np.float32


def telescope(ratio, per, levels, seed, scale=1.0, min_size=MIN_SIZE):
    """prt.Mesh with normals (face normals, float64 cross products): 3 * per * levels vertices, triangle t belongs to
    level t // per."""
    assert float(ratio) ** -(levels - 1) >= min_size, (ratio, levels)
    rng = np.random.default_rng([seed, per, levels])
    V = np.zeros((levels, per, 3, 3))
    for i in range(levels):
        s = float(scale) * float(ratio) ** -i
        u = rng.random((per, 2))
        base = np.stack([np.full(per, s), 0.3 * s * (np.arange(per) - per / 2), np.zeros(per)], axis=1)
        V[i, :, 0] = base
        V[i, :, 1] = base + np.stack([np.full(per, 0.4 * s), np.zeros(per), 0.1 * s * u[:, 0]], axis=1)
        V[i, :, 2] = base + np.stack([np.zeros(per), np.full(per, 0.25 * s), 0.1 * s * u[:, 1]], axis=1)
    V32 = V.reshape(-1, 3).astype(F)
    T = V32.astype(np.float64).reshape(-1, 3, 3)
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return prt.Mesh(vertices=V32, normals=np.repeat(n, 3, axis=0).astype(F), indices=np.arange(len(V32), dtype=np.uint32).reshape(-1, 3))


# name -> (ratio, per, levels, seed, depth8 of the host builder's tree, asserted by test_deep_trees_host.py)
CASES = {
    "d9": (1.25, 3, 40, 1, 9),
    "d10": (1.5, 4, 40, 1, 10),
    "d12": (1.25, 8, 80, 1, 12),
    "d15": (1.25, 3, 80, 1, 15),
    "d16": (1.35, 3, 70, 1, 16),
    "d17": (1.25, 3, 100, 1, 17),
    "d19": (1.3, 3, 95, 1, 19),
}
NAMES = list(CASES)
# max_stack4 92 .. 99: beyond the 27 + 64 entries the spill area held before it was sized from the tree.  CPU only.
BIG = {"big30": (2.0, 3, 80, 1), "big34": (2.0, 8, 80, 1)}
# the instanced meshes of the two-level scenes may use this one too (11 levels)
EXTRA = {"d11": (1.5, 4, 44, 1, 11)}
# two-level scenes: name -> (instanced mesh, placed copies, top_depth + mesh depth).  Six copies fit one top-level node.
PLACED = {"p11": ("d10", 6, 11), "p12": ("d11", 6, 12)}
PLACED_REFUSED = ("d11", 10, "2 + 11 > 12")   # ten copies need two top levels: 13, refused
FAMILIES = ("axis", "level", "random", "far")


def params(name):
    return CASES.get(name) or EXTRA.get(name) or BIG[name]


def case_mesh(name):
    ratio, per, levels, seed = params(name)[:4]
    return telescope(ratio, per, levels, seed, min_size=0.0 if name in BIG else MIN_SIZE)


def mesh_scene(mesh):
    s = prt.Scene(preset=None)
    s.AddMesh(mesh, s.AddLambertian((0.8, 0.8, 0.8)))
    return s


def case_scene(name):
    return mesh_scene(case_mesh(name))


def host(scene):
    r = prt.HipWavefrontRenderer(device=-1)
    r.set_scene_host_only(scene)
    return r


def copy_transforms(n, seed=7):
    """(scale, euler_deg, translation) of n placed copies: rotated, scaled 0.5 .. 2, on a ring (so that the top level has
    something to split) with their combs pointing every way."""
    rng = np.random.default_rng([seed, n])
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        out.append((float(rng.uniform(0.5, 2.0)), tuple(float(v) for v in rng.uniform(-180, 180, 3)),
                    (float(6 * np.cos(a)), float(rng.uniform(-1, 1)), float(6 * np.sin(a)))))
    return out


def placed_scene(mesh, n, seed=7, moved=False):
    s = prt.Scene(preset=None)
    mat = s.AddLambertian((0.7, 0.7, 0.7))
    for scale, eu, tr in copy_transforms(n, seed):
        if moved:
            eu, tr = tuple(e + 25.0 for e in eu), (tr[0] * 1.25, tr[1] - 0.5, tr[2] * 1.25)
        s.AddInstance(mesh, mat, scale=scale, euler_deg=eu, translation=tr)
    return s


def clustered_scene(mesh, n, step=0.01):
    """n unrotated copies `step` apart: one top-level node holds them all (three copies per leaf slot)."""
    s = prt.Scene(preset=None)
    mat = s.AddLambertian((0.7, 0.7, 0.7))
    for k in range(n):
        s.AddInstance(mesh, mat, scale=1.0, euler_deg=(0.0, 0.0, 0.0), translation=(step * k, 0.0, 0.0))
    return s


def deformed(mesh):
    """The same topology scaled by 1.5 and sheared (x += 0.3 y, z += 0.2 x), with its own face normals."""
    v = mesh.GetVertices().astype(np.float64) * 1.5
    v = np.stack([v[:, 0] + 0.3 * v[:, 1], v[:, 1], v[:, 2] + 0.2 * v[:, 0]], axis=1).astype(F)
    T = v.astype(np.float64)[mesh.GetIndices()]
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    nv = np.zeros((len(v), 3))
    nv[mesh.GetIndices().ravel()] = np.repeat(n, 3, axis=0)
    return prt.Mesh(vertices=v, normals=nv.astype(F), indices=mesh.GetIndices())


# ---- rays -------------------------------------------------------------------------------------------------------------
def _unit(rng, k):
    u = rng.normal(size=(k, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def local_rays(tris, per, rng, n=256):
    """name -> (o, d, level aimed at) in float64, in the mesh's own space.  tris: [nt, 3, 3], triangle t of level t // per."""
    levels = len(tris) // per
    lo, hi = tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)
    diam = float(np.linalg.norm(hi - lo))
    size = np.abs(tris[::per, 0, 0])   # s of every level

    def targets(lv):
        t = lv * per + rng.integers(0, per, len(lv))
        w = 0.5 / 3 + 0.5 * rng.dirichlet((1.0, 1.0, 1.0), len(lv))   # interior: every weight >= 1/6
        return (tris[t] * w[:, :, None]).sum(axis=1)

    fam = {}
    # along the chain axis from outside through the shells: all 8 direction octants, small slopes in y and z
    # (twice as many as of the other families: two of the eight octants reach the bottom of the stack)
    na = 2 * n
    lv = rng.integers(0, levels, na)
    tg = targets(lv)
    k = np.arange(na)
    sg = np.stack([np.where(k & 1, -1.0, 1.0), np.where(k & 2, -1.0, 1.0), np.where(k & 4, -1.0, 1.0)], axis=1)
    d = sg * np.stack([np.ones(na), rng.uniform(0.005, 0.3, na), rng.uniform(0.005, 0.12, na)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    fam["axis"] = (tg - d * rng.uniform(2.0, 3.0, (na, 1)) * diam, d, lv)
    # from near each level at that level's triangles: every level several times, half of them straight down / up z from
    # exactly above the target (the origin's x and y ARE the target's), never closer than the reference's tmin allows
    m = max(n, 8 * levels)
    lv = np.arange(m) % levels
    tg = targets(lv)
    reach = np.maximum(3.0 * size[lv], sc.REACH_MIN)
    u = _unit(rng, m) + 2.0 * np.where(rng.random(m) < 0.5, -1.0, 1.0)[:, None] * np.array([0.0, 0.0, 1.0])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    straight = (np.arange(m) // levels) % 2 == 0
    u[straight] = np.where(rng.random(int(straight.sum())) < 0.5, -1.0, 1.0)[:, None] * np.array([0.0, 0.0, 1.0])
    fam["level"] = (tg + u * reach[:, None], -u, lv)
    lv = rng.integers(0, levels, n)
    tg = targets(lv)
    o = (lo + hi) / 2 + _unit(rng, n) * rng.uniform(1.0, 4.0, (n, 1)) * diam
    fam["random"] = (o, tg - o, lv)
    lv = rng.integers(0, levels, n)
    tg = targets(lv)
    o = (lo + hi) / 2 + _unit(rng, n) * 1e3 * diam
    fam["far"] = (o, tg - o, lv)
    assert tuple(fam) == FAMILIES
    return fam


def _f32_rays(o, d):
    o = np.asarray(o, F)
    return o, np.stack([prt.glm_normalize(v) for v in np.asarray(d, F)]).astype(F)


def ray_families(scene, per, seed, n=256):
    """name -> (o, d, level) in fp32 world space.  One-level scenes: the mesh's own space.  Placed copies: the local rays
    of the instanced mesh dealt out to the copies in turn and moved by each copy's matrix."""
    rng = np.random.default_rng([41, seed])
    if not scene.instances:
        tris = scene.meshes[0][0].GetVertices().astype(np.float64)[scene.meshes[0][0].GetIndices()]
        return {f: _f32_rays(o, d) + (lv,) for f, (o, d, lv) in local_rays(tris, per, rng, n).items()}
    mesh = scene.instanced_meshes[0]
    tris = mesh.GetVertices().astype(np.float64)[mesh.GetIndices()]
    fam = {}
    for f, (o, d, lv) in local_rays(tris, per, rng, n).items():
        ow, dw = np.zeros_like(o), np.zeros_like(d)
        for k, inst in enumerate(scene.instances):
            M = np.array(inst.mat[:], np.float64).reshape(4, 4).T
            sel = np.arange(len(o)) % len(scene.instances) == k
            ow[sel] = o[sel] @ M[:3, :3].T + M[:3, 3]
            dw[sel] = d[sel] @ M[:3, :3].T
        fam[f] = _f32_rays(ow, dw) + (lv,)
    return fam


def all_rays(fam):
    return np.concatenate([fam[f][0] for f in fam]), np.concatenate([fam[f][1] for f in fam])


def family_slices(fam):
    out, k = {}, 0
    for f in fam:
        out[f] = slice(k, k + len(fam[f][0]))
        k += len(fam[f][0])
    return out


def make_scene(name, moved=False):
    if name in PLACED:
        mname, n, _ = PLACED[name]
        return placed_scene(case_mesh(mname), n, moved=moved)
    return case_scene(name)


def scene_data(scene, per, seed, n=256):
    """What a test of one scene needs, computed once: the ray families, all rays, the oracle's LINEAR SCAN of them, the
    scene's diameter, and the probe: the ray with the deepest stack by the lower estimate of stack_need8 on the host
    builder's tree, as a camera (33 x 33: the centre pixel's primary ray is that ray) for measure_traversal and frames."""
    fam = ray_families(scene, per, seed, n)
    o, d = all_rays(fam)
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=False, n_threads=8)
    lo, hi = sc.world_box(scene)
    r = host(scene)
    low = stack_need8(r, scene, o, d, want["d2"])
    best = int(np.argmax(low))
    cam = prt.Camera(position=tuple(float(v) for v in o[best]), front=tuple(float(v) for v in d[best]), width=33, height=33)
    co, cd = util.orc.camera_rays(cam.desc(), np.array([16.5], F), np.array([16.5], F))
    cw = util.oracle_scene(scene).closest_hit(co, cd, use_bvh=False, n_threads=1)
    probe_need = int(stack_need8(r, scene, co, cd, cw["d2"])[0])
    probe_need4 = 0 if scene.instances else int(stack_need4(r, co, cd, cw["d2"])[0])   # (the same ray on the 4-wide tree)
    return dict(scene=scene, per=per, fam=fam, o=o, d=d, want=want, diam=float(np.linalg.norm(hi - lo)), cam=cam, probe_need=probe_need,
                probe_need4=probe_need4, info=r.bvh_info())


@functools.lru_cache(maxsize=None)
def case_data(name, moved=False):
    per = params(PLACED[name][0] if name in PLACED else name)[1]
    return scene_data(make_scene(name, moved), per, (list(CASES) + list(PLACED)).index(name) + (100 if moved else 0))


def hit_shares(fam, want):
    return {f: float((want["prim"][s] >= 0).mean()) for f, s in family_slices(fam).items()}


# ---- the 8-wide walk in numpy --------------------------------------------------------------------------------------------
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)
_TOP8 = np.array([max(i.bit_length() - 1, 0) for i in range(256)], np.int64)


def walk8(D, o, d, pad, tlimit, root=None):
    """k_traverse8_persistent's node-group / hit-mask logic (same bit operations, same visiting order) for all rays in
    lockstep.  D: util.decode8 of the node array; o, d: [n, 3] float64 (d need not be unit: tlimit is in its parameter);
    pad [n]: the slack every child box gets (the kernel's per-ray pad); tlimit [n]: culling bound (np.inf: none);
    root [n]: the node each ray starts at (default 0).
    Returns (need [n]: the deepest stack, in entries; leaves: list of (ray, first slot, 24-bit mask, stack entries at
    that moment, siblings pending in the current group) in visiting order)."""
    n = len(o)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    dmin = float(bx.kernel_dir_min())
    inv = 1.0 / np.where(np.abs(d) < dmin, np.copysign(dmin, d), d)
    neg = inv < 0
    octinv = 7 - (neg[:, 0].astype(np.int64) | neg[:, 1].astype(np.int64) << 1 | neg[:, 2].astype(np.int64) << 2)
    gx = np.zeros(n, np.int64) if root is None else np.asarray(root, np.int64).copy()
    gy = np.int64(1) << (24 + octinv)
    depth_cap = 64
    stack = np.zeros((n, depth_cap, 2), np.int64)
    sp = np.zeros(n, np.int64)
    need = np.zeros(n, np.int64)
    alive = np.ones(n, bool)
    leaves = []
    pad = np.broadcast_to(np.asarray(pad, np.float64), (n,))
    tlimit = np.broadcast_to(np.asarray(tlimit, np.float64), (n,))
    while True:
        has = gy > 0x00FFFFFF
        alive &= has | (sp > 0)
        if not alive.any():
            break
        r = np.nonzero(alive)[0]
        pop = r[~has[r]]
        sp[pop] -= 1
        gx[pop], gy[pop] = stack[pop, sp[pop], 0], stack[pop, sp[pop], 1]
        bit = 24 + _TOP8[gy[r] >> 24]
        gy[r] &= ~(np.int64(1) << bit)
        push = r[gy[r] > 0x00FFFFFF]
        stack[push, sp[push], 0], stack[push, sp[push], 1] = gx[push], gy[push]
        sp[push] += 1
        assert sp.max() < depth_cap
        need = np.maximum(need, sp)
        slot = (bit - 24) ^ octinv[r]
        idx = gx[r] + _POP8[gy[r] & ((np.int64(1) << slot) - 1) & 0xFF]
        lo, hi = D["lo"][idx] - pad[r, None, None], D["hi"][idx] + pad[r, None, None]   # [m, child, axis]
        ng = neg[r][:, None, :]
        near, far = np.where(ng, hi, lo), np.where(ng, lo, hi)
        with np.errstate(all="ignore"):
            tn = np.maximum(((near - o[r, None, :]) * inv[r, None, :]).max(axis=2), 0.0)
            tf = np.minimum(((far - o[r, None, :]) * inv[r, None, :]).min(axis=2), tlimit[r, None])
        meta = D["meta"][idx]
        ok = (meta != 0) & (tn <= tf)
        inner = ((meta & (meta << 1)) & 0x10) != 0
        bidx = (meta ^ np.where(inner, octinv[r, None], 0)) & 0x1F
        hitmask = np.bitwise_or.reduce(np.where(ok, (meta >> 5) << bidx, 0), axis=1)
        gx[r] = D["child_base"][idx]
        gy[r] = (hitmask & 0xFF000000) | D["imask"][idx]
        tm = hitmask & 0x00FFFFFF
        for j in np.nonzero(tm)[0]:
            leaves.append((int(r[j]), int(D["tri_base"][idx[j]]), int(tm[j]), int(sp[r[j]]), bool(gy[r[j]] > 0x00FFFFFF)))
    return need, leaves


def leaf_slots(first, mask):
    out = []
    while mask:
        out.append(first + (mask & -mask).bit_length() - 1)
        mask &= mask - 1
    return out


def _limits(o, d2, extent):
    """The kernel's per-ray pad, and limit_from_d2 of a known squared hit distance (None / a miss: no bound)."""
    pad = bx.ray_pad(np.asarray(o, F), extent).astype(np.float64)
    if d2 is None:
        return pad, np.full(len(pad), np.inf)
    d2 = np.asarray(d2, np.float64)
    with np.errstate(all="ignore"):
        return pad, np.where(d2 < 3.0e38, np.sqrt(d2) * 1.0000153 + 4.0 * pad, np.inf)


def stack_need8(r, scene, o, d, d2=None):
    """Per ray, the deepest stack (entries) the 8-wide walk of renderer r's tree of `scene` reaches; for scenes with placed copies the
    sum across the level switch (the top level's entries, its pending siblings, the sentinel, the copy's own tree).

    d2 = None: no culling bound at all: an UPPER estimate (the kernel culls with the best hit so far).  d2 = the closest
    hits' squared distances (misses: FLT_MAX): the walk culled with the FINAL bound from its first step, which the kernel
    only knows at the end: a LOWER estimate, up to the boxes' slack (the kernel's pad, here in float64).  The hard figure
    is measure_traversal().max_stack_used on the device."""
    n8 = r.bvh_read8()
    D = util.decode8(n8)
    o64 = np.asarray(o, F).astype(np.float64)
    d64 = np.stack([prt.glm_normalize(v) for v in np.asarray(d, F)]).astype(np.float64)
    _, tris = r.bvh_read()
    tab = r.instances_read() if scene.instances else None
    if tab is None:
        pad, tl = _limits(o, d2, np.abs(tris.reshape(-1, 3, 4)[:, :, :3]).max())
        return walk8(D, o64, d64, pad, tl)[0]
    # two levels: the top-level walk's leaves are copies
    insts = scene.instances
    ext_w = float(np.abs(sc.world_triangles(scene)).max())
    pad_w, tl_w = _limits(o, d2, ext_w)
    need, leaves = walk8(D, o64, d64, pad_w, tl_w)
    ray, root, base = [], [], []
    for k, first, mask, sp, pending in leaves:
        for s in leaf_slots(first, mask):
            ray.append(k)
            root.append(s)
            base.append(sp + int(pending) + 1)   # the pending siblings go below the sentinel
    if not ray:
        return need
    ray, slot = np.array(ray), np.array(root)
    which = tab["slot_instance"][slot].astype(np.int64)
    ol, dl, padl, tll = np.zeros((len(ray), 3)), np.zeros((len(ray), 3)), np.zeros(len(ray)), np.zeros(len(ray))
    mesh = scene.instanced_meshes[0]
    ext_l = float(np.abs(mesh.GetVertices()).max())
    for i in np.unique(which):
        sel = which == i
        Mi = np.array(insts[i].inv[:], np.float64).reshape(4, 4).T
        ol[sel] = o64[ray[sel]] @ Mi[:3, :3].T + Mi[:3, 3]
        dl[sel] = d64[ray[sel]] @ Mi[:3, :3].T
        inv_scale = np.linalg.norm(Mi[:3, 0])
        padl[sel] = 2.0 ** -18 * (np.abs(ol[sel]).sum(axis=1) + ext_l)
        tll[sel] = (tl_w[ray[sel]] + 4.0 * pad_w[ray[sel]]) * inv_scale * 1.000001 + 4.0 * padl[sel]
    # (dl is the unit world direction times inv_scale: the parameter along it is the world distance, so the local bound
    # above, a local length, is divided by inv_scale again)
    scale_l = np.linalg.norm(dl, axis=1)
    need_l, _ = walk8(D, ol, dl, padl, tll / scale_l, root=tab["root"][which].astype(np.int64))
    np.maximum.at(need, ray, np.array(base) + need_l)
    return need


def _fma32(a, b, c):
    """fp32 fma: the product of two binary32 values is exact in binary64."""
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def stack_need4(r, o, d, d2):
    """Per ray, a LOWER estimate of the deepest stack (entries held at the end of a node step, what the kernel's
    max_stack_used counts) of k_traverse4_persistent's walk of renderer r's 4-wide tree: the kernel's box test in its own
    fp32 operations, the same 5-comparator ordering and farthest-first pushes, culled with the FINAL bound (d2: the closest
    hits' squared distances) from the first step, and every leaf consumed the moment it is met.  The kernel culls with the
    best hit so far, a looser bound: what it enters beyond this walk lies behind everything this walk keeps (entry
    distance above the final bound), sorts after it and is stacked below the same path.  It also holds one leaf back while
    it walks on, which only delays pops.  One-level scenes; plain Python, meant for a few rays."""
    n4 = r.bvh_read4()
    refs = n4[:, 24:28].copy().view(np.int32)
    _, tris = r.bvh_read()
    extent = np.abs(tris.reshape(-1, 3, 4)[:, :, :3]).max()
    dmin, inf = bx.kernel_dir_min(), F(np.inf)
    out = []
    for oo, dd, q2 in zip(np.asarray(o, F), np.asarray(d, F), np.asarray(d2, F)):
        ld = np.asarray(prt.glm_normalize(dd), F)
        pad = bx.ray_pad(oo, extent)
        inv = (F(1.0) / np.where(np.abs(ld) < dmin, np.copysign(dmin, ld), ld)).astype(F)
        a, b = ((oo + pad) * inv).astype(F), ((oo - pad) * inv).astype(F)
        tlimit = F(np.sqrt(q2) * F(1.0000153) + F(4.0) * pad) if q2 < 3.0e38 else F(3.4e38)
        stack, node, need = [], 0, 0
        while node is not None:
            q = n4[node]
            with np.errstate(all="ignore"):
                lo = [_fma32(q[8 * ax:8 * ax + 4], inv[ax], -a[ax]) for ax in range(3)]
                hi = [_fma32(q[8 * ax + 4:8 * ax + 8], inv[ax], -b[ax]) for ax in range(3)]
                tn = np.fmax(np.fmax(np.fmin(lo[0], hi[0]), np.fmin(lo[1], hi[1])), np.fmax(np.fmin(lo[2], hi[2]), F(0.0)))
                tf = np.fmin(np.fmin(np.fmax(lo[0], hi[0]), np.fmax(lo[1], hi[1])), np.fmin(np.fmax(lo[2], hi[2]), tlimit))
                key = np.where(tn <= (tf * F(1.0000005)).astype(F), tn, inf)
            kr = [[key[c], int(refs[node, c])] for c in range(4)]
            for i, j in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
                if kr[j][0] < kr[i][0]:
                    kr[i], kr[j] = kr[j], kr[i]
            stack += [ref for k, ref in (kr[3], kr[2], kr[1]) if k < inf]
            node = kr[0][1] if kr[0][0] < inf else (stack.pop() if stack else None)
            while node is not None and node < 0:
                node = stack.pop() if stack else None
            need = max(need, len(stack))
        out.append(need)
    return np.array(out, np.int64)


def need_histogram(need):
    return {int(v): int(c) for v, c in zip(*np.unique(need, return_counts=True))}
