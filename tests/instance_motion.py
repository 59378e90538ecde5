"""Moving placed copies (prt_set_instance_transforms): the scenes, the motion steps and the host-side checks shared by
test_instance_motion_host.py and test_gpu_instance_motion.py.

A motion is a list of (scale, euler_deg, translation) per placed copy; `move` writes it into the scene through
Scene.SetInstanceTransform, so that the description a renderer is updated with and the description a fresh renderer or
the oracle gets are one and the same object."""
import numpy as np

import scale_cases as sc
import util
from util import prt

STEPS = ("jiggle", "permute", "collapse", "random", "back")


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def _srt(rng, scale, center, span):
    return (float(scale * rng.uniform(0.5, 2.0)), tuple(float(v) for v in rng.uniform(-180, 180, 3)),
            tuple(float(v) for v in np.asarray(center) + rng.uniform(-span, span, 3)))


def _place(scene, meshes, mats, srts):
    for k, (s, e, t) in enumerate(srts):
        scene.AddInstance(meshes[k % len(meshes)], mats[k % len(mats)], scale=s, euler_deg=e, translation=t)
    scene.start = list(srts)
    return scene


def scene_a(world=True, emissive=False):
    """A world bunny (optional), 12 copies of the icosahedron and of cube_uv, 3 analytic primitives.  emissive: copy 1 and
    copy 7 emit (triangle lights of placed copies), next to the quad light."""
    rng = np.random.default_rng(41)
    s = prt.Scene(preset=None)
    body, metal, light = s.AddLambertian((0.7, 0.6, 0.5)), s.AddMetal((0.9, 0.9, 0.9), 0.05), s.AddEmissive((6.0, 5.0, 4.0))
    s.AddQuad(40.0, 40.0, body, translation=(0.0, -3.0, 0.0))
    s.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 8.0, 0.0))
    s.AddCircle(0.8, metal, translation=(2.5, -2.2, 1.5))
    if world:
        s.AddMesh(sc.move_mesh(sc.asset_mesh("bunny.ply"), 8.0, (0.0, 0.0, 0.0)), body)
    mats = [body, metal]
    if emissive:
        mats = [body, light, metal, body, metal, body]
    return _place(s, [sc.asset_mesh("icosahedron.ply"), sc.asset_mesh("cube_uv.ply")], mats, [_srt(rng, 0.6, (0, 0, 0), 4.0) for _ in range(12)])


def scene_b():
    """No world mesh: 40 copies of the icosahedron, 8 of them with one and the same transform (coinciding boxes)."""
    rng = np.random.default_rng(42)
    s = prt.Scene(preset=None)
    srts = [_srt(rng, 0.8, (0, 0, 0), 6.0) for _ in range(40)]
    for k in range(8):
        srts[5 * k] = srts[0]
    return _place(s, [sc.asset_mesh("icosahedron.ply", 80)], [s.AddLambertian((0.8, 0.8, 0.8)), s.AddMetal((0.9, 0.9, 0.9), 0.0)], srts)


C_SCALES = (2.0 ** -10, 1.0, 2.0 ** 10)
C_FAR = (1e4, 0.0, -1e4)


def _c_center(k):
    return (0.0, 0.0, 0.0) if k % 2 == 0 else C_FAR


def scene_c():
    """A world bunny and 9 copies at scales 2^-10 / 1 / 2^10 x (0.5 .. 2), around the origin and around a point 1e4 away."""
    rng = np.random.default_rng(43)
    s = prt.Scene(preset=None)
    body = s.AddLambertian((0.7, 0.6, 0.5))
    s.AddMesh(sc.move_mesh(sc.asset_mesh("bunny.ply"), 8.0, (0.0, 0.0, 0.0)), body)
    srts = [_srt(rng, C_SCALES[k % 3], _c_center(k), 4.0 * C_SCALES[k % 3]) for k in range(9)]
    s = _place(s, [sc.asset_mesh("icosahedron.ply", 300)], [body, s.AddMetal((0.9, 0.9, 0.9), 0.05)], srts)
    s.scales = [C_SCALES[k % 3] for k in range(9)]
    return s


SCENES = {"A": scene_a, "B": scene_b, "C": scene_c}


# ---- motions ----------------------------------------------------------------------------------------------------------------
def motion(scene, step, seed=0):
    """The transforms of every placed copy at `step` (one of STEPS), from the scene's starting transforms."""
    start = scene.start
    n = len(start)
    rng = np.random.default_rng([77, STEPS.index(step), seed])
    scales = getattr(scene, "scales", None)
    if step == "jiggle":     # a few percent of a copy's own size, a few degrees
        return [(s, tuple(float(v) for v in np.asarray(e) + rng.uniform(-3, 3, 3)),
                 tuple(float(v) for v in np.asarray(t) + rng.uniform(-0.05, 0.05, 3) * s)) for s, e, t in start]
    if step == "permute":    # the copies exchange places (no copy stays): the worst case for a kept topology
        shift = n // 2 + 1
        return [(start[k][0], start[k][1], start[(k + shift) % n][2]) for k in range(n)]
    if step == "collapse":   # every copy onto the first one's spot
        return [(s, e, start[0][2]) for s, e, _ in start]
    if step == "random":
        if scales:
            return [_srt(rng, scales[k], _c_center(int(rng.integers(0, 2))), 4.0 * scales[k]) for k in range(n)]
        return [_srt(rng, 0.7, (0, 0, 0), 5.0) for _ in range(n)]
    if step == "back":
        return list(start)
    raise ValueError(step)


def move(scene, srts):
    for k, (s, e, t) in enumerate(srts):
        scene.SetInstanceTransform(k, scale=s, euler_deg=e, translation=t)
    return scene


def host_renderer(scene, sources=None):
    r = prt.HipWavefrontRenderer(device=-1)
    if sources:
        r.set_light_sources(sources)
    r.set_scene_host_only(scene)
    return r


# ---- the top level, read back ------------------------------------------------------------------------------------------------
def instance_boxes64(scene):
    """Per instance of the top level (the world meshes' identity instance first, if any): its world box in float64: the 8
    corners of its mesh's box through the copy's (fp32) matrix; for the world meshes the box of their vertices."""
    out = []
    if scene.meshes:
        v = np.concatenate([m.GetVertices().astype(np.float64) for m, _ in scene.meshes])
        out.append((v.min(axis=0), v.max(axis=0)))
    for inst in scene.instances:
        v = scene.instanced_meshes[inst.mesh].GetVertices().astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        corners = np.array([[(hi if (c >> a) & 1 else lo)[a] for a in range(3)] for c in range(8)])
        M = np.array(inst.mat[:], np.float64).reshape(4, 4).T
        w = corners @ M[:3, :3].T + M[:3, 3]
        out.append((w.min(axis=0), w.max(axis=0)))
    return out


def check_top_level(r, scene):
    """The top-level tree of `r` (prt_bvh_read8's first top_nodes nodes + prt_instances_read) is a valid tree over the
    instances of `scene`: every node reached once, every leaf slot in exactly one leaf, slot -> instance a permutation, and
    every quantized child box contains the float64 world box of every instance below it.  Returns (D, T, levels)."""
    n8 = r.bvh_read8()
    info = r.instance_update_info()
    T = r.instances_read()
    n_inst = len(scene.instances) + (1 if scene.meshes else 0)
    assert len(T["slot_instance"]) == n_inst and sorted(T["slot_instance"].tolist()) == list(range(n_inst))
    n_top = info.top_nodes
    assert 0 < n_top < len(n8) == r.bvh_info().n_nodes8
    D = util.decode8(n8[:n_top])
    boxes = instance_boxes64(scene)
    seen = np.zeros(n_top, np.int32)
    covered = np.zeros(n_inst, np.int32)

    def below(n, level):
        """(exact lo, exact hi, levels) of everything below node n."""
        seen[n] += 1
        lo, hi, depth, rank = np.full(3, np.inf), np.full(3, -np.inf), level, 0
        for i in range(8):
            meta = int(D["meta"][n, i])
            if meta == 0:
                assert not (D["imask"][n] >> i) & 1
                continue
            if (D["imask"][n] >> i) & 1:
                c = int(D["child_base"][n]) + rank
                rank += 1
                assert 0 < c < n_top, (n, c, n_top)
                clo, chi, cd = below(c, level + 1)
                depth = max(depth, cd)
            else:
                cnt = bin(meta >> 5).count("1")
                first = int(D["tri_base"][n]) + (meta & 31)
                assert (meta >> 5) in (1, 3, 7) and first + cnt <= n_inst
                covered[first:first + cnt] += 1
                members = [boxes[int(T["slot_instance"][sl])] for sl in range(first, first + cnt)]
                clo, chi = np.min([m[0] for m in members], axis=0), np.max([m[1] for m in members], axis=0)
            assert (clo >= D["lo"][n, i]).all() and (chi <= D["hi"][n, i]).all(), (n, i, clo, chi, D["lo"][n, i], D["hi"][n, i])
            lo, hi = np.minimum(lo, clo), np.maximum(hi, chi)
        return lo, hi, depth
    _, _, levels = below(0, 1)
    assert (seen == 1).all() and (covered == 1).all()
    assert levels == info.top_depth
    # every instance's root lies behind the top level, and two copies of one mesh share it
    roots = T["root"]
    assert (roots >= n_top).all() and (roots < len(n8)).all()
    first_placed = 1 if scene.meshes else 0
    by_mesh = {}
    for k, inst in enumerate(scene.instances):
        by_mesh.setdefault(inst.mesh, set()).add(int(roots[first_placed + k]))
    assert all(len(v) == 1 for v in by_mesh.values())
    return n8, T, levels


def _slab(lo, hi, o, inv, pad):
    near = np.where(inv < 0, hi + pad, lo - pad)
    far = np.where(inv < 0, lo - pad, hi + pad)
    tn = np.maximum(((near - o) * inv).max(axis=1), 0.0)
    tf = ((far - o) * inv).min(axis=1)
    return tn <= tf


def walk_two_level(r, scene, o, d, want):
    """A plain float64 walk of the read-back two-level tree (quantized boxes with a slack far below any box size, the ray
    taken into a copy's space through its inverse matrix): the triangles it reaches include the oracle's winner for every
    ray whose winner is a triangle.  Returns the number of rays checked."""
    n8 = r.bvh_read8()
    T = r.instances_read()
    _, tris = r.bvh_read()
    D = util.decode8(n8)
    n_top = r.instance_update_info().top_nodes
    n_prims = len(scene.primitives)
    face = tris[:, 3].copy().view(np.uint32).astype(np.int64)
    first_placed = 1 if scene.meshes else 0
    inv_m = [np.array(i.inv[:], np.float64).reshape(4, 4).T for i in scene.instances]
    extent = max(float(np.abs(np.array(b)).max()) for b in instance_boxes64(scene))

    def leaves(root, oo, dd, pad, top):
        inv = 1.0 / np.where(np.abs(dd) < 1e-300, 1e-300, dd)
        out, stack = [], [root]
        while stack:
            n = stack.pop()
            assert (n < n_top) == top
            hit = _slab(D["lo"][n], D["hi"][n], oo, inv, pad)
            rank = 0
            for i in range(8):
                meta = int(D["meta"][n, i])
                if meta == 0:
                    continue
                inner = (D["imask"][n] >> i) & 1
                if inner:
                    c = int(D["child_base"][n]) + rank
                    rank += 1
                if not hit[i]:
                    continue
                if inner:
                    stack.append(c)
                else:
                    first = int(D["tri_base"][n]) + (meta & 31)
                    out += list(range(first, first + bin(meta >> 5).count("1")))
        return out

    checked = 0
    for k in np.nonzero(want["prim"] >= n_prims)[0]:
        ok, dk = o[k].astype(np.float64), d[k].astype(np.float64)
        pad = 1e-5 * (np.abs(ok).sum() + extent)
        reached = set()
        for sl in leaves(0, ok, dk, pad, True):
            inst = int(T["slot_instance"][sl])
            if inst < first_placed:
                lo_, ld_, lpad, base = ok, dk, pad, 0
            else:
                M = inv_m[inst - first_placed]
                lo_, ld_ = M[:3, :3] @ ok + M[:3, 3], M[:3, :3] @ dk
                lpad, base = pad * np.linalg.norm(M[:3, 0]), int(T["prim_base"][inst])
            for ts in leaves(int(T["root"][inst]), lo_, ld_, lpad, False):
                assert int(T["slot_base"][inst]) <= ts < len(face)
                reached.add(base + int(face[ts]))
        assert int(want["prim"][k]) in reached, (k, int(want["prim"][k]))
        checked += 1
    return checked
