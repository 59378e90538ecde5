"""The two-level tree of a scene with placed copies, restated (HIP-free): what the top-level builders are fed, and the
read-back cut into the trees it is made of.

    place_copy      prt_scene.cpp place_copy / bvh_gpu.hip k_place_copies, which state the same fp32 expressions: the 8
                    corners of the mesh box through (M[a] x + M[4+a] y) + (M[8+a] z + M[12+a]), their min / max and the
                    largest magnitude `mag`, the pad 1e-5f * (mag + 1e-30f) on both sides
    instance_boxes  the boxes of build_instance_table in instance order: the identity instance of the world meshes first
                    (it carries the root box of their vertices), then every placed copy
    box_triangles   the degenerate triangle (mn, mx, (mn.x, mx.y, mn.z)) per box that build_top_level hands the builders
    split_read_back bvh_read8() + bvh_read()[1] + instances_read() + top_nodes -> the top level, the world meshes' tree and
                    one tree per instanced mesh, each with child_base / tri_base relative again and its own records, so
                    that ploc_replay.canonical applies
    requantize      a refit: the topology of a canonical tree kept, its boxes bottom-up from new leaf boxes, the exact
                    quantization (util.grid_exponent / util.grid_planes)"""
import numpy as np

import util

F = np.float32
FLT_MAX = F(3.402823466e+38)


def mesh_triangles(mesh):
    """[n, 3, 3] in face order: what prt_flatten_mesh makes of a mesh."""
    return np.ascontiguousarray(mesh.GetVertices()[mesh.GetIndices().astype(np.int64)], F)


def place_copy(mat, bmn, bmx):
    """The world box [6] of a copy with the column-major mat4 `mat` of a mesh whose box is bmn .. bmx, one fp32 operation
    at a time (neither side contracts to FMA)."""
    M = np.asarray(mat, F).reshape(16)
    bmn, bmx = np.asarray(bmn, F), np.asarray(bmx, F)
    mn, mx, mag = np.full(3, FLT_MAX, F), np.full(3, -FLT_MAX, F), F(0.0)
    for corner in range(8):
        p = [bmx[0] if corner & 1 else bmn[0], bmx[1] if corner & 2 else bmn[1], bmx[2] if corner & 4 else bmn[2]]
        for a in range(3):
            wv = F(F(F(M[a] * p[0]) + F(M[4 + a] * p[1])) + F(F(M[8 + a] * p[2]) + M[12 + a]))
            mn[a], mx[a], mag = min(mn[a], wv), max(mx[a], wv), max(mag, abs(wv))
    pad = F(F(1e-5) * F(mag + F(1e-30)))
    return np.concatenate([(mn - pad).astype(F), (mx + pad).astype(F)])


def instance_boxes(scene):
    """[n_instances, 6] fp32, in instance order (the world meshes' identity instance first, if there are world meshes)."""
    out = []
    if scene.meshes:
        v = np.concatenate([mesh_triangles(m).reshape(-1, 3) for m, _ in scene.meshes])
        out.append(np.concatenate([v.min(axis=0), v.max(axis=0)]))
    boxes = [mesh_triangles(m).reshape(-1, 3) for m in scene.instanced_meshes]
    boxes = [(v.min(axis=0), v.max(axis=0)) for v in boxes]
    for inst in scene.instances:
        out.append(place_copy(inst.mat[:], *boxes[inst.mesh]))
    return np.asarray(out, F).reshape(-1, 6)


def box_triangles(boxes):
    """[n, 3, 3]: per box the triangle (mn, mx, (mn.x, mx.y, mn.z))."""
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    mn, mx = boxes[:, 0:3], boxes[:, 3:6]
    return np.ascontiguousarray(np.stack([mn, mx, np.stack([mn[:, 0], mx[:, 1], mn[:, 2]], axis=1)], axis=1), F)


def records(tv, ids):
    """Triangle records [n, 12] as the builders write them: {P0, id}, {P1, 0}, {P2, 0}."""
    rec = np.zeros((len(tv), 3, 4), F)
    rec[:, :, :3] = tv
    rec[:, 0, 3] = np.asarray(ids, np.uint32).view(F)
    return rec.reshape(-1, 12)


def split_read_back(n8, tris, T, top_nodes, scene):
    """The parts of a two-level read-back: {"top": (nodes, records, n_prims), "world": ..., ("mesh", k): ...}.  The top
    level's records are made here, in leaf-slot order, from the restated boxes: slot -> instance through slot_instance, a
    record's id = the instance.  The mesh trees lie behind the top level, each from its root to the next one's; `n_prims`
    is what a part's record ids start at (the world triangles carry their full primitive index, a mesh's its faces)."""
    n8, tris = np.asarray(n8), np.asarray(tris)
    slot_instance, roots = T["slot_instance"].astype(np.int64), T["root"].astype(np.int64)
    boxes = instance_boxes(scene)
    assert len(boxes) == len(slot_instance) and sorted(slot_instance.tolist()) == list(range(len(boxes)))
    parts = {"top": (n8[:top_nodes].copy(), records(box_triangles(boxes[slot_instance]), slot_instance), 0)}
    first_placed = 1 if scene.meshes else 0
    starts = sorted(set(roots.tolist()))
    assert starts[0] == top_nodes and len(starts) == first_placed + len(scene.instanced_meshes)
    ends = dict(zip(starts, starts[1:] + [len(n8)]))

    def cut(root, slot_base, n_tris):
        nodes = n8[root:ends[root]].copy()
        nodes[:, 4] -= np.uint32(root)
        nodes[:, 5] -= np.uint32(slot_base)
        return nodes, tris[slot_base:slot_base + n_tris].copy()
    if scene.meshes:
        n_world = sum(m.n_triangles for m, _ in scene.meshes)
        assert int(T["slot_base"][0]) == 0
        parts["world"] = cut(int(roots[0]), 0, n_world) + (len(scene.primitives),)
    for k, inst in enumerate(scene.instances):
        if ("mesh", inst.mesh) in parts:
            continue
        i = first_placed + k
        parts[("mesh", inst.mesh)] = cut(int(roots[i]), int(T["slot_base"][i]), scene.instanced_meshes[inst.mesh].n_triangles) + (0,)
    return parts


def requantize(tree, leaf_boxes):
    """The canonical tree `tree` refitted: topology (imask, meta, tri, child) kept, every node's box the union of the new
    boxes leaf_boxes [n, 6] (by the ids in `tri`) below it, origin / exp / planes by the exact rule."""
    leaf_boxes = np.asarray(leaf_boxes, F).reshape(-1, 6)
    tri, child = tree["tri"], tree["child"]
    N = len(child)
    inner, leaf = child >= 0, (tri >= 0).any(axis=2)
    occ = inner | leaf
    slot_lo = np.full((N, 8, 3), FLT_MAX, F)
    slot_hi = np.full((N, 8, 3), -FLT_MAX, F)
    for k in range(3):
        sel = tri[:, :, k] >= 0
        slot_lo[sel] = np.minimum(slot_lo[sel], leaf_boxes[tri[:, :, k][sel], 0:3])
        slot_hi[sel] = np.maximum(slot_hi[sel], leaf_boxes[tri[:, :, k][sel], 3:6])
    node_lo, node_hi = np.zeros((N, 3), F), np.zeros((N, 3), F)
    for n in range(N - 1, -1, -1):   # (canonical order: children behind their parent)
        s = np.nonzero(inner[n])[0]
        slot_lo[n, s], slot_hi[n, s] = node_lo[child[n, s]], node_hi[child[n, s]]
        node_lo[n], node_hi[n] = slot_lo[n, occ[n]].min(axis=0), slot_hi[n, occ[n]].max(axis=0)
    e = util.grid_exponent(node_lo, node_hi)
    o3 = occ[:, :, None]
    qlo, qhi = util.grid_planes(node_lo[:, None, :], e[:, None, :], np.where(o3, slot_lo, node_lo[:, None, :]), np.where(o3, slot_hi, node_lo[:, None, :]))
    qlo, qhi = np.where(o3, qlo, 255.0), np.where(o3, qhi, 0.0)
    assert qhi.max() <= 255.0
    out = {k: np.asarray(v).copy() for k, v in tree.items()}
    out.update(origin=node_lo.copy().view(np.uint32), exp=e, planes=np.concatenate([qlo.transpose(0, 2, 1), qhi.transpose(0, 2, 1)], axis=1).astype(np.int64))
    return out
