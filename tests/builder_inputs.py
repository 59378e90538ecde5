"""Inputs of the builder tests (test_gpu_ploc_replay.py, test_octree_replay.py, test_gpu_octree_replay.py,
test_gpu_two_level_replay.py): triangle soups that reach one path of a builder each, and the mesh that carries them."""
import numpy as np

import util
from util import prt

F = np.float32


def soup(tv):
    """A mesh of the triangles tv [n, 3, 3], in that order."""
    tv = np.ascontiguousarray(tv, F)
    n = len(tv)
    e1, e2 = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    nrm = np.cross(e1, e2).astype(np.float64)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.maximum(ln, 1e-300), np.asarray([0.0, 1.0, 0.0]))
    return prt.Mesh(vertices=tv.reshape(-1, 3), normals=np.repeat(nrm, 3, axis=0).astype(F),
                    indices=np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))


def triangles(mesh):
    return mesh.GetVertices()[mesh.GetIndices().astype(np.int64)]


def ico(n_refined, n_keep=None):
    tv = triangles(prt.scenes.refined("icosahedron.ply", n_refined))
    return tv if n_keep is None else tv[:n_keep]


def tiny(n):
    rng = np.random.default_rng(n)
    return (rng.uniform(-0.8, 0.8, (n, 1, 3)) + rng.normal(size=(n, 3, 3)) * 0.05).astype(F)


def grid():
    """70 x 70 equal quads of side 1/32 in the plane y = 0.25 (9 800 triangles): every pair of neighbours has the same area."""
    i, j = np.meshgrid(np.arange(70), np.arange(70), indexing="ij")
    x0, z0 = (i.ravel() / 32.0 - 1.0), (j.ravel() / 32.0 - 1.0)
    d, y = 1.0 / 32.0, np.full(4900, 0.25)
    p00, p10, p01, p11 = (np.stack([x0 + a, y, z0 + b], axis=1) for a, b in ((0, 0), (d, 0), (0, d), (d, d)))
    return np.stack([np.stack([p00, p10, p11], axis=1), np.stack([p00, p11, p01], axis=1)], axis=1).reshape(-1, 3, 3).astype(F)


def coplanar():
    rng = np.random.default_rng(77)
    tv = (rng.uniform(-1, 1, (5000, 1, 3)) + rng.normal(size=(5000, 3, 3)) * 0.03).astype(F)
    tv[:, :, 1] = F(0.0)
    return tv


def bunny():
    return triangles(prt.Mesh(prt.scenes.asset("bunny.ply")))


def around(c, d=2.0 ** -14):
    """One triangle per row of c [n, 3] whose fp32 bounds are c -+ d on every axis: its centroid, 0.5f lo + 0.5f hi, is c
    exactly where c -+ d are fp32 values."""
    c = np.asarray(c, np.float64)
    o = np.asarray([[-d, -d, -d], [d, -d, d], [-d, d, d]])
    tv = (c[:, None, :] + o[None, :, :]).astype(F)
    assert np.array_equal(tv.astype(np.float64), c[:, None, :] + o[None, :, :])
    return tv


def two_clusters():
    """4 + 4 triangles in opposite corners of the centroid bounds [-1, 1]^3 (finest Morton cell: 2^-9).  Each cluster lies
    in one column of finest cells: one cell in x and y, four consecutive cells along z.  The root splits into slots 0 and
    7; below each, seven levels do not split the range and are skipped; the next separates the cells 0, 1 from 2, 3."""
    cell = 2.0 ** -9
    a = np.asarray([[0.0, 0.0, 0.0], [0.25, 0.25, 1.5], [0.5, 0.25, 2.5], [0.25, 0.5, 3.5]]) * cell - 1.0
    b = 1.0 - np.asarray([[0.0, 0.0, 0.0], [0.25, 0.25, 1.5], [0.5, 0.25, 2.5], [0.25, 0.5, 3.5]]) * cell
    return around(np.concatenate([a, b]))


def dup(n):
    return np.tile(tiny(1), (n, 1, 1))


def dup_in_mesh():
    tv = ico(300)
    return np.concatenate([tv[:100], np.tile(tv[17:18], (40, 1, 1)), tv[100:]])


def prepare(tv):
    """What the tests of one input share, built once: the triangles, their scene, 2 000 rays and the oracle's closest hits."""
    tv = np.ascontiguousarray(tv, F)
    scene = prt.scenes.mesh_scene(soup(tv))
    rng = np.random.default_rng(31)
    o1, d1 = util.random_rays(rng, 1000, center=(0, 0, 0), radius=9.0, spread=1.0)
    o2 = rng.uniform(-1, 1, size=(1000, 3)).astype(F)
    d2 = np.stack([prt.glm_normalize(v) for v in rng.normal(size=o2.shape).astype(F)])
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=len(tv) > 3000, n_threads=8)
    return dict(tv=tv, scene=scene, binaries={}, o=o, d=d, want=want)


def build(scene, builder=1):
    r = prt.HipWavefrontRenderer(device=0)
    r.set_param("gpu_build", builder)
    r.Init(prt.Film(16, 16), scene, prt.Camera(width=16, height=16))
    assert r.bvh_info().built_on_device == (1 if builder else 0)
    return r


def check_tree(r, c):
    """What every builder test asks of a tree: valid, tight, complete, and 2 000 closest hits equal to the oracle's."""
    n8 = r.bvh_read8()
    _, tris = r.bvh_read()
    _, depth = util.check_bvh8(n8, tris)
    assert depth == r.bvh_info().depth8
    assert util.check_bvh8_tight(n8, tris) == len(n8)
    n_prims = len(c["scene"].primitives)
    ids = tris[:, 3].copy().view(np.uint32).astype(np.int64) - n_prims
    assert sorted(ids.tolist()) == list(range(len(c["tv"])))
    assert np.array_equal(tris.reshape(-1, 3, 4)[np.argsort(ids), :, :3], c["tv"])   # the records hold the input's vertices
    assert util.hits_equal(r.closest_hit(c["o"], c["d"]), c["want"]) == []
    return n8, tris, n_prims


# The Morton octree builder's inputs: name -> (triangles, what octree_replay's info must say the input reached; a number is
# an exact count, a tuple (k,) a minimum).  Checked without a GPU by test_octree_replay.py.
OCTREE_INPUTS = {
    "tri1": (lambda: tiny(1), dict(n_nodes=1, skipped_levels=0, flat_axes=3, index_splits_small=0, index_splits_8=0)),
    "tri3": (lambda: tiny(3), dict(n_nodes=1, skipped_levels=0, flat_axes=0, clamped_1023=3, index_splits_small=0, index_splits_8=0)),
    "tri4": (lambda: tiny(4), dict(n_nodes=1, flat_axes=0, clamped_1023=3, index_splits_small=0, index_splits_8=0)),
    "tri9": (lambda: tiny(9), dict(n_nodes=1, flat_axes=0, index_splits_small=0, index_splits_8=0)),
    # (these nine fall into leaves of the root alone; ten are the fewest of this family with an internal child beside leaves)
    "tri10": (lambda: tiny(10), dict(n_nodes=2, leaf_slots_beside_internal=1, index_splits_small=0, index_splits_8=0)),
    "two_clusters": (two_clusters, dict(n_nodes=3, skipped_levels=14, index_splits_small=0, index_splits_8=0, clamped_1023=(3,))),
    "dup10": (lambda: dup(10), dict(n_nodes=1, skipped_levels=10, flat_axes=3, index_splits_small=1, index_splits_8=0)),
    "dup30": (lambda: dup(30), dict(n_nodes=7, skipped_levels=10, flat_axes=3, index_splits_small=6, index_splits_8=1)),
    "dup_in_mesh": (dup_in_mesh, dict(index_splits_8=1, index_splits_small=(1,), skipped_levels=(1,), flat_axes=0)),
    "coplanar": (coplanar, dict(flat_axes=1, n_nodes=(129,), index_splits_8=0)),
    "grid70": (grid, dict(flat_axes=1, n_nodes=(129,), index_splits_8=0)),
    "ico4400": (lambda: ico(4400), dict(flat_axes=0, n_nodes=(513,), clamped_1023=(3,))),
    "bunny": (bunny, dict(flat_axes=0, n_nodes=(2049,), clamped_1023=(3,))),
}
