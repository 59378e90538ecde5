"""Device-built trees held to the builder's own algorithm and to tight boxes.

gpu_build 1 (PLOC + optimal collapse, csrc/bvh_gpu.hip): the tree read back must EQUAL tests/ploc_replay.py's numpy
restatement of the builder, field by field, up to node and slot numbering (child_base / tri_base come from atomics).
The closest hit does not depend on the tree, so hits alone cannot see a wrong window, a non-optimal collapse or a loose
box; this can.  The inputs are the smallest that reach each path of the builder (see INPUTS).  Every builder's tree
(gpu_build 0, 1, 2) must also have the tightest boxes its format allows (util.check_bvh8_tight).

The two-level row of the issue (the top-level tree of a scene with placed copies, leaf_cost 64) is not here: the
top-level tree's input is the copies' world boxes as the scene compiler places them, which the read-back does not hand
out in input order; prt_instances_read would have to be combined with a restatement of place_copy.  Left for later."""
import numpy as np
import pytest

import ploc_replay as pr
import util
from util import prt

pytestmark = pytest.mark.gpu
F = np.float32


def _soup(tv):
    """A mesh of the triangles tv [n, 3, 3], in that order."""
    tv = np.ascontiguousarray(tv, F)
    n = len(tv)
    e1, e2 = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    nrm = np.cross(e1, e2).astype(np.float64)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.maximum(ln, 1e-300), np.asarray([0.0, 1.0, 0.0]))
    return prt.Mesh(vertices=tv.reshape(-1, 3), normals=np.repeat(nrm, 3, axis=0).astype(F),
                    indices=np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))


def _triangles(mesh):
    return mesh.GetVertices()[mesh.GetIndices().astype(np.int64)]


def _ico(n_refined, n_keep=None):
    tv = _triangles(prt.scenes.refined("icosahedron.ply", n_refined))
    return tv if n_keep is None else tv[:n_keep]


def _tiny(n):
    rng = np.random.default_rng(n)
    return (rng.uniform(-0.8, 0.8, (n, 1, 3)) + rng.normal(size=(n, 3, 3)) * 0.05).astype(F)


def _grid():
    """70 x 70 equal quads of side 1/32 in the plane y = 0.25 (9 800 triangles): every pair of neighbours has the same area."""
    i, j = np.meshgrid(np.arange(70), np.arange(70), indexing="ij")
    x0, z0 = (i.ravel() / 32.0 - 1.0), (j.ravel() / 32.0 - 1.0)
    d, y = 1.0 / 32.0, np.full(4900, 0.25)
    p00, p10, p01, p11 = (np.stack([x0 + a, y, z0 + b], axis=1) for a, b in ((0, 0), (d, 0), (0, d), (d, d)))
    return np.stack([np.stack([p00, p10, p11], axis=1), np.stack([p00, p11, p01], axis=1)], axis=1).reshape(-1, 3, 3).astype(F)


def _coplanar():
    rng = np.random.default_rng(77)
    tv = (rng.uniform(-1, 1, (5000, 1, 3)) + rng.normal(size=(5000, 3, 3)) * 0.03).astype(F)
    tv[:, :, 1] = F(0.0)
    return tv


# name -> (triangles, windowed passes the input must take: a set, or a minimum)
INPUTS = {
    "tri1": (lambda: _tiny(1), {0}), "tri2": (lambda: _tiny(2), {0}), "tri3": (lambda: _tiny(3), {0}),
    "tri4": (lambda: _tiny(4), {0}), "tri9": (lambda: _tiny(9), {0}),
    "ico300": (lambda: _ico(300), {0}),                        # full search only, two 256-wide trips
    "ico4097": (lambda: _ico(4700, 4097), {1}),                # exactly one windowed pass; the last block holds 1 cluster
    "ico4353": (lambda: _ico(4700, 4096 + 256 + 1), {1, 2}),   # 4096 + 256 k + 1
    "ico4400": (lambda: _ico(4400), {1, 2}),
    "ico20000": (lambda: _ico(20000), 5),                      # five or more windowed passes, many blocks
    "grid70": (_grid, 1),                                      # all areas tie: the tie key, in both searches
    "copies4": (lambda: np.tile(_ico(1250), (4, 1, 1)), 1),    # 1 250 distinct triangles, four copies each
    "coplanar": (_coplanar, 1),                                # zero extent on y: exponent -126, area products of 0
    "bunny": (lambda: _triangles(prt.Mesh(prt.scenes.asset("bunny.ply"))), 1),
}
_cache = {}   # name -> dict(tv, scene, binaries, want hits): built once per input


def _input(name):
    if name not in _cache:
        tv = np.ascontiguousarray(INPUTS[name][0](), F)
        scene = prt.scenes.mesh_scene(_soup(tv))
        rng = np.random.default_rng(31)
        o1, d1 = util.random_rays(rng, 1000, center=(0, 0, 0), radius=9.0, spread=1.0)
        o2 = rng.uniform(-1, 1, size=(1000, 3)).astype(F)
        d2 = np.stack([prt.glm_normalize(v) for v in rng.normal(size=o2.shape).astype(F)])
        o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
        want = util.oracle_scene(scene).closest_hit(o, d, use_bvh=len(tv) > 3000, n_threads=8)
        _cache[name] = dict(tv=tv, scene=scene, binaries={}, o=o, d=d, want=want)
    return _cache[name]


def _build(scene, builder=1):
    r = prt.HipWavefrontRenderer(device=0)
    r.set_param("gpu_build", builder)
    r.Init(prt.Film(16, 16), scene, prt.Camera(width=16, height=16))
    assert r.bvh_info().built_on_device == (1 if builder else 0)
    return r


def _check_tree(r, c):
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


def _set_env(monkeypatch, top="host", radius=None, ci=None):
    for name, value in (("PRT_PLOC_TOP", "device" if top == "device" else None), ("PRT_PLOC_RADIUS", radius), ("PRT_PLOC_CI", ci)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def _replay(c, top="host", radius=24, ci=0.6, info=None):
    return pr.replay(c["tv"], *pr.centroid_bounds(c["tv"]), radius=radius, ci=ci, top=top, info=info, binaries=c["binaries"])


def _run(monkeypatch, name, top="host", radius=None, ci=None):
    c = _input(name)
    _set_env(monkeypatch, top, radius, ci)
    r = _build(c["scene"])
    n8, tris, n_prims = _check_tree(r, c)
    info = {}
    want = _replay(c, top, 24 if radius is None else radius, 0.6 if ci is None else float(F(ci)), info)
    passes = INPUTS[name][1] if radius is None else 1   # (the table's pass counts are for the default radius)
    assert info["windowed_passes"] in passes if isinstance(passes, set) else info["windowed_passes"] >= passes, info
    assert (info["full_passes"] > 0) == (top == "device" and len(c["tv"]) > 1)
    pr.assert_same_tree(pr.canonical(n8, tris, n_prims), want, f"{name}, top on the {top}, radius {radius}, ci {ci}")
    return want


@pytest.mark.parametrize("top", ["host", "device"])
@pytest.mark.parametrize("name", list(INPUTS))
def test_quality_builder_tree_equals_the_replay(name, top, monkeypatch):
    _run(monkeypatch, name, top)


@pytest.mark.parametrize("radius,ci", [(1, None), (64, None), (None, "0.1"), (None, "4.0")])
def test_quality_builder_tree_equals_the_replay_under_the_tunables(radius, ci, monkeypatch):
    c = _input("ico20000")
    got = _run(monkeypatch, "ico20000", "host", radius, ci)
    default = _replay(c)
    assert len(got["imask"]) != len(default["imask"]) or any(not np.array_equal(got[f], default[f]) for f in pr.FIELDS)


def test_tunables_mean_what_the_environment_says_at_each_build(monkeypatch):
    """PRT_PLOC_TOP / PRT_PLOC_RADIUS were sticky: once set in a process, deleting the variable kept the last value.  Build
    with the variable set, delete it, build again in the same process: the second tree is the DEFAULT's."""
    c = _input("ico4400")
    default = _replay(c)
    for kw in (dict(top="device"), dict(radius=1)):
        other = _run(monkeypatch, "ico4400", **kw)
        assert len(other["imask"]) != len(default["imask"]) or any(not np.array_equal(other[f], default[f]) for f in pr.FIELDS)
        _run(monkeypatch, "ico4400")             # every variable deleted
        monkeypatch.setenv("PRT_PLOC_TOP", "")   # empty counts as unset
        monkeypatch.setenv("PRT_PLOC_RADIUS", "")
        monkeypatch.setenv("PRT_PLOC_CI", "")
        r = _build(c["scene"])
        pr.assert_same_tree(pr.canonical(r.bvh_read8(), r.bvh_read()[1], len(c["scene"].primitives)), default, "empty variables")


@pytest.mark.parametrize("builder", [0, 1, 2])
@pytest.mark.parametrize("name", ["tri1", "tri9", "ico300", "ico4353", "ico20000", "grid70", "copies4", "coplanar", "bunny"])
def test_every_builder_gives_tight_boxes(name, builder, monkeypatch):
    c = _input(name)
    _set_env(monkeypatch)
    _check_tree(_build(c["scene"], builder), c)
