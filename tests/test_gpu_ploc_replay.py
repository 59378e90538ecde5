"""Device-built trees held to the builder's own algorithm and to tight boxes.

gpu_build 1 (PLOC + optimal collapse, csrc/bvh_gpu.hip): the tree read back must EQUAL tests/ploc_replay.py's numpy
restatement of the builder, field by field, up to node and slot numbering (child_base / tri_base come from atomics).
The closest hit does not depend on the tree, so hits alone cannot see a wrong window, a non-optimal collapse or a loose
box; this can.  The inputs are the smallest that reach each path of the builder (see INPUTS).  Every builder's tree
(gpu_build 0, 1, 2) must also have the tightest boxes its format allows (util.check_bvh8_tight).

gpu_build 2 (the Morton octree) is held to its own restatement in tests/test_gpu_octree_replay.py, and the two-level
rows (the top-level tree of a scene with placed copies, leaf_cost 64; the mesh trees behind it; the top level after a
refit or a rebuild) in tests/test_gpu_two_level_replay.py."""
import numpy as np
import pytest

import ploc_replay as pr
from builder_inputs import bunny as _bunny, coplanar as _coplanar, grid as _grid, ico as _ico, tiny as _tiny
from builder_inputs import build as _build, check_tree as _check_tree, prepare as _prepare

pytestmark = pytest.mark.gpu
F = np.float32


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
    "bunny": (_bunny, 1),
}
_cache = {}   # name -> dict(tv, scene, binaries, want hits): built once per input


def _input(name):
    if name not in _cache:
        _cache[name] = _prepare(INPUTS[name][0]())
    return _cache[name]


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
