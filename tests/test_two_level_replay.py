"""tests/two_level_replay.py on host-only contexts (no GPU): the restated place_copy must give the very boxes the host
builder's top level was built over: util.check_bvh8_tight over the top-level nodes, with the restated boxes' degenerate
triangles in leaf-slot order, has one right answer per plane, so a box one ulp off cannot pass.  The splitter's parts must
be whole trees over their own records, and requantize of a tree with its own boxes must give the tree back."""
import numpy as np
import pytest

import instance_motion as im
import ploc_replay as pr
import two_level_replay as tl
import util

F = np.float32


def _parts(r, scene):
    return tl.split_read_back(r.bvh_read8(), r.bvh_read()[1], r.instances_read(), r.instance_update_info().top_nodes, scene)


def _check(r, scene):
    im.check_top_level(r, scene)
    parts = _parts(r, scene)
    assert set(parts) == {"top"} | ({"world"} if scene.meshes else set()) | {("mesh", i.mesh) for i in scene.instances}
    for name, (nodes, recs, n_prims) in parts.items():
        _, depth = util.check_bvh8(nodes, recs)
        assert util.check_bvh8_tight(nodes, recs) == len(nodes), name
        ids = recs[:, 3].copy().view(np.uint32).astype(np.int64) - n_prims
        assert sorted(ids.tolist()) == list(range(len(recs))), name
        if name == "top":
            assert depth == r.instance_update_info().top_depth
    # the records of a mesh tree hold that mesh's vertices, those of the world tree the world meshes'
    for k, mesh in enumerate(scene.instanced_meshes):
        nodes, recs, _ = parts[("mesh", k)]
        ids = recs[:, 3].copy().view(np.uint32).astype(np.int64)
        assert np.array_equal(recs.reshape(-1, 3, 4)[np.argsort(ids), :, :3], tl.mesh_triangles(mesh))
    return parts


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_host_built_top_level_is_tight_against_the_restated_boxes(name):
    scene = im.SCENES[name]()
    r = im.host_renderer(scene)
    first = _check(r, scene)
    for step in ("jiggle", "random", "collapse"):
        im.move(scene, im.motion(scene, step))
        r.UpdateInstances(scene, "rebuild")
        parts = _check(r, scene)
        for key in parts:   # the mesh trees, relative again, are what they were
            if key != "top":
                assert np.array_equal(parts[key][0], first[key][0]) and np.array_equal(parts[key][1], first[key][1]), (step, key)


def test_restated_boxes_contain_the_float64_boxes_and_differ_from_them():
    """The pad is part of the restatement: without it the boxes would be the rounded float64 ones, and tightness against
    those is NOT what the library builds over."""
    scene = im.scene_c()
    got = tl.instance_boxes(scene)
    want = im.instance_boxes64(scene)
    assert len(got) == len(want) == 10
    for g, (lo, hi) in zip(got[1:], want[1:]):
        assert (g[0:3] < lo).all() and (g[3:6] > hi).all()
        mag = max(np.abs(lo).max(), np.abs(hi).max())
        assert (lo - g[0:3] <= 2.1e-5 * mag).all() and (g[3:6] - hi <= 2.1e-5 * mag).all()
    assert np.array_equal(got[0, 0:3].astype(np.float64), want[0][0]) and np.array_equal(got[0, 3:6].astype(np.float64), want[0][1])
    t = tl.box_triangles(got)
    assert np.array_equal(t.min(axis=1), got[:, 0:3]) and np.array_equal(t.max(axis=1), got[:, 3:6])
    assert np.array_equal(t[:, 2], np.stack([got[:, 0], got[:, 4], got[:, 2]], axis=1))


@pytest.mark.parametrize("name", ["A", "B"])
def test_requantize_with_a_trees_own_boxes_gives_the_tree_back_and_follows_moved_boxes(name):
    scene = im.SCENES[name]()
    r = im.host_renderer(scene)
    nodes, recs, _ = _parts(r, scene)["top"]
    tree = pr.canonical(nodes, recs, 0)
    boxes = tl.instance_boxes(scene)
    pr.assert_same_tree(tl.requantize(tree, boxes), tree, "own boxes")
    # moved boxes over the kept topology: a valid tree with the tightest boxes over the moved records
    im.move(scene, im.motion(scene, "random"))
    moved = tl.instance_boxes(scene)
    assert not np.array_equal(moved, boxes)
    refit = tl.requantize(tree, moved)
    for f in ("imask", "meta", "tri", "child"):
        assert np.array_equal(refit[f], tree[f])
    n8, rec = pr.as_read_back(refit, tl.box_triangles(moved), n_prims=0)
    util.check_bvh8(n8, rec)
    assert util.check_bvh8_tight(n8, rec) == len(n8)
    with pytest.raises(AssertionError):
        pr.assert_same_tree(refit, tree)
    # shrunk copies: every box of the refit lies inside the one before (a refit tightens as well as grows)
    scene = im.SCENES[name]()
    im.move(scene, [(s * 0.25, e, t) for s, e, t in scene.start])
    small = tl.requantize(tree, tl.instance_boxes(scene))
    D0, D1 = util.decode8(pr.as_read_back(tree, tl.box_triangles(boxes), 0)[0]), util.decode8(pr.as_read_back(small, tl.box_triangles(boxes), 0)[0])
    occ = D0["meta"] != 0
    assert (D1["hi"][occ] - D1["lo"][occ] <= D0["hi"][occ] - D0["lo"][occ]).all()
    assert (D1["hi"][occ] - D1["lo"][occ] < D0["hi"][occ] - D0["lo"][occ]).any()


def test_no_finite_box_overflows_a_nodes_grid():
    """Why test_gpu_two_level_replay.py has no refit step that falls back to a rebuild: the fall-back needs a box that does
    not fit its node's grid (cell exponent above 126, or a plane above 255), and finite fp32 bounds never produce one."""
    big = np.finfo(F).max
    lo = np.asarray([-big, -big, 0.0, big / 2, -1e-38, -big], F)
    hi = np.asarray([big, -big / 2, big, big, big, 1e-38], F)
    e = util.grid_exponent(lo, hi)
    assert (e <= 126).all() and e.max() >= 120
    for inner_lo, inner_hi in ((lo, hi), (hi, hi), (lo, lo)):
        qlo, qhi = util.grid_planes(lo, e, inner_lo, inner_hi)
        assert (qlo >= 0).all() and (qhi <= 255).all() and (qlo <= qhi).all()
