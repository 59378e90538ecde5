"""tests/octree_replay.py against independent statements of what the Morton octree builder is FOR, on inputs small enough
for brute force (CPU only).  The replay is the yardstick the device-built trees are held to (tests/test_gpu_octree_replay.py,
tests/test_gpu_two_level_replay.py); these tests keep it from being a transliteration that shares a bug with the source,
show that the comparison sees the faults it is for, and check that every input of the GPU table reaches what it is there for."""
import numpy as np
import pytest

import builder_inputs as bi
import octree_replay as oc
import ploc_replay as pr
import util

F = np.float32


# ---- a brute-force octree: cells, no sorted array, no search -----------------------------------------------------------------
def _grid_coordinates(tv):
    """The three 10-bit grid coordinates of every triangle, read out of its code bit by bit."""
    raw = pr.morton_codes(tv, *pr.centroid_bounds(tv)).astype(np.int64)
    return np.stack([sum(((raw >> (3 * b + a)) & 1) << b for b in range(10)) for a in range(3)], axis=1)


def _brute_force(q, members, level):
    """The node over the triangles `members` (input indices) whose cell at `level` is common: slot -> a frozenset of at
    most 3 triangles (a leaf) or a nested node.  Levels at which one cell holds everything are dropped; below the finest
    level the members, in index order, are cut into parts of floor(count * c / parts)."""
    members = sorted(members)
    count = len(members)
    if count <= 3:
        return {0: frozenset(members)}
    while level < 10:
        bit = 9 - level
        cells = {}
        for t in members:
            digit = (((q[t, 2] >> bit) & 1) << 2) | (((q[t, 1] >> bit) & 1) << 1) | ((q[t, 0] >> bit) & 1)
            cells.setdefault(int(digit), []).append(t)
        level += 1
        if len(cells) >= 2:
            break
    else:
        parts = -(-count // 3) if count <= 24 else 8
        cells = {c: members[count * c // parts:count * (c + 1) // parts] for c in range(parts)}
    return {s: frozenset(m) if len(m) <= 3 else _brute_force(q, m, level) for s, m in cells.items()}


def _partition(tree, n=0):
    """The replayed canonical tree in the nested form of _brute_force."""
    out = {}
    for s in range(8):
        if tree["child"][n, s] >= 0:
            out[s] = _partition(tree, int(tree["child"][n, s]))
        elif tree["meta"][n, s]:
            out[s] = frozenset(int(t) for t in tree["tri"][n, s] if t >= 0)
    return out


def _clustered():
    rng = np.random.default_rng(5)
    return (rng.integers(0, 4, (200, 1, 3)) * 0.5 + rng.normal(size=(200, 3, 3)) * 1e-4).astype(F)   # many shared cells


SMALL = {"tri1": lambda: bi.tiny(1), "tri2": lambda: bi.tiny(2), "tri3": lambda: bi.tiny(3), "tri4": lambda: bi.tiny(4),
         "tri9": lambda: bi.tiny(9), "tri60": lambda: bi.tiny(60), "two_clusters": bi.two_clusters, "dup10": lambda: bi.dup(10),
         "dup25": lambda: bi.dup(25), "dup30": lambda: bi.dup(30), "dup200": lambda: bi.dup(200), "dup_in_mesh": bi.dup_in_mesh,
         "ico300": lambda: bi.ico(300), "clustered": _clustered, "coplanar": lambda: bi.coplanar()[:400]}
_made = {}


def _small(name):
    if name not in _made:
        _made[name] = np.ascontiguousarray(SMALL[name](), F)
    return _made[name]


@pytest.mark.parametrize("name", list(SMALL))
def test_partition_into_nodes_and_slots_equals_the_brute_force_octree(name):
    tv = _small(name)
    tree = oc.replay(tv, *pr.centroid_bounds(tv))
    assert _partition(tree) == _brute_force(_grid_coordinates(tv), range(len(tv)), 0)
    # inside a leaf the triangles stand in sorted order: by code, equal codes by index
    code = pr.morton_codes(tv, *pr.centroid_bounds(tv)).astype(np.int64)
    for t in tree["tri"].reshape(-1, 3):
        t = t[t >= 0]
        key = code[t] * len(tv) + t
        assert (np.diff(key) > 0).all()


def test_the_digit_is_the_octant_of_the_child_in_its_parent():
    """Bit a of a slot = the upper half on axis a: below every node, the centroids in slot s lie on the s side of ONE
    plane per axis (the cell boundary the level cut at), whatever levels were skipped."""
    tv = bi.ico(300)
    tree = oc.replay(tv, *pr.centroid_bounds(tv))
    cen = (F(0.5) * tv.min(axis=1) + F(0.5) * tv.max(axis=1)).astype(np.float64)

    def below(part):
        return sorted(t for v in part.values() for t in (v if isinstance(v, frozenset) else below(v)))

    def check(part):
        sets = {s: (sorted(v) if isinstance(v, frozenset) else below(v)) for s, v in part.items()}
        for a in range(3):
            lower = [cen[t, a] for s, m in sets.items() if not (s >> a) & 1 for t in m]
            upper = [cen[t, a] for s, m in sets.items() if (s >> a) & 1 for t in m]
            assert not lower or not upper or max(lower) < min(upper)
        for v in part.values():
            if not isinstance(v, frozenset):
                check(v)
    check(_partition(tree))


# ---- the whole replay: a valid, tight tree that survives the round trip ------------------------------------------------------
@pytest.mark.parametrize("name", list(SMALL))
def test_replayed_tree_is_valid_tight_and_complete(name):
    tv = _small(name)
    tree = oc.replay(tv, *pr.centroid_bounds(tv))
    n8, tris = pr.as_read_back(tree, tv)
    util.check_bvh8(n8, tris)
    assert util.check_bvh8_tight(n8, tris) == len(n8)
    assert sorted(tree["tri"][tree["tri"] >= 0].tolist()) == list(range(len(tv)))
    pr.assert_same_tree(pr.canonical(n8, tris, 2), tree, "round trip")


# ---- the comparison sees the faults it is for --------------------------------------------------------------------------------
def _parts(tv):
    codes, idx = pr.morton_order(tv, *pr.centroid_bounds(tv))
    return codes, idx, oc.split(codes)


def _swapped_slots(tv):
    """Two occupied slots of one node exchange places (children in the wrong octant)."""
    _, idx, (cf, cc, child) = _parts(tv)
    n = int(np.nonzero((cc > 0).sum(axis=1) >= 2)[0][-1])
    a, b = np.nonzero(cc[n] > 0)[0][:2]
    for x in (cf, cc, child):
        x[n, [a, b]] = x[n, [b, a]]
    return oc.emit(cf, cc, child, idx, tv)


def _x_and_z_exchanged(tv):
    """The digit built as x << 2 | y << 1 | z."""
    codes = pr.morton_codes(tv, *pr.centroid_bounds(tv)).astype(np.int64)
    x, y, z = codes & 0x09249249, codes & 0x12492492, codes & 0x24924924
    wrong = (x << 2) | y | (z >> 2)
    idx = np.argsort(wrong, kind="stable")
    return oc.emit(*oc.split(wrong[idx]), idx, tv)


def _boundary_moved(tv):
    """One range boundary between two leaf slots one element off."""
    _, idx, (cf, cc, child) = _parts(tv)
    leaf = (cc > 0) & (child < 0)
    for n in range(len(cf)):
        s = np.nonzero(leaf[n])[0]
        for a, b in zip(s[:-1], s[1:]):
            if cc[n, a] <= 2 and cc[n, b] >= 2 and cf[n, a] + cc[n, a] == cf[n, b]:
                cc[n, a] += 1
                cf[n, b] += 1
                cc[n, b] -= 1
                return oc.emit(cf, cc, child, idx, tv)
    raise AssertionError("no pair of neighbouring leaf slots to move a boundary between")


def _plane_loosened(tv):
    tree = {k: v.copy() for k, v in oc.replay(tv, *pr.centroid_bounds(tv)).items()}
    n = len(tree["imask"]) // 2
    s = int(np.nonzero(tree["meta"][n])[0][0])
    pl = 3 if tree["planes"][n, 3, s] < 255 else 0
    tree["planes"][n, pl, s] += 1 if pl == 3 else -1
    return tree


FAULTS = {"swapped slots": _swapped_slots, "x and z exchanged": _x_and_z_exchanged, "boundary moved": _boundary_moved,
          "plane loosened": _plane_loosened}


# (identical triangles: every code is 0, there is no digit to exchange)
@pytest.mark.parametrize("name,fault", [(n, f) for n in ("tri9", "dup30", "ico300") for f in FAULTS if (n, f) != ("dup30", "x and z exchanged")])
def test_comparison_sees_a_faulty_builder(name, fault):
    """Each fault is built into a tree that is otherwise the builder's; but for the loosened plane the faulty tree is
    still a valid one with tight boxes and the same leaves' worth of triangles: only the comparison can tell."""
    tv = _small(name)
    want = oc.replay(tv, *pr.centroid_bounds(tv))
    bad = FAULTS[fault](tv)
    n8, tris = pr.as_read_back(bad, tv)
    util.check_bvh8(n8, tris)
    if fault != "plane loosened":
        assert util.check_bvh8_tight(n8, tris) == len(n8)
    with pytest.raises(AssertionError):
        pr.assert_same_tree(pr.canonical(n8, tris, 2), want, fault)


# ---- the GPU table's inputs reach what they are there for --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bi.OCTREE_INPUTS))
def test_input_reaches_what_the_table_says(name):
    make, reaches = bi.OCTREE_INPUTS[name]
    tv = np.ascontiguousarray(make(), F)
    info = {}
    oc.replay(tv, *pr.centroid_bounds(tv), info=info)
    for key, want in reaches.items():
        assert info[key] >= want[0] if isinstance(want, tuple) else info[key] == want, (name, key, info)
