"""tests/ploc_replay.py against independent statements of what each stage of the quality builder is FOR, on inputs small
enough for brute force (CPU only).  The replay is the yardstick the device-built trees are held to
(tests/test_gpu_ploc_replay.py); these tests keep it from being a transliteration that shares a bug with the source."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import ploc_replay as pr
import util

F = np.float32


def _boxes(rng, m, spread=1.0):
    c = rng.uniform(-spread, spread, (m, 3))
    h = rng.uniform(0.0, 0.2, (m, 3))
    return np.concatenate([c - h, c + h], axis=1).astype(F)


# ---- sorting ---------------------------------------------------------------------------------------------------------------
def test_morton_codes_are_sorted_and_equal_codes_stay_in_index_order():
    rng = np.random.default_rng(1)
    tv = rng.uniform(-1, 1, (3000, 3, 3)).astype(F)
    tv[500:900] = tv[500]            # a run of identical triangles: equal codes
    tv[1000:1400, :, 0] = F(0.25)    # and a flat sheet
    cmin, cmax = pr.centroid_bounds(tv)
    codes, idx = pr.morton_order(tv, cmin, cmax)
    assert sorted(idx.tolist()) == list(range(len(tv))) and codes.max() < 2 ** 30
    assert (np.diff(codes.astype(np.int64)) >= 0).all()
    same = np.diff(codes.astype(np.int64)) == 0
    assert same.sum() >= 399 and (np.diff(idx)[same] > 0).all()
    # the code is the bit interleave of the three truncated grid coordinates, z y x from the top; extremes hit 0 and 1023
    c = (F(0.5) * tv.min(axis=1) + F(0.5) * tv.max(axis=1)).astype(np.float64)
    g = np.clip(np.floor((c - cmin) * (F(1024.0) / (cmax - cmin)).astype(np.float64) * (1 - 1e-7)), 0, 1023).astype(np.int64)
    raw = pr.morton_codes(tv, cmin, cmax).astype(np.int64)
    coords = np.stack([sum(((raw >> (3 * b + a)) & 1) << b for b in range(10)) for a in range(3)], axis=1)
    assert (np.abs(coords - g) <= 1).all() and coords.min() == 0 and coords.max() == 1023
    # a degenerate axis (all centroids equal) maps to coordinate 0
    flat = tv.copy()
    flat[:, :, 1] = F(0.0)
    raw = pr.morton_codes(flat, *pr.centroid_bounds(flat)).astype(np.int64)
    assert (sum(((raw >> (3 * b + 1)) & 1) << b for b in range(10)) == 0).all()


# ---- neighbour search --------------------------------------------------------------------------------------------------------
def _naive_nn(B, radius):
    m = len(B)
    nn = []
    for i in range(m):
        best = None
        for j in range(m):
            if j == i or (radius is not None and abs(i - j) > radius):
                continue
            lo = np.minimum(B[i, 0:3], B[j, 0:3])
            hi = np.maximum(B[i, 3:6], B[j, 3:6])
            dx, dy, dz = (hi - lo).tolist()
            ar = F(F(F(dx) * F(dy)) + F(F(dy) * F(dz))) + F(F(dz) * F(dx))
            key = (float(ar), abs(i - j), min(i, j) & 1, min(i, j), j)
            best = key if best is None or key < best else best
        nn.append(i if best is None else best[4])
    return np.asarray(nn)


@pytest.mark.parametrize("m", [2, 3, 257, 600])
@pytest.mark.parametrize("radius", [1, 24, 64, None])
def test_neighbour_search_equals_the_double_loop(m, radius):
    rng = np.random.default_rng([m, radius or 0])
    B = _boxes(rng, m)
    if m > 100:
        B[40:72] = B[40]                      # a run of identical boxes
        B[200:230, 0:3] = np.round(B[200:230, 0:3] * 4) / 4   # and many equal areas
        B[200:230, 3:6] = B[200:230, 0:3] + F(0.25)
    assert np.array_equal(pr.nn_search(B, radius), _naive_nn(B, radius))


@pytest.mark.parametrize("radius", [1, 24, None])
def test_a_run_of_identical_boxes_pairs_up_and_halves_per_pass(radius):
    B = np.tile(np.asarray([[0, 0, 0, 1, 1, 1]], F), (64, 1))
    nn = pr.nn_search(B, radius)
    assert np.array_equal(nn, np.arange(64) ^ 1)   # (0,1), (2,3), ...
    bt = pr.build_binary(B, radius=radius or 24, top="device")
    assert bt.pairs_per_pass == [32, 16, 8, 4, 2, 1]
    assert np.array_equal(bt.left[64:96], np.arange(0, 64, 2)) and np.array_equal(bt.right[64:96], np.arange(1, 64, 2))


def test_binary_tree_of_the_passes_is_a_tree_with_exact_boxes():
    rng = np.random.default_rng(9)
    for top in ("host", "device"):
        B = _boxes(rng, 700)
        bt = pr.build_binary(B, 24, top)
        assert bt.n_nodes == 2 * 700 - 1 and bt.root == bt.n_nodes - 1
        kids = np.concatenate([bt.left[700:bt.n_nodes], bt.right[700:bt.n_nodes]])
        assert sorted(kids.tolist()) == list(range(bt.n_nodes - 1))   # every node but the root is a child once
        for k in range(700, bt.n_nodes):
            l, r = bt.left[k], bt.right[k]
            assert l < k and r < k and bt.cnt[k] == bt.cnt[l] + bt.cnt[r]
            assert np.array_equal(bt.box[k, 0:3], np.minimum(bt.box[l, 0:3], bt.box[r, 0:3]))
            assert np.array_equal(bt.box[k, 3:6], np.maximum(bt.box[l, 3:6], bt.box[r, 3:6]))


def test_top_builder_takes_the_cheapest_sweep_split_and_ties_go_to_the_middle():
    rng = np.random.default_rng(4)
    B = _boxes(rng, 9)
    bt = pr.Binary(B)
    bt.cnt[:9] = rng.integers(1, 5, 9)
    root = pr.top_build(bt, np.arange(9))
    # brute force over every axis and split of the root's sweep, in float64 over the fp32 half areas
    best = None
    for axis in range(3):
        order = sorted(range(9), key=lambda x: (float(F(B[x, axis] + B[x, 3 + axis])), x))
        for s in range(1, 9):
            cst = 0.0
            for part in (order[:s], order[s:]):
                lo, hi = B[part, 0:3].min(axis=0), B[part, 3:6].max(axis=0)
                cst += float(pr.half_area(lo, hi)) * float(bt.cnt[part].sum())
            key = (cst, abs(s - 4), axis, s)
            if best is None or key < best[0]:
                best = (key, set(order[:s]))

    def below(k):
        return {int(k)} if k < 9 else below(bt.left[k]) | below(bt.right[k])
    assert below(bt.left[root]) == best[1] and below(root) == set(range(9)) and bt.cnt[root] == bt.cnt[:9].sum()
    # identical boxes: every split costs the same, the tree must be balanced (depth log2), not a chain
    bt = pr.Binary(np.tile(np.asarray([[0, 0, 0, 1, 1, 1]], F), (64, 1)))
    root = pr.top_build(bt, np.arange(64))

    def depth(k):
        return 0 if k < 64 else 1 + max(depth(bt.left[k]), depth(bt.right[k]))
    assert depth(root) == 6


# ---- collapse DP ---------------------------------------------------------------------------------------------------------
def _random_binary(rng, n):
    """A random binary tree over n single-triangle leaves (ids as in the builder: children before parents)."""
    bt = pr.Binary(_boxes(rng, n))
    roots = list(range(n))
    while len(roots) > 1:
        i, j = sorted(rng.choice(len(roots), 2, replace=False).tolist())
        a, b = roots[i], roots[j]
        k = bt.n_nodes
        bt.left[k], bt.right[k], bt.cnt[k] = a, b, bt.cnt[a] + bt.cnt[b]
        bt.box[k, 0:3], bt.box[k, 3:6] = np.minimum(bt.box[a, 0:3], bt.box[b, 0:3]), np.maximum(bt.box[a, 3:6], bt.box[b, 3:6])
        bt.n_nodes += 1
        roots = [r for r in roots if r not in (a, b)] + [k]
    bt.root = roots[0]
    return bt


def _brute_force_minimum(bt, ci):
    """The least cost over EVERY legal collapse, in float64 over the fp32 terms (half areas, ci * count * area): wide nodes
    of at most 8 children, leaves of at most 3 triangles, a single triangle is always a leaf."""
    area = pr.half_area(bt.box[:, 0:3], bt.box[:, 3:6])
    n = bt.n

    def cuts(k, room):   # every set of disjoint subtrees that covers the leaves below k, of at most `room` members
        yield (k,)
        if k >= n and room >= 2:
            for a in range(1, room):
                for x in cuts(int(bt.left[k]), a):
                    for y in cuts(int(bt.right[k]), room - len(x)):
                        yield x + y

    memo = {}

    def as_child(k):     # least cost of the subtree of k as ONE child of a wide node
        if k not in memo:
            c = int(bt.cnt[k])
            options = [float(F(F(ci) * F(c)) * area[k])] if c <= 3 else []
            if k >= n:
                options.append(float(area[k]) + min(sum(as_child(x) for x in cut) for cut in set(cuts(k, 8)) if cut != (k,)))
            memo[k] = min(options)
        return memo[k]
    return as_child(bt.root)


def _decoded(bt, cost, pick, ci):
    """The wide tree the picks encode below the root: (its cost in float64 over the same fp32 terms, its cost summed in
    fp32 in the DP's own association, widest node, largest leaf)."""
    n, area = bt.n, pr.half_area(bt.box[:, 0:3], bt.box[:, 3:6])
    left, right, pk = bt.left.tolist(), bt.right.tolist(), pick.tolist()
    widest, largest = [0], [0]

    def leaf_term(k):
        largest[0] = max(largest[0], int(bt.cnt[k]))
        return F(F(ci) * F(int(bt.cnt[k]))) * area[k]

    def exact(k, leaf):   # as one child
        if leaf:
            return float(leaf_term(k))
        kids = pr.collapse(k, False, n, left, right, pk)
        widest[0] = max(widest[0], len(kids))
        return float(area[k]) + sum(exact(x, lf) for x, lf in kids)

    def in_fp32(k, slots):   # the value the DP row claims for k in `slots` slots, from the picks alone
        if k < n:
            return leaf_term(k)
        i = min(slots, 7)
        while i > 1 and pk[k][i - 1] == 0:
            i -= 1
        if pk[k][i - 1] == pr.PLOC_LEAF:
            return leaf_term(k)
        if i == 1:
            return F(F(in_fp32(left[k], pk[k][7]) + in_fp32(right[k], 8 - pk[k][7])) + area[k])
        return F(in_fp32(left[k], pk[k][i - 1]) + in_fp32(right[k], i - pk[k][i - 1]))

    root_is_leaf = pk[bt.root][0] == pr.PLOC_LEAF
    return exact(bt.root, root_is_leaf), in_fp32(bt.root, 1), widest[0], largest[0]


@pytest.mark.parametrize("n", range(2, 11))
@pytest.mark.parametrize("ci", [0.1, 0.6, 4.0])
def test_collapse_dp_finds_the_minimum_over_every_legal_collapse(n, ci):
    """cost[root][0] equals the brute-force minimum within k * 2^-23 relative, k = 2 n: a collapse's cost is a sum of at most
    2 n - 1 positive terms (<= n - 1 wide nodes, <= n leaves), so at most 2 n - 2 fp32 additions of positive values lie
    on any path through the DP, each off by at most 2^-24 relative: (1 + 2^-24)^(2n) - 1 < 2 n * 2^-23.  (The terms
    themselves are the same fp32 values on both sides.)  The tree decoded from the picks must be legal, must have that
    cost in exact arithmetic within the same bound, and its cost summed in the DP's own association must be
    cost[root][0] bit for bit: the picks describe the tree the row prices."""
    for trial in range(6):
        rng = np.random.default_rng([n, int(ci * 10), trial])
        bt = _random_binary(rng, n)
        cost, pick = pr.dp_rows(bt, ci)
        want = _brute_force_minimum(bt, ci)
        got = float(cost[bt.root, 0])
        bound = 2 * n * 2.0 ** -23
        assert abs(got - want) <= bound * want, (n, ci, trial, got, want)
        exact, fp32, widest, largest = _decoded(bt, cost, pick, ci)
        assert widest <= 8 and largest <= 3
        assert fp32 == cost[bt.root, 0], (n, ci, trial)
        assert abs(exact - want) <= bound * want, (n, ci, trial, exact, want)
        # rows never get worse with more slots, and the children of the root's wide node cover every triangle once
        assert (np.diff(cost[bt.root, 0:7]) <= 0).all()
        kids = pr.collapse(bt.root, True, n, bt.left.tolist(), bt.right.tolist(), pick.tolist())
        below = sorted(itertools.chain.from_iterable(pr.leaf_triangles(k, n, bt.left.tolist(), bt.right.tolist()) for k, _ in kids))
        assert below == list(range(n))


# ---- quantization ------------------------------------------------------------------------------------------------------------
def _fraction_rule(lo, hi, clo, chi):
    lo, hi, clo, chi = (Fraction(float(x)) for x in (lo, hi, clo, chi))
    ext, big = hi - lo, max(abs(lo), abs(hi))
    floor_e = -126
    if big > 0:
        floor_e = max(floor_e, math.floor(math.log2(big)) - 30)
        while Fraction(2) ** (floor_e + 30) > big and floor_e > -126:   # (math.log2 of a Fraction rounds: settle it exactly)
            floor_e -= 1
        while Fraction(2) ** (floor_e + 31) <= big:
            floor_e += 1
    e = floor_e
    while math.ceil(ext / Fraction(2) ** e) > 255:
        e += 1
    cell = Fraction(2) ** e
    qlo = max(math.floor((clo - lo) / cell), 0)
    assert lo + qlo * cell <= clo and (qlo == 0 and clo == lo or lo + (qlo + 1) * cell > clo)
    qhi = math.ceil((chi - lo) / cell)
    assert lo + qhi * cell >= chi and (qhi == 0 or lo + (qhi - 1) * cell < chi)
    return e, qlo, qhi


def test_quantization_rule_against_rational_arithmetic():
    rng = np.random.default_rng(12)
    cases = []
    for k in (-140, -126, -100, -20, -1, 0, 1, 7, 30, 100):   # extents at, just below and just above 255 * 2^k and 2^k
        for base in (255.0, 256.0, 1.0):
            x = F(base * 2.0 ** k) if abs(k) < 120 or base == 1.0 else F(0)
            for ext in (x, np.nextafter(x, F(0)), np.nextafter(x, F(np.inf))):
                for lo in (F(0), F(-1), F(1), -ext / F(2), F(rng.normal()), F(1e-30), F(-3e5)):
                    cases.append((lo, F(lo + ext)))
    for _ in range(400):
        lo = F(rng.normal() * 10.0 ** rng.integers(-6, 6))
        cases.append((lo, F(lo + abs(F(rng.normal() * 10.0 ** rng.integers(-8, 6))))))
    cases = [(lo, hi) for lo, hi in cases if np.isfinite(lo) and np.isfinite(hi) and hi >= lo]
    inexact = 0
    for lo, hi in cases:
        t = rng.uniform(0, 1, 2)
        clo = F(min(max(lo + F(t.min()) * (hi - lo), lo), hi))
        chi = F(min(max(lo + F(t.max()) * (hi - lo), clo), hi))
        for c0, c1 in ((clo, chi), (lo, hi), (hi, hi), (lo, lo)):
            want = _fraction_rule(lo, hi, c0, c1)
            e = util.grid_exponent(np.asarray([lo]), np.asarray([hi]))
            qlo, qhi = util.grid_planes(np.asarray([lo]), e, np.asarray([c0]), np.asarray([c1]))
            assert (int(e[0]), int(qlo[0]), int(qhi[0])) == want, (lo, hi, c0, c1)
            assert want[2] <= 255
        inexact += not util._exact_sub(np.float64(hi), np.float64(lo))[1]
    assert inexact > 0 and len(cases) > 600   # (both the double path and the rational fall-back ran)


# ---- the whole replay on small meshes: a valid, tight tree ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 300])
@pytest.mark.parametrize("top", ["host", "device"])
def test_replayed_tree_is_a_valid_tight_tree_and_survives_the_round_trip(n, top):
    rng = np.random.default_rng(n)
    c = rng.uniform(-1, 1, (n, 1, 3))
    tv = (c + rng.normal(size=(n, 3, 3)) * 0.05).astype(F)
    if n == 300:
        tv[100:140] = tv[100]   # duplicated triangles
        tv[:, :, 1][200:] = F(0.0)
    tree = pr.replay(tv, *pr.centroid_bounds(tv), top=top)
    n8, tris = pr.as_read_back(tree, tv)
    fill, _ = util.check_bvh8(n8, tris)
    assert util.check_bvh8_tight(n8, tris) == len(n8)
    assert sorted(tree["tri"][tree["tri"] >= 0].tolist()) == list(range(n))
    pr.assert_same_tree(pr.canonical(n8, tris, 2), tree, "round trip")
    if n <= 3:
        assert len(n8) == 1 and (fill == [1] if n == 1 else fill[0] <= n)   # one node: the root holds the leaves
    # the checker and the comparison see a loosened plane, a wrong exponent and swapped triangles
    bad = n8.copy()
    bad[0, 14] += 1 if (bad[0, 14] & 0xFF) < 255 else -1
    with pytest.raises(AssertionError):
        util.check_bvh8_tight(bad, tris)
    with pytest.raises(AssertionError):
        pr.assert_same_tree(pr.canonical(bad, tris, 2), tree)
    bad = n8.copy()
    bad[0, 3] += 1
    with pytest.raises(AssertionError):
        util.check_bvh8_tight(bad, tris)
    if n >= 4:
        swapped = tris.copy()
        swapped[[0, len(tris) - 1]] = swapped[[len(tris) - 1, 0]]
        with pytest.raises(AssertionError):
            pr.assert_same_tree(pr.canonical(n8, swapped, 2), tree)
