"""The quality builder (csrc/bvh_gpu.hip, prt_gpu_bvh8_build_ploc; prt_set_param("gpu_build", 1)) restated in numpy.

bvh_gpu.hip is compiled without FMA contraction, and every choice the builder makes is a single fp32 operation or an
integer tie-break with a strict total order (stable radix sort, symmetric neighbour key, TopBuilder's comparator, the
greedy slot rule).  So the tree it builds is a FUNCTION of its input, and this module computes that function one fp32
operation at a time in the source's order:

    morton_order    k_morton + the radix sort (stable)
    nn_search       k_ploc_nn (radius given) / k_ploc_nn_full (radius None)
    build_binary    the PLOC passes: mutual pairs, new ids, compaction; then TopBuilder (top = "host") or full-search
                    passes down to the root (top = "device")
    dp_rows         ploc_dp_node for every binary node
    collapse        the slot walk of k_ploc_emit for one wide node
    replay          all of it + the emission (slots, leaves, quantization) -> the canonical tree

The one thing that is NOT a transliteration is the quantization: the source computes the cell exponent with log2 / ceil
in double precision plus fix-up loops; here it is the exact rule those are meant to implement (util.grid_exponent /
util.grid_planes: integer and rational arithmetic), so a device tree that equals the replay also has the tightest boxes.

Only child_base and tri_base come from atomics and differ from run to run.  `canonical` renumbers a tree read back
from the library (and the replay emits its tree directly) in the same form: nodes breadth first with children in slot
order, per node the origin bits, the three exponents, imask, the eight meta bytes (off recomputed in slot order), the
6 x 8 planes, per leaf slot the ORIGINAL triangle ids in stored order, per internal slot the canonical child index.
"""
import numpy as np

import util

F = np.float32
FLT_MAX = F(3.402823466e+38)
PLOC_TOP = 4096      # the passes stop at this many clusters (top = "host"); the windowed search runs only above it
PLOC_LEAF = 0xFF     # pick value: "this subtree is one leaf"
FIELDS = ("origin", "exp", "imask", "meta", "planes", "tri", "child")


# ---- 1. Morton codes + sort ------------------------------------------------------------------------------------------
def centroid_bounds(tv):
    """cmin, cmax as the scene compiler computes them: bounds of 0.5f * lo + 0.5f * hi over the triangles tv [n, 3, 3]."""
    c = F(0.5) * tv.min(axis=1) + F(0.5) * tv.max(axis=1)
    return c.min(axis=0), c.max(axis=0)


def expand10(v):
    v = v.astype(np.uint64)
    for mul, mask in ((0x00010001, 0xFF0000FF), (0x00000101, 0x0F00F00F), (0x00000011, 0xC30C30C3), (0x00000005, 0x49249249)):
        v = ((v * np.uint64(mul)) & np.uint64(0xFFFFFFFF)) & np.uint64(mask)
    return v.astype(np.uint32)


def morton_codes(tv, cmin, cmax):
    tv, cmin, cmax = np.asarray(tv, F), np.asarray(cmin, F), np.asarray(cmax, F)
    c = F(0.5) * tv.min(axis=1) + F(0.5) * tv.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(cmax > cmin, F(1024.0) / (cmax - cmin), F(0.0)).astype(F)
    f = np.minimum(np.maximum((c - cmin) * inv, F(0.0)), F(1023.0))
    q = f.astype(np.uint32)   # truncation
    return expand10(q[:, 0]) | (expand10(q[:, 1]) << np.uint32(1)) | (expand10(q[:, 2]) << np.uint32(2))


def morton_order(tv, cmin, cmax):
    """(sorted codes, sorted_idx): equal codes stay in input order."""
    codes = morton_codes(tv, cmin, cmax)
    idx = np.argsort(codes, kind="stable")
    return codes[idx], idx


# ---- 2. PLOC ---------------------------------------------------------------------------------------------------------
def half_area(lo, hi):
    d = hi - lo
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return dx * dy + dy * dz + dz * dx


def nn_search(B, radius=None):
    """nn[i] for the cluster boxes B [m, 6] in array order: the best partner within `radius` positions (None: among all),
    ranked by (merged half area, distance, parity of the lower position, lower position); i itself if there is none."""
    B = np.asarray(B, F)
    m = len(B)
    nn = np.arange(m, dtype=np.int64)
    if radius is None:
        offs = None
        K = m
    else:
        offs = np.concatenate([np.arange(-radius, 0), np.arange(1, radius + 1)]).astype(np.int64)
        K = len(offs)
    rows = max(1, (1 << 20) // max(K, 1))
    for i0 in range(0, m, rows):
        i = np.arange(i0, min(m, i0 + rows), dtype=np.int64)[:, None]
        J = np.arange(m, dtype=np.int64)[None, :] + 0 * i if offs is None else i + offs[None, :]
        valid = (J >= 0) & (J < m) & (J != i)
        Jc = np.clip(J, 0, m - 1)
        d = [np.maximum(B[i, 3 + a], B[Jc, 3 + a]) - np.minimum(B[i, a], B[Jc, a]) for a in range(3)]   # hi - lo of the merged box
        ar = d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
        ok = valid & (ar <= FLT_MAX)
        arm = np.where(ok, ar, np.inf)
        amin = arm.min(axis=1)
        r, c = np.nonzero(ok & (arm == amin[:, None]))   # the candidates of least area, row by row: the tie key decides
        ii, jj = i[r, 0], J[r, c]
        lowp = np.minimum(ii, jj)
        tie = (np.abs(ii - jj).astype(np.uint64) << np.uint64(33)) | ((lowp & 1).astype(np.uint64) << np.uint64(32)) | lowp.astype(np.uint64)
        order = np.lexsort((tie, r))
        rows_with, first = np.unique(r[order], return_index=True)
        nn[i[rows_with, 0]] = jj[order][first]
    return nn


class Binary:
    """The binary tree: nodes 0 .. n - 1 are the triangles in Morton order, internal nodes have larger ids than their children."""

    def __init__(self, leaf_box):
        n = len(leaf_box)
        self.n = n
        self.box = np.zeros((max(2 * n, 1), 6), F)
        self.box[:n] = leaf_box
        self.left = np.full(2 * n, -1, np.int64)
        self.right = np.full(2 * n, -1, np.int64)
        self.cnt = np.zeros(2 * n, np.int64)
        self.cnt[:n] = 1
        self.n_nodes = n
        self.root = 0
        self.windowed_passes = self.full_passes = 0
        self.pairs_per_pass = []


def ploc_pass(bt, cl, radius):
    """One pass over the cluster array cl: nearest neighbours, mutual pairs -> new nodes (ids in position order of the
    leaders), compaction.  Returns the next cluster array."""
    m = len(cl)
    nn = nn_search(bt.box[cl], radius)
    i = np.arange(m)
    mutual = (nn != i) & (nn[nn] == i)
    leader = mutual & (i < nn)
    keep = ~(mutual & (i > nn))
    L = np.nonzero(leader)[0]
    assert len(L) > 0, "a pass merges at least the globally best pair"
    ids = bt.n_nodes + np.arange(len(L))
    a, b = cl[L], cl[nn[L]]
    bt.box[ids, 0:3] = np.minimum(bt.box[a, 0:3], bt.box[b, 0:3])
    bt.box[ids, 3:6] = np.maximum(bt.box[a, 3:6], bt.box[b, 3:6])
    bt.left[ids], bt.right[ids], bt.cnt[ids] = a, b, bt.cnt[a] + bt.cnt[b]
    bt.n_nodes += len(L)
    bt.pairs_per_pass.append(len(L))
    out = cl.copy()
    out[L] = ids
    return out[keep]


def top_build(bt, cl):
    """TopBuilder: full-sweep SAH over the remaining clusters (weights = triangle counts), nodes in post order."""
    cbox, ccnt = bt.box[cl].copy(), bt.cnt[cl].astype(np.float64)

    def build(items):
        n = len(items)
        if n == 1:
            return int(cl[items[0]])
        bb = np.concatenate([cbox[items, 0:3].min(axis=0), cbox[items, 3:6].max(axis=0)])
        mid = n // 2
        cand = []   # per axis: (cost, distance of the split from the middle), in the sweep's order
        orders = []
        for axis in range(3):
            key = cbox[items, axis] + cbox[items, 3 + axis]
            order = items[np.lexsort((items, key))]   # cx < cy || (cx == cy && x < y)
            orders.append(order)
            sb = cbox[order]
            rlo = np.minimum.accumulate(sb[::-1, 0:3], axis=0)[::-1]
            rhi = np.maximum.accumulate(sb[::-1, 3:6], axis=0)[::-1]
            rc = np.cumsum(ccnt[order][::-1])[::-1]
            right_cost = half_area(rlo, rhi).astype(np.float64) * rc
            llo = np.minimum.accumulate(sb[:, 0:3], axis=0)
            lhi = np.maximum.accumulate(sb[:, 3:6], axis=0)
            lc = np.cumsum(ccnt[order])
            c = half_area(llo, lhi).astype(np.float64)[:-1] * lc[:-1] + right_cost[1:]
            cand.append(c)
        c = np.concatenate(cand)
        split = np.tile(np.arange(1, n), 3)
        di = np.abs(split - mid)
        # "c < best || (c == best && di < db)" in sweep order: the least cost; among those the split nearest the middle;
        # among those the first met
        sel = np.nonzero(c == c.min())[0]
        w = sel[np.argmin(di[sel])]
        order, s = orders[w // (n - 1)], int(split[w])
        l = build(order[:s])
        r = build(order[s:])
        k = bt.n_nodes
        bt.left[k], bt.right[k], bt.box[k], bt.cnt[k] = l, r, bb, int(ccnt[items].sum())
        bt.n_nodes += 1
        return k

    return build(np.arange(len(cl), dtype=np.int64))


def build_binary(leaf_box, radius=24, top="host"):
    assert top in ("host", "device") and 1 <= radius <= 64
    bt = Binary(np.asarray(leaf_box, F))
    cl = np.arange(bt.n, dtype=np.int64)
    stop_at = 1 if top == "device" else PLOC_TOP
    while len(cl) > stop_at:
        windowed = len(cl) > PLOC_TOP
        cl = ploc_pass(bt, cl, radius if windowed else None)
        bt.windowed_passes += windowed
        bt.full_passes += not windowed
    bt.root = int(cl[0]) if len(cl) == 1 else top_build(bt, cl)
    assert bt.n_nodes == 2 * bt.n - 1
    return bt


# ---- 3. the collapse DP ------------------------------------------------------------------------------------------------
def dp_rows(bt, ci):
    """cost [n_nodes, 8] fp32 and pick [n_nodes, 8] of ploc_dp_node, for every node (children first)."""
    ci = F(ci)
    n, N = bt.n, bt.n_nodes
    area = half_area(bt.box[:N, 0:3], bt.box[:N, 3:6])
    cost = np.zeros((N, 8), F)
    pick = np.zeros((N, 8), np.uint8)
    cost[:n] = (ci * area[:n])[:, None]
    pick[:n] = PLOC_LEAF
    height = np.zeros(N, np.int64)
    left, right = bt.left.tolist(), bt.right.tolist()
    hl = height.tolist()
    for k in range(n, N):
        hl[k] = 1 + max(hl[left[k]], hl[right[k]])
    height = np.asarray(hl, np.int64)
    for h in range(1, int(height.max()) + 1 if N > n else 1):
        ids = np.nonzero(height == h)[0]
        cl, cr, a = cost[bt.left[ids]], cost[bt.right[ids]], area[ids]
        dist, dk = {}, {}
        for j in range(2, 9):   # distribute j slots over the two children
            bestc = np.full(len(ids), FLT_MAX, F)
            bk = np.ones(len(ids), np.uint8)
            for k in range(1, j):
                v = cl[:, min(k, 7) - 1] + cr[:, min(j - k, 7) - 1]
                upd = v < bestc
                bestc, bk = np.where(upd, v, bestc), np.where(upd, np.uint8(k), bk)
            dist[j], dk[j] = bestc, bk
        c = bt.cnt[ids]
        leaf_cost = np.where(c <= 3, ci * c.astype(F) * a, FLT_MAX).astype(F)
        own = dist[8] + a
        is_leaf = leaf_cost <= own
        cn = np.zeros((len(ids), 8), F)
        pn = np.zeros((len(ids), 8), np.uint8)
        cn[:, 0] = np.where(is_leaf, leaf_cost, own)
        pn[:, 0] = np.where(is_leaf, PLOC_LEAF, 0)
        cn[:, 7], pn[:, 7] = dist[8], dk[8]
        for i in range(2, 8):   # i slots: split over the children, or do with i - 1 slots
            take = dist[i] < cn[:, i - 2]
            cn[:, i - 1] = np.where(take, dist[i], cn[:, i - 2])
            pn[:, i - 1] = np.where(take, dk[i], np.where(pn[:, i - 2] == PLOC_LEAF, PLOC_LEAF, 0))
        cost[ids], pick[ids] = cn, pn
    return cost, pick


def collapse(R, is_root, n, left, right, pick):
    """The children of the wide node that represents binary node R: [(binary node, is a leaf child)] in the walk's order.
    left / right / pick: plain lists (pick: a list of 8-lists)."""
    if R < n or (is_root and pick[R][0] == PLOC_LEAF):
        return [(R, True)]
    kids = []
    k8 = pick[R][7]
    stack = [(right[R], 8 - k8), (left[R], k8)]
    while stack:
        nd, slots = stack.pop()
        if nd < n:
            kids.append((nd, True))
            continue
        i = min(slots, 7)
        pn = pick[nd]
        while i > 1 and pn[i - 1] == 0:   # "use fewer slots"
            i -= 1
        if pn[i - 1] == PLOC_LEAF:
            kids.append((nd, True))
        elif i == 1:
            kids.append((nd, False))
        else:
            k = pn[i - 1]
            stack.append((right[nd], i - k))
            stack.append((left[nd], k))
    assert len(kids) <= 8
    return kids


def leaf_triangles(kid, n, left, right):
    """The Morton positions below binary node kid, left subtree first."""
    out, stack = [], [kid]
    while stack:
        x = stack.pop()
        if x < n:
            out.append(x)
        else:
            stack.append(right[x])
            stack.append(left[x])
    return out


# ---- 4. emission ---------------------------------------------------------------------------------------------------------
def assign_slots(node_box, kid_box, n_kids):
    """The greedy octant rule for a batch of wide nodes: node_box [N, 6], kid_box [N, 8, 6] (walk order), n_kids [N].
    Returns child_in [N, 8]: the kid in every slot, or -1."""
    N = len(node_box)
    half = F(0.5)
    d = (half * kid_box[:, :, 0:3] + half * kid_box[:, :, 3:6]) - (half * node_box[:, None, 0:3] + half * node_box[:, None, 3:6])
    sl = np.arange(8)
    t = [np.where((sl[None, None, :] >> a) & 1 == 1, d[:, :, a:a + 1], -d[:, :, a:a + 1]) for a in range(3)]
    score = ((t[0] + t[1]) + t[2]).astype(np.float64)   # [N, kid, slot]
    kid_free = np.arange(8)[None, :] < n_kids[:, None]
    slot_free = np.ones((N, 8), bool)
    child_in = np.full((N, 8), -1, np.int64)
    rows = np.arange(N)
    for rnd in range(8):
        act = rnd < n_kids
        if not act.any():
            break
        s = np.where(kid_free[:, :, None] & slot_free[:, None, :], score, -np.inf).reshape(N, 64)
        w = np.argmax(s, axis=1)   # the first maximum, kids outer, slots inner: "score > best" keeps the first
        c, b = w // 8, w % 8
        child_in[rows[act], b[act]] = c[act]
        kid_free[rows[act], c[act]] = False
        slot_free[rows[act], b[act]] = False
    return child_in


def replay(tv, cmin, cmax, radius=24, ci=0.6, top="host", leaf_cost=0.0, info=None, binaries=None):
    """The canonical tree prt_gpu_bvh8_build_ploc builds over the triangles tv [n, 3, 3] (fp32, input order).
    binaries: a dict of the caller's, per input, in which the binary trees are kept by (radius, top): they do not depend
    on ci, and the passes are the expensive part of a replay."""
    tv = np.ascontiguousarray(tv, F)
    n = len(tv)
    _, sorted_idx = morton_order(tv, cmin, cmax)
    sv = tv[sorted_idx]
    bt = None if binaries is None else binaries.get((radius, top))
    if bt is None:
        bt = build_binary(np.concatenate([sv.min(axis=1), sv.max(axis=1)], axis=1), radius, top)
        if binaries is not None:
            binaries[(radius, top)] = bt
    _, pick = dp_rows(bt, F(leaf_cost) if leaf_cost > 0.0 else F(ci))
    if info is not None:
        info.update(windowed_passes=bt.windowed_passes, full_passes=bt.full_passes, pairs_per_pass=bt.pairs_per_pass)
    left, right, pk = bt.left.tolist(), bt.right.tolist(), pick.tolist()
    out = {f: [] for f in FIELDS}
    level, n_emitted = [bt.root], 0
    while level:
        N = len(level)
        kids = [collapse(R, n_emitted == 0, n, left, right, pk) for R in level]
        K = np.zeros((N, 8), np.int64)
        KL = np.zeros((N, 8), bool)
        nk = np.asarray([len(k) for k in kids], np.int64)
        for r_, k in enumerate(kids):
            K[r_, :len(k)] = [x[0] for x in k]
            KL[r_, :len(k)] = [x[1] for x in k]
        nb = bt.box[np.asarray(level)]
        child_in = assign_slots(nb, bt.box[K], nk)
        occ = child_in >= 0
        ck = np.take_along_axis(K, np.maximum(child_in, 0), axis=1)        # binary node per slot
        leaf = occ & np.take_along_axis(KL, np.maximum(child_in, 0), axis=1)
        inner = occ & ~leaf
        cb = bt.box[ck]
        e = util.grid_exponent(nb[:, 0:3], nb[:, 3:6])
        qlo, qhi = util.grid_planes(nb[:, None, 0:3], e[:, None, :], cb[:, :, 0:3], cb[:, :, 3:6])
        qlo, qhi = np.where(occ[:, :, None], qlo, 255.0), np.where(occ[:, :, None], qhi, 0.0)
        assert qhi.max() <= 255.0
        kc = np.where(leaf, bt.cnt[ck], 0)
        off = np.cumsum(kc, axis=1) - kc
        assert (kc <= 3).all() and (off + kc <= 24).all()
        meta = np.where(leaf, (((1 << kc) - 1) << 5) | off, np.where(inner, (1 << 5) | (24 + np.arange(8))[None, :], 0))
        tri = np.full((N, 8, 3), -1, np.int64)
        for r_, s_ in zip(*np.nonzero(leaf)):
            t = leaf_triangles(int(ck[r_, s_]), n, left, right)
            tri[r_, s_, :len(t)] = sorted_idx[t]
        first_child = n_emitted + N + np.cumsum(inner.sum(axis=1)) - inner.sum(axis=1)
        child = np.where(inner, first_child[:, None] + np.cumsum(inner, axis=1) - inner, -1)
        out["origin"].append(nb[:, 0:3].copy().view(np.uint32))
        out["exp"].append(e)
        out["imask"].append((inner * (1 << np.arange(8))[None, :]).sum(axis=1))
        out["meta"].append(meta)
        out["planes"].append(np.concatenate([qlo.transpose(0, 2, 1), qhi.transpose(0, 2, 1)], axis=1).astype(np.int64))   # [N, plane, slot]
        out["tri"].append(tri)
        out["child"].append(child)
        n_emitted += N
        level = ck[inner].tolist()   # row-major: node by node, slot by slot
    return {f: np.concatenate(v) for f, v in out.items()}


# ---- the same form from a tree read back -----------------------------------------------------------------------------------
def canonical(n8, tris, n_prims):
    """bvh_read8() / bvh_read()[1] of a one-level tree in the canonical form (see the module docstring)."""
    S = util.slot_fields(n8)
    levels = util.tree_levels(S)
    order = np.concatenate(levels)
    assert len(order) == len(n8) and len(np.unique(order)) == len(n8)
    new_index = np.empty(len(n8), np.int64)
    new_index[order] = np.arange(len(n8))
    ids = tris[:, 3].copy().view(np.uint32).astype(np.int64) - n_prims
    w = n8[order]
    S = {k: v[order] for k, v in S.items()}
    leaf = S["occ"] & ~S["inner"]
    off = np.cumsum(S["cnt"], axis=1) - S["cnt"]
    meta = np.where(leaf, ((S["meta"] >> 5) << 5) | off, S["meta"])
    tri = np.full((len(n8), 8, 3), -1, np.int64)
    for k in range(3):
        sel = S["cnt"] > k
        tri[sel, k] = ids[S["first"][sel] + k]
    planes = np.stack([np.stack([(w[:, 8 + 2 * pl + (i >> 2)] >> (8 * (i & 3))) & 0xFF for i in range(8)], axis=1)
                       for pl in range(6)], axis=1).astype(np.int64)
    return dict(origin=w[:, 0:3].copy(), exp=np.stack([(w[:, 3] >> (8 * a)) & 0xFF for a in range(3)], axis=1).astype(np.int64) - 127,
                imask=(w[:, 3] >> 24).astype(np.int64), meta=meta, planes=planes, tri=tri,
                child=np.where(S["inner"], new_index[np.minimum(S["child"], len(n8) - 1)], -1))


def as_read_back(tree, tv, n_prims=2):
    """The canonical tree as the node / record arrays the library would hand back (records in leaf order)."""
    N = len(tree["imask"])
    n8 = np.zeros((N, 20), np.uint32)
    tris = []
    n8[:, 0:3] = tree["origin"]
    n8[:, 3] = ((tree["exp"] + 127) << (8 * np.arange(3))[None, :]).sum(axis=1) | (tree["imask"] << 24)
    for n in range(N):
        kids = tree["child"][n][tree["child"][n] >= 0]
        n8[n, 4] = kids[0] if len(kids) else 0
        n8[n, 5] = len(tris)
        for s in range(8):
            for t in tree["tri"][n, s][tree["tri"][n, s] >= 0]:
                tris.append(np.concatenate([tv[t, 0], np.asarray([n_prims + t], np.uint32).view(F), tv[t, 1], [F(0)], tv[t, 2], [F(0)]]))
    for w in range(2):
        n8[:, 6 + w] = (tree["meta"][:, 4 * w:4 * w + 4] << (8 * np.arange(4))[None, :]).sum(axis=1)
    for pl in range(6):
        for w in range(2):
            n8[:, 8 + 2 * pl + w] = (tree["planes"][:, pl, 4 * w:4 * w + 4] << (8 * np.arange(4))[None, :]).sum(axis=1)
    return n8, np.asarray(tris, F).reshape(-1, 12)


def assert_same_tree(got, want, what=""):
    """Field by field, with the first differing node in the message."""
    assert len(got["imask"]) == len(want["imask"]), f"{what}: {len(got['imask'])} nodes, the replay has {len(want['imask'])}"
    for f in FIELDS:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        if not np.array_equal(a, b):
            n = int(np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0][0])
            detail = "\n".join(f"    {g}: got {np.asarray(got[g])[n].tolist()}\n    {' ' * len(g)}  want {np.asarray(want[g])[n].tolist()}" for g in FIELDS)
            raise AssertionError(f"{what}: field '{f}' differs first at canonical node {n} of {len(a)}\n{detail}")
