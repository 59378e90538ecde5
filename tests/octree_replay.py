"""The Morton octree builder (csrc/bvh_gpu.hip, prt_gpu_bvh8_build; prt_set_param("gpu_build", 2)) restated in numpy.

The builder makes no floating-point choice after the Morton codes: the tree's topology is a function of the sorted 30-bit
codes alone (k_split), the boxes are exact fp32 minima / maxima (k_boxes), and the quantization has one right answer.  So
the tree is a FUNCTION of its input, and this module computes that function in the source's order:

    morton_order    ploc_replay's: k_morton + the stable radix sort (the two builders share both)
    split           k_split for every node, breadth first: the range of a node -> its eight sub-ranges
    emit            slots, leaves, k_boxes bottom-up, quantization -> the canonical tree of ploc_replay.FIELDS
    replay          all of it

What the header comment of bvh_gpu.hip promises and only this comparison can see: the Morton digit (z << 2 | y << 1 | x)
IS the child's slot; levels at which a range falls into one octant are skipped; ten consumed levels mean identical codes,
which are split by index into parts = count <= 24 ? (count + 2) / 3 : 8; a child range of 1 .. 3 triangles is a leaf of
its parent (in sorted order, `off` accumulating in slot order), one of more than 3 an internal node.

As in ploc_replay the quantization is not a transliteration of k_quantize (log2 / ceil in double plus fix-up loops) but the
exact rule it is meant to implement (util.grid_exponent / util.grid_planes), so a device tree that equals the replay also
has the tightest boxes.  child_base and tri_base come from atomics; ploc_replay.canonical removes them from a read-back."""
import numpy as np

import ploc_replay as pr
import util

F = np.float32
LEVELS = 10      # octree levels in a 30-bit code
MAX_LEAF = 3     # a range of at most this many triangles is a leaf
FLT_MAX = pr.FLT_MAX


def code_facts(tv, cmin, cmax):
    """What k_morton's clamps and the bounds did to this input: (coordinates clamped at the upper end, flat axes)."""
    tv, cmin, cmax = np.asarray(tv, F), np.asarray(cmin, F), np.asarray(cmax, F)
    c = F(0.5) * tv.min(axis=1) + F(0.5) * tv.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(cmax > cmin, F(1024.0) / (cmax - cmin), F(0.0)).astype(F)
    f = (c - cmin) * inv
    return int((f > F(1023.0)).sum()), int((~(cmax > cmin)).sum())


def lower_bound(codes, a, b, key):
    """First position in [a, b) whose code is >= key (the device's binary search; codes ascending)."""
    return a + int(np.searchsorted(codes[a:b], key, side="left"))


def split_range(codes, first, count, level, info=None):
    """k_split's loop for one node: (cf[8], cc[8], levels consumed afterwards)."""
    info = {} if info is None else info
    cf, cc = [first] * 8, [0] * 8
    while True:
        if count <= MAX_LEAF:    # only the root of a tiny mesh: one leaf child, in slot 0
            cc[0] = count
            return cf, cc, level
        if level >= LEVELS:      # identical codes: split by index
            parts = (count + 2) // 3 if count <= 24 else 8
            which = "index_splits_small" if count <= 24 else "index_splits_8"
            info[which] = info.get(which, 0) + 1
            for c in range(8):
                lo, hi = (count * c) // parts, (count * (c + 1)) // parts
                cf[c] = first + (lo if c < parts else count)
                cc[c] = hi - lo if c < parts else 0
            return cf, cc, level
        shift = 3 * (LEVELS - 1 - level)
        prefix = int(codes[first]) & ~((8 << shift) - 1)
        prev, end = first, first + count
        for c in range(8):
            nxt = end if c == 7 else lower_bound(codes, prev, end, prefix | ((c + 1) << shift))
            cf[c], cc[c] = prev, nxt - prev
            prev = nxt
        level += 1
        if sum(1 for x in cc if x) >= 2:
            return cf, cc, level
        info["skipped_levels"] = info.get("skipped_levels", 0) + 1   # a level that does not split the range


def split(codes, info=None):
    """The topology over the sorted codes, nodes breadth first with children in slot order (= the canonical order):
    cf, cc [N, 8] (sub-range of every slot in the sorted array) and child [N, 8] (node of a slot with more than 3, else -1)."""
    codes = np.asarray(codes, np.uint32).astype(np.int64)
    CF, CC, CH = [], [], []
    level_nodes = [(0, len(codes), 0)]
    n_emitted = 0
    while level_nodes:
        nxt = []
        first_child = n_emitted + len(level_nodes)
        for first, count, level in level_nodes:
            cf, cc, lv = split_range(codes, first, count, level, info)
            ch = [-1] * 8
            for c in range(8):
                if cc[c] > MAX_LEAF:
                    ch[c] = first_child + len(nxt)
                    nxt.append((cf[c], cc[c], lv))
            CF.append(cf), CC.append(cc), CH.append(ch)
        n_emitted += len(level_nodes)
        level_nodes = nxt
    return np.asarray(CF, np.int64), np.asarray(CC, np.int64), np.asarray(CH, np.int64)


def emit(cf, cc, child, sorted_idx, tv):
    """The canonical tree of a topology (split) over the triangles tv [n, 3, 3] in input order: meta, leaves, the boxes
    bottom-up as exact fp32 minima / maxima (k_boxes), the exact quantization."""
    tv = np.ascontiguousarray(tv, F)
    sv = tv[sorted_idx]
    tlo, thi = sv.min(axis=1), sv.max(axis=1)
    N = len(cf)
    inner = child >= 0
    leaf = (cc > 0) & ~inner
    occ = inner | leaf
    assert (cc[leaf] <= MAX_LEAF).all()
    kc = np.where(leaf, cc, 0)
    off = np.cumsum(kc, axis=1) - kc
    assert (off + kc <= 24).all()
    meta = np.where(leaf, (((1 << kc) - 1) << 5) | off, np.where(inner, (1 << 5) | (24 + np.arange(8))[None, :], 0))
    tri = np.full((N, 8, 3), -1, np.int64)
    slot_lo = np.full((N, 8, 3), FLT_MAX, F)
    slot_hi = np.full((N, 8, 3), -FLT_MAX, F)
    for k in range(MAX_LEAF):
        sel = kc > k
        pos = cf[sel] + k
        tri[sel, k] = sorted_idx[pos]
        slot_lo[sel] = np.minimum(slot_lo[sel], tlo[pos])
        slot_hi[sel] = np.maximum(slot_hi[sel], thi[pos])
    node_lo = np.full((N, 3), FLT_MAX, F)
    node_hi = np.full((N, 3), -FLT_MAX, F)
    for n in range(N - 1, -1, -1):   # children have larger indices than their parent
        s = np.nonzero(inner[n])[0]
        slot_lo[n, s], slot_hi[n, s] = node_lo[child[n, s]], node_hi[child[n, s]]
        o = occ[n]
        node_lo[n], node_hi[n] = slot_lo[n, o].min(axis=0), slot_hi[n, o].max(axis=0)
    e = util.grid_exponent(node_lo, node_hi)
    safe_lo, safe_hi = np.where(occ[:, :, None], slot_lo, node_lo[:, None, :]), np.where(occ[:, :, None], slot_hi, node_lo[:, None, :])
    qlo, qhi = util.grid_planes(node_lo[:, None, :], e[:, None, :], safe_lo, safe_hi)
    qlo, qhi = np.where(occ[:, :, None], qlo, 255.0), np.where(occ[:, :, None], qhi, 0.0)
    assert qhi.max() <= 255.0
    return dict(origin=node_lo.copy().view(np.uint32), exp=e, imask=(inner * (1 << np.arange(8))[None, :]).sum(axis=1), meta=meta,
                planes=np.concatenate([qlo.transpose(0, 2, 1), qhi.transpose(0, 2, 1)], axis=1).astype(np.int64), tri=tri, child=child.copy())


def replay(tv, cmin, cmax, info=None):
    """The canonical tree prt_gpu_bvh8_build builds over the triangles tv [n, 3, 3] (fp32, input order).  info: a dict that
    receives what the input reached (skipped_levels, index_splits_small, index_splits_8, clamped_1023, flat_axes, n_nodes,
    leaf_slots_beside_internal: nodes with leaf slots and internal slots side by side)."""
    tv = np.ascontiguousarray(tv, F)
    codes, sorted_idx = pr.morton_order(tv, cmin, cmax)
    counts = dict(skipped_levels=0, index_splits_small=0, index_splits_8=0)
    cf, cc, child = split(codes, counts)
    if info is not None:
        clamped, flat = code_facts(tv, cmin, cmax)
        inner, leaf = child >= 0, (cc > 0) & (child < 0)
        info.update(counts, clamped_1023=clamped, flat_axes=flat, n_nodes=len(cf),
                    leaf_slots_beside_internal=int((inner.any(axis=1) & leaf.any(axis=1)).sum()))
    return emit(cf, cc, child, sorted_idx, tv)
