"""The numpy restatement of surface baking (tests/bake_replay.py) against what the header promises, without a GPU: the
coverage rule on small layouts whose answer is known by hand, and the conditions the GPU tests (tests/test_gpu_bake.py,
tests/test_gpu_bake_shapes.py) rely on, shown from the reference alone: for the shapes beyond toy maps, the grid's owners
against exact rational arithmetic and its no-crack law, the soup's shares, and the slivers under the rule with and without
the box condition."""
import numpy as np
import pytest

import bake_replay as br
import closed_form as cf

F = np.float32


def faces(uv, y=0.0):
    """Faces with the given UVs [F, 3, 2] whose positions are (u, y, v) and whose normals are +y"""
    uv = np.asarray(uv, F)
    pos = np.stack([uv[..., 0], np.full(uv.shape[:2], y, F), uv[..., 1]], -1).astype(F)
    nrm = np.zeros_like(pos)
    nrm[..., 1] = 1.0
    return uv, pos, nrm


SQUARE = [[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]]


def test_unit_square_covers_every_texel_once_and_the_diagonal_is_face_0():
    W, H = 5, 3
    s = br.surface(faces(SQUARE), W, H)
    assert s["n_covered"] == 15 and (s["coverage"] == 1).all() and s["n_degenerate"] == 0 and s["n_faces_skipped"] == 0
    # each face alone: together they cover every texel, and they share exactly the texels whose centre is on the diagonal
    a = br.surface(faces(SQUARE[:1]), W, H)["coverage"].astype(bool)
    b = br.surface(faces(SQUARE[1:]), W, H)["coverage"].astype(bool)
    i, j = np.indices((H, W))
    px, py = (j + 0.5) / W, 1.0 - (i + 0.5) / H
    assert (a | b).all() and np.array_equal(a & b, px == py) and (a & b).sum() >= 1      # (the centre texel: 0.5, 0.5)
    assert (s["owner"][a & b] == 0).all()
    assert np.array_equal(s["owner"] == 0, a) and np.array_equal(s["owner"] == 1, ~a)
    # face 0 lies below the diagonal (v <= u): the bottom right of the map, row 0 being the top
    assert s["owner"][H - 1, W - 1] == 0 and s["owner"][0, 0] == 1
    # position = (u, 0, v) of the texel centre up to fp32 rounding of the interpolation
    assert np.allclose(s["position"][..., 0], px, atol=1e-6) and np.allclose(s["position"][..., 2], py, atol=1e-6)
    assert (s["normal"] == np.array([0, 1, 0], F)).all()


def test_winding_does_not_matter():
    flipped = [[t[0], t[2], t[1]] for t in SQUARE]
    a, b = br.surface(faces(SQUARE), 5, 3), br.surface(faces(flipped), 5, 3)
    assert np.array_equal(a["owner"], b["owner"]) and np.allclose(a["position"], b["position"], atol=1e-6)


def test_overlapping_faces_give_the_lowest_index():
    tri = [[0, 0], [1, 0], [0, 1]]
    s = br.surface(faces([SQUARE[1], tri, SQUARE[0], tri]), 8, 8)
    only = br.surface(faces([tri]), 8, 8)["coverage"].astype(bool)
    first = br.surface(faces([SQUARE[1]]), 8, 8)["coverage"].astype(bool)
    assert (only & ~first).any() and (only & first).any()
    assert (s["owner"][first] == 0).all() and (s["owner"][only & ~first] == 1).all() and (s["owner"][~only & ~first] == 2).all()
    assert not (s["owner"] == 3).any()


def test_zero_area_face_is_skipped_and_counted():
    line = [[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]]
    point = [[0.5, 0.5]] * 3
    s = br.surface(faces([line, point] + SQUARE), 4, 4)
    assert s["n_faces_skipped"] == 2 and s["n_covered"] == 16 and set(np.unique(s["owner"])) == {2, 3}
    nan = [[0, 0], [np.nan, 0], [1, 1]]
    assert br.surface(faces([nan] + SQUARE), 4, 4)["n_faces_skipped"] == 1


def test_uvs_outside_the_unit_square_are_clipped_not_wrapped():
    big = [[-1.0, -1.0], [3.0, -1.0], [-1.0, 3.0]]          # contains the whole unit square
    assert br.surface(faces([big]), 7, 5)["n_covered"] == 35
    away = [[1.25, 0.0], [2.0, 0.0], [2.0, 1.0]]            # u > 1 everywhere: nothing, where wrapping would cover texels
    assert br.surface(faces([away]), 7, 5)["n_covered"] == 0
    half = [[0.5, -2.0], [4.0, -2.0], [0.5, 4.0]]           # its left edge u = 0.5 passes through the centres of column 3 of 7
    s = br.surface(faces([half]), 7, 5)
    assert np.array_equal(s["coverage"].astype(bool), np.broadcast_to(np.arange(7) >= 3, (5, 7)))


def test_one_by_one_map():
    s = br.surface(faces(SQUARE), 1, 1)
    assert s["owner"].shape == (1, 1) and s["owner"][0, 0] == 0 and np.array_equal(s["bary"][0, 0], np.array([0.0, 0.5], F))
    assert np.array_equal(s["position"][0, 0], np.array([0.5, 0.0, 0.5], F))


def test_degenerate_normal_is_not_covered_and_counted():
    uv, pos, nrm = faces(SQUARE)
    nrm[0] = 0.0                                            # face 0 has no normal anywhere; face 1 keeps its own
    s = br.surface((uv, pos, nrm), 4, 4)
    bad = (s["owner"] == br.NONE)
    assert s["n_degenerate"] == bad.sum() > 0 and s["n_covered"] == 16 - bad.sum() > 0
    assert (s["coverage"][bad] == 0).all() and not s["position"][bad].any() and np.isfinite(s["normal"]).all()


def test_rng_matches_the_library_constants():
    # pcg_hash(0) and the first draws of a known state, by hand from the header's formulas
    assert int(br.pcg_hash(np.array([0]))[0]) == ((lambda w: (w >> 22) ^ w)(((2891336453 >> ((2891336453 >> 28) + 4)) ^ 2891336453) * 277803737 & 0xFFFFFFFF))
    s, u = br.rnd01(np.array([12345], np.uint32))
    assert 0.0 <= u[0] < 1.0 and u.dtype == F and s[0] == br.pcg_hash(np.array([12345]))[0]
    st, v = br.random_unit_vector(np.arange(1000, dtype=np.uint32))
    l2 = (v.astype(np.float64) ** 2).sum(1)
    assert np.allclose(l2, 1.0, atol=1e-6) and (st != np.arange(1000)).all()
    assert np.allclose(v.mean(0), 0.0, atol=0.1)


def test_rays_are_cosine_distributed_and_keyed_by_the_full_map_index():
    s = br.reference("square", 16, 16)
    r0, r3 = br.rays(s, 0, 11), br.rays(s, 3, 11)
    assert (r0["rng_state"] != r3["rng_state"]).all() and np.array_equal(r0["o"], s["position"])
    d = r0["d"].reshape(-1, 3).astype(np.float64)
    assert np.allclose((d ** 2).sum(1), 1.0, atol=1e-6) and (d[:, 1] > 0).all()
    assert abs(d[:, 1].mean() - 2.0 / 3.0) < 0.05            # E cos = 2/3 under the cosine law
    # a texel's ray does not depend on coverage elsewhere: the same texel on a map where another face is missing
    uv, pos, nrm = br.mesh_faces(br.shape("square")["mesh"])
    half = br.surface((uv[:1], pos[:1], nrm[:1]), 16, 16)
    rh = br.rays(half, 0, 11)
    keep = half["coverage"] != 0
    assert 0 < keep.sum() < 256 and np.array_equal(rh["d"][keep], r0["d"][keep]) and np.array_equal(rh["rng_state"][keep], r0["rng_state"][keep])
    assert not rh["d"][~keep].any() and not rh["rng_state"][~keep].any()


def test_dilate_fills_gutters_in_order():
    cov = np.zeros((3, 4), np.uint8)
    val = np.zeros((3, 4, 3), F)
    cov[1, 1] = 1
    val[1, 1] = (1.0, 2.0, 3.0)
    cov[1, 2] = 1
    val[1, 2] = (3.0, 2.0, 1.0)
    c1, v1, n1 = br.dilate(cov, val, 1)
    assert n1 == 10 and (c1 == np.array([[2, 2, 2, 2], [2, 1, 1, 2], [2, 2, 2, 2]])).all()
    assert np.array_equal(v1[0, 0], val[1, 1]) and np.array_equal(v1[0, 1], np.array([2.0, 2.0, 2.0], F)) and np.array_equal(v1[1, 1], val[1, 1])
    c0, v0, n0 = br.dilate(cov, val, 0)
    assert n0 == 0 and np.array_equal(c0, cov) and np.array_equal(v0, val)
    far = np.zeros((1, 5), np.uint8)
    far[0, 0] = 1
    fv = np.zeros((1, 5, 3), F)
    fv[0, 0] = 7.0
    c3, v3, n3 = br.dilate(far, fv, 3)
    assert n3 == 3 and list(c3[0]) == [1, 2, 2, 2, 0] and (v3[0, :4] == 7.0).all() and not v3[0, 4].any()


# ---- the conditions the GPU tests rely on ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.SHAPES)
def test_every_gpu_case_covers_texels(name):
    for H, W in br.SIZES:
        s = br.reference(name, H, W)
        empty = name.endswith("atlas") and (H, W) == (1, 1)      # the one centre lies in a gutter: a map without a covered texel
        assert (s["n_covered"] > 0) != empty and s["n_degenerate"] == 0 and s["n_faces_skipped"] == 0, (name, H, W)
        assert np.isfinite(s["position"]).all() and np.isfinite(s["normal"]).all()
        n = s["normal"][s["coverage"] != 0].astype(np.float64)
        assert np.allclose((n ** 2).sum(1), 1.0, atol=1e-6)
    full = br.reference(name, 17, 33)
    if name.endswith("atlas"):       # gutters: some texels are uncovered, and one pass does not fill them all ...
        assert 0 < full["n_covered"] < 561
        c1, _, n1 = br.dilate(full["coverage"], np.ones((17, 33, 3), F), 1)
        c3, _, n3 = br.dilate(full["coverage"], np.ones((17, 33, 3), F), 3)
        assert 0 < n1 < n3 and (c1 == 0).any(), (n1, n3)
        assert len(np.unique(full["owner"][full["coverage"] != 0])) == 12      # every face of the cube owns texels
    else:                            # the PLY's UVs / the square: the unit square, every texel covered
        assert full["n_covered"] == 561


@pytest.mark.parametrize("name", ["cube", "copy"])
def test_interior_texels_are_at_least_half_of_the_16x16_cube_map(name):
    s = br.reference(name, 16, 16)
    inside = br.interior(s)
    assert 2 * inside.sum() >= s["n_covered"] > 0, (inside.sum(), s["n_covered"])


def test_placed_copy_is_the_mesh_through_its_transform():
    a, b = br.reference("cube", 16, 16), br.reference("copy", 16, 16)
    assert np.array_equal(a["owner"], b["owner"]) and np.array_equal(a["bary"], b["bary"])
    mat, _ = br.prt.make_transform((br.COPY_SRT[0],) * 3, br.COPY_SRT[1], br.COPY_SRT[2])
    M = mat.reshape(4, 4).T.astype(np.float64)
    want = a["position"].reshape(-1, 3).astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    assert np.allclose(b["position"].reshape(-1, 3), want, atol=1e-5)
    wn = a["normal"].reshape(-1, 3).astype(np.float64) @ M[:3, :3].T / br.COPY_SRT[0]
    assert np.allclose(b["normal"].reshape(-1, 3), wn, atol=1e-5)


def test_form_factor_case_keeps_every_texel_between_5_and_95_percent():
    sc, mat = br.ff_scene()
    H, W = br.FF_MAP
    s = br.surface(br.mesh_faces(br.square_mesh()), W, H)
    assert s["n_covered"] == H * W
    p = s["position"].reshape(-1, 3).astype(np.float64)
    n = s["normal"].reshape(-1, 3).astype(np.float64)
    Fq = cf.form_factor(p, n, cf.quad_corners(mat, br.FF_QUAD["width"], br.FF_QUAD["height"]))
    assert Fq.min() >= 0.05 and Fq.max() <= 0.95, (Fq.min(), Fq.max())


# ---- shapes beyond toy maps (br.BIG_SHAPES): what makes each of them a test, shown from the replay alone ------------------------
def _uv(name):
    s = br.shape(name)
    return br.mesh_faces(s["mesh"], s["uvs"])[0]


def _boxes(uv):
    """[F, 4]: min u, max u, min v, max v of every face, in double"""
    u, v = uv[..., 0].astype(np.float64), uv[..., 1].astype(np.float64)
    return np.stack([u.min(1), u.max(1), v.min(1), v.max(1)], 1)


def _sane(s):
    """What the bit-for-bit comparisons on the GPU need of a reference: no NaN anywhere (a NaN has no one bit pattern)"""
    return not (np.isnan(s["position"]).any() or np.isnan(s["normal"]).any() or np.isnan(s["bary"]).any())


def _old_rule(uv, px, py):
    """The rule before the box condition: the signs of the rounded edge functions alone"""
    A2, E0, E1, E2 = br._edges(uv, px, py)
    return ((E0 >= 0) & (E1 >= 0) & (E2 >= 0)) if A2 > 0 else ((E0 <= 0) & (E1 <= 0) & (E2 <= 0))


def test_big_shapes_use_maps_of_several_compaction_trips():
    assert all(H * W > 4 * 1024 for H, W in br.BIG_SIZES) and (128 * 128) % 1024 == 0 and (80 * 96) % 1024 == 512
    for name in br.BIG_SHAPES:
        assert set(br.BIG_SIZES) <= set(br.SHAPE_SIZES[name])
    assert set(br.STRIPS) <= set(br.SHAPE_SIZES["soup"]) and set(br.STRIPS + br.DYADIC) <= set(br.SHAPE_SIZES["grid"])
    assert set(br.SLIVER_SIZES) <= set(br.SHAPE_SIZES["slivers"])


def test_grid_is_98_faces_a_third_of_them_clockwise():
    uv = _uv("grid")
    a, b, c = (uv[:, k].astype(np.float64) for k in range(3))
    A2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    assert len(uv) == 98 and len(uv) % 4 != 0 and (np.abs(A2) == 1.0 / 64.0).all()
    assert 0.25 <= (A2 < 0).mean() <= 0.42, (A2 < 0).mean()
    assert np.array_equal(np.unique(uv), ((4.0 * np.arange(8) + 1.0) / 32.0).astype(F))


@pytest.mark.parametrize("H,W", br.DYADIC)
def test_grid_owner_is_the_lowest_exact_coverer_on_dyadic_maps(H, W):
    uv = _uv("grid")
    s = br.reference("grid", H, W)
    owner, count = br.exact_owner(uv, W, H)
    tied = int((count > 1).sum())
    print(f"grid {H} x {W}: covered {(count > 0).sum()}, tied {tied}, most coverers {count.max()}")
    assert np.array_equal(s["owner"], owner) and np.array_equal(s["coverers"], count) and s["n_degenerate"] == 0
    assert tied > 0
    if (H, W) == (16, 16):      # vertices are texel centres: ties on vertices, axis-aligned edges and diagonals
        assert ((count > 0).sum(), tied, count.max()) == (225, 195, 8)


@pytest.mark.parametrize("H,W", [(24, 24), (17, 33), (80, 96), (100, 100)])
def test_grid_leaves_no_crack_and_claims_nothing_outside(H, W):
    s = br.reference("grid", H, W) if (H, W) in br.SHAPE_SIZES["grid"] else br.surface(br.mesh_faces(br.shape("grid")["mesh"]), W, H)
    px, py = (a.reshape(H, W) for a in br.centres(W, H))
    lo, hi = 1.0 / 32.0, 29.0 / 32.0
    inside = (lo < px) & (px < hi) & (lo < py) & (py < hi)
    outside = (px < lo) | (px > hi) | (py < lo) | (py > hi)
    assert inside.sum() > 100 and outside.sum() > 10
    assert (s["coverage"][inside] == 1).all() and (s["coverage"][outside] == 0).all() and s["n_degenerate"] == 0 and _sane(s)


@pytest.mark.parametrize("H,W", br.SHAPE_SIZES["grid"])
def test_grid_strips_and_large_maps_are_covered_and_uncovered(H, W):
    s = br.reference("grid", H, W)
    assert 0 < s["n_covered"] < H * W and s["n_faces_skipped"] == 0 and _sane(s)


@pytest.mark.parametrize("H,W", br.SHAPE_SIZES["soup"])
def test_soup_conditions(H, W):
    uv = _uv("soup")
    s = br.reference("soup", H, W)
    cov = s["coverage"].ravel() != 0
    share, multi, nothing = cov.mean(), (s["coverers"].ravel()[cov] > 1).mean(), (s["face_texels"] == 0).mean()
    print(f"soup {H} x {W}: covered {share:.3f}, of them with two or more coverers {multi:.3f}, faces covering nothing {nothing:.3f}")
    assert len(uv) == br.SOUP_FACES == 2003 and len(uv) % 4 != 0 and s["n_faces_skipped"] == 0 and s["n_degenerate"] == 0 and _sane(s)
    assert np.array_equal(cov, s["coverers"].ravel() > 0)
    assert 0.30 <= share <= 0.80
    # every 1024-texel stretch of the compaction holds covered and uncovered texels (the strips' last stretch is one texel)
    for start in range(0, H * W, 1024):
        part = cov[start:start + 1024]
        assert len(part) == 1 or (part.any() and not part.all()), start
    assert multi >= 0.10 and nothing >= 0.25
    a, b = br.SOUP_TWINS
    assert np.array_equal(uv[a], uv[b]) and a < b and not (s["owner"] == b).any()
    box = _boxes(uv)
    assert ((box[:, 1] < 0) | (box[:, 0] > 1) | (box[:, 3] < 0) | (box[:, 2] > 1)).any()         # wholly outside the map
    for lo, hi, edge in ((0, 1, 0.0), (0, 1, 1.0), (2, 3, 0.0), (2, 3, 1.0)):                       # across each border
        assert ((box[:, lo] < edge) & (box[:, hi] > edge)).any()
    size = np.maximum(box[:, 1] - box[:, 0], box[:, 3] - box[:, 2])
    assert size.min() < 0.5 / 128 and size.max() > 4.0 / 80      # from below a texel to several across, on the square maps


def test_soup_twins_cover_texels_on_the_square_maps():
    a, b = br.SOUP_TWINS
    s = br.reference("soup", 128, 128)
    assert s["face_texels"][a] == s["face_texels"][b] > 0 and (s["owner"] == a).any()


@pytest.mark.parametrize("H,W", br.SHAPE_SIZES["huge"])
def test_huge_faces_cover_the_map_and_small_faces_keep_their_texels(H, W):
    uv = _uv("huge")
    s = br.reference("huge", H, W)
    assert len(uv) == 6 and np.abs(uv[4:]).max() == 2.0 ** 20 and s["n_faces_skipped"] == 0 and _sane(s)
    n = H * W
    assert s["face_texels"][3] == n and s["face_texels"][4] == n and s["face_texels"][5] == 0
    assert s["n_covered"] == n and s["n_degenerate"] == 0
    alone = br.surface(tuple(a[:3] for a in br.mesh_faces(br.shape("huge")["mesh"])), W, H)
    for f in range(3):
        assert (alone["owner"] == f).sum() > 8 and np.array_equal(s["owner"] == f, alone["owner"] == f)
    assert np.array_equal(s["owner"] == 3, alone["owner"] == br.NONE) and not (s["owner"] >= 4).any()


@pytest.mark.parametrize("H,W", br.SHAPE_SIZES["slivers"])
def test_slivers_own_nothing_outside_their_boxes(H, W):
    uv = _uv("slivers")
    s = br.reference("slivers", H, W)
    box = _boxes(uv)
    px, py = (a.reshape(H, W) for a in br.centres(W, H))
    own = s["owner"] != br.NONE
    b = box[s["owner"][own].astype(np.int64)]
    assert ((b[:, 0] <= px[own]) & (px[own] <= b[:, 1]) & (b[:, 2] <= py[own]) & (py[own] <= b[:, 3])).all()
    assert 24 <= len(uv) <= 60 and _sane(s) and np.isfinite(s["position"]).all()
    assert (np.abs(uv)[uv != 0].min() < 1.2e-38) and (uv == F(1e-30)).any()      # subnormal and 1e-30 third vertices
    # without the box condition some face claims a texel outside its box
    stray = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(len(uv)):
            new = br.covers(uv[f], px.ravel(), py.ravel())[0]
            if new is None:
                continue
            old = _old_rule(uv[f], px.ravel(), py.ravel())
            assert not (new & ~old).any()
            stray += int((old & ~new).sum())
    print(f"slivers {H} x {W}: covered {s['n_covered']}, texels the rule without the box would add: {stray}")
    if (H, W) in br.SLIVER_SIZES:
        assert stray > 0 and s["n_covered"] > 0


def test_sliver_0_covers_8_3_and_2_texels_where_the_signs_alone_give_the_whole_diagonal():
    uv = _uv("slivers")[0]
    assert np.array_equal(uv, np.array(br.SLIVER_0, F))
    want = {(16, 16): 8, (17, 17): 3, (12, 12): 2}
    for (H, W), n in want.items():
        px, py = br.centres(W, H)
        new, A2, _, _ = br.covers(uv, px, py)
        old = _old_rule(uv, px, py)
        assert A2 != 0.0 and new.sum() == n and old.sum() > n, (H, W, new.sum(), old.sum())
        assert (px[new] <= 0.5).all() and (py[new] <= 0.5).all() and (px[old].max() > 0.9)
    px, py = br.centres(16, 16)
    old = _old_rule(uv, px, py)
    assert old.sum() == 16 and np.array_equal(old, px == py)        # all 16 texels of the diagonal; 8 lie on the face's edge


@pytest.mark.parametrize("name", ["bunny", "ico_copy"])
def test_scanned_meshes_under_a_planar_projection_overlap_front_and_back(name):
    mesh = br.shape(name)["mesh"]
    assert mesh.n_triangles >= (20_000 if name == "bunny" else 2000) and br.shape(name)["placed"] == (name == "ico_copy")
    for H, W in br.SHAPE_SIZES[name]:
        s = br.reference(name, H, W)
        cov = s["coverage"].ravel() != 0
        multi = (s["coverers"].ravel()[cov] > 1).mean()
        print(f"{name} {H} x {W}: covered {cov.mean():.3f}, two or more coverers {multi:.3f}, faces covering nothing {(s['face_texels'] == 0).mean():.3f}")
        assert 0.3 <= cov.mean() < 1.0 and multi >= 0.9 and s["n_degenerate"] == 0 and s["n_faces_skipped"] == 0 and _sane(s)
        assert (s["face_texels"] == 0).mean() >= (0.25 if name == "bunny" else 0.0)      # sub-texel faces
        n = s["normal"].reshape(-1, 3)[cov].astype(np.float64)
        assert np.allclose((n ** 2).sum(1), 1.0, atol=1e-6)


def test_soup_has_gutters_that_one_pass_does_not_fill():
    cov = br.reference("soup", 80, 96)["coverage"]
    ones = np.ones((80, 96, 3), F)
    c1, _, n1 = br.dilate(cov, ones, 1)
    c2, _, n2 = br.dilate(cov, ones, 2)
    _, _, n4 = br.dilate(cov, ones, 4)
    second = (c2 == 2) & (c1 == 0)        # filled by pass 2: none of their neighbours is owned, all they see was filled by pass 1
    padded = np.pad(cov, 1)
    owned_near = sum(padded[1 + di:81 + di, 1 + dj:97 + dj] for di, dj in br.NEIGHBOURS)
    assert 0 < n1 < n2 < n4 and second.sum() == n2 - n1 and not owned_near[second].any()


@pytest.mark.parametrize("name,H,W", [("grid", 24, 24), ("grid", 17, 33), ("grid", 7, 5), ("grid", 100, 100), ("soup", 80, 96), ("soup", 1, 2049),
                                      ("huge", 33, 129)])
def test_box_condition_changes_nothing_for_well_conditioned_faces(name, H, W):
    uv = _uv(name)
    px, py = br.centres(W, H)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(len(uv)):
            new = br.covers(uv[f], px, py)[0]
            assert new is not None and np.array_equal(new, _old_rule(uv[f], px, py)), f
