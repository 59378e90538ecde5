"""The numpy restatement of surface baking (tests/bake_replay.py) against what the header promises, without a GPU: the
coverage rule on small layouts whose answer is known by hand, and the conditions the GPU tests (tests/test_gpu_bake.py)
rely on, shown from the reference alone."""
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
