"""CPU-side checks of the texture restatement (tests/texture_replay.py), before any GPU run relies on it.

The gate: on every hit of every test scene (primary rays, random rays and every vertex of walked paths) the position that
hit_uv() restates from Triangle::Intersect / Quad::Intersect equals OracleScene.closest_hit's position bit for bit.  Then the
laws of the lookup, the 1 x 1 law of the walker, and the share of undecidable samples of the lighting cases that
tests/test_gpu_textures.py and tests/test_gpu_texture_instances.py replay (within lighting_replay.MAX_UNSTABLE, as the existing
replay tests assert it)."""
import numpy as np
import pytest

import environment_replay as er
import lighting_replay as lr
import texture_replay as tr
from util import orc, prt

F = np.float32


def _same(a, b):
    """bit for bit, except that -0.0 == +0.0 and a NaN on both sides is agreement (util.hits_equal's rule)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


CASES = {"A": lambda: tr.scene_a(), "B": lambda: tr.scene_b(), "B_light": lambda: tr.scene_b(emissive_copy=True),
         "C": lambda: tr.scene_c(emissive_mesh=True), "D": lambda: tr.scene_d(emissive_copy=True), "Q_small": lambda: tr.scene_q(),
         "Q_big": lambda: tr.scene_q(big=True), "E": lambda: tr.scene_e(emissive_mesh=True)}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    c = CASES[request.param]()
    c["osc"] = orc.OracleScene(c["scene"].desc())
    return c


def test_vectorised_transforms_equal_the_oracles():
    rng = np.random.default_rng(1)
    mat, inv = prt.make_transform((0.45, 0.45, 0.45), (15.0, 30.0, 0.0), (-1.6, -0.3, 0.6))
    p = rng.normal(size=(200, 3)).astype(F) * F(3.0)
    for m in (mat, inv):
        assert _same(tr.transform_point(m, p), np.stack([orc.transform_point(m, v) for v in p]))
        assert _same(tr.transform_normal(m, p), np.stack([orc.transform_normal(m, v) for v in p]))


def test_gate_restated_positions_equal_the_oracles_bit_for_bit(case):
    ts = tr.TexScene(case["scene"])
    o, d = tr.primary_and_random_rays(case)
    hits = case["osc"].closest_hit(o, d, use_bvh=True, n_threads=lr.n_threads_default())
    uv, pos = ts.hit_uv(o, d, hits)
    hit = hits["prim"] >= 0
    assert hit.sum() > 0.5 * len(o)
    prim = hits["prim"][hit]
    quads = [q for q, p in enumerate(case["scene"].primitives) if p.shape_type == prt.capi.SHAPE_QUAD]
    kinds = {"quad": np.isin(prim, quads), "world": (prim >= ts.n_prims) & (prim < ts.n_prims + ts.n_world), "copy": prim >= ts.n_prims + ts.n_world}
    has = {"quad": len(quads) > 0, "world": ts.n_world > 0, "copy": len(ts.inst) > 0}
    if "rotated_quads" in case:    # C, D, Q: quads turned about at least two axes, and quads hit on their back faces
        kinds["rotated quad"] = np.isin(prim, case["rotated_quads"])
        kinds["back of a quad"] = kinds["quad"] & (hits["front_face"][hit] == 0)
        kinds["back of a rotated quad"] = kinds["rotated quad"] & kinds["back of a quad"]
        has.update({"rotated quad": True, "back of a quad": True, "back of a rotated quad": True})
        assert len(case["rotated_quads"]) >= 4 and len(case["scene"].primitives) != 0
    if case["name"] in ("C", "D", "Q_big"):
        assert len(case["scene"].primitives) >= 20
    if case["name"].startswith("Q"):
        assert not has["world"] and not has["copy"]
    assert all(kinds[k].sum() > 20 for k in kinds if has[k]), {k: int(v.sum()) for k, v in kinds.items()}
    assert all(kinds[k].sum() == 0 for k in kinds if not has[k])
    assert _same(pos[hit], hits["position"][hit])
    # and at every vertex of walked paths (scattered rays from every kind of surface), jittered
    W, H = case["W"], case["H"]
    pix = np.tile(np.arange(W * H), 2)
    samp = np.repeat([0, 1], W * H)
    verts, _, _, _ = tr.walk(case["scene"], case["osc"], case["cam"], W, H, case["depth"], tr.SEED, pix, samp, (1, 0, 0.0), True)
    assert len(verts) == case["depth"]
    for v in verts:
        h = v["hit"]["prim"] >= 0
        uv2, pos2 = ts.hit_uv(v["o"], v["d"], v["hit"])
        assert _same(pos2[h], v["hit"]["position"][h])
        assert np.all(np.isfinite(uv2))


def test_untextured_and_one_by_one_walks_equal_the_plain_walk():
    """A scene without textures walks exactly as lighting_replay.walk does, and a 1 x 1 texture of colour c exactly as a
    material of albedo c (nearest, both wraps)."""
    none, flat = tr.scene_a("none"), tr.scene_a("flat")
    osc = orc.OracleScene(none["scene"].desc())
    W, H = none["W"], none["H"]
    pix = np.tile(np.arange(W * H), 3)
    samp = np.repeat([0, 1, 4], W * H)
    for smp in ((0, 0, 0.0), (1, 2, 1.5)):
        ref = lr.walk(none["scene"], osc, none["cam"], W, H, 4, tr.SEED, pix, samp, smp, True)
        for c in (none, flat):
            got = tr.walk(c["scene"], osc, c["cam"], W, H, 4, tr.SEED, pix, samp, smp, True)
            assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)) and got[3] == ref[3]
            assert np.array_equal(got[2], ref[2])
            for a, b in zip(got[0], ref[0]):
                assert np.array_equal(a["albedo"], b["albedo"]) and np.array_equal(a["thr"], b["thr"])
    # the oracle's own render agrees with the plain walk (the walker's licence, as in test_lighting_replay.py)
    acc, wts, _ = tr.frame(none["scene"], osc, none["cam"], W, H, 4, tr.SEED, 0, 2)
    want, wwant, _ = osc.render(none["cam"].desc(), W, H, spp=2, first_sample=0, max_depth=4, seed=tr.SEED, iterative=True, use_bvh=True, n_threads=4)
    assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)) and np.array_equal(wts, wwant)
    # and a checker changes what is delivered
    full = tr.scene_a("full")
    assert not np.array_equal(tr.frame(full["scene"], osc, full["cam"], W, H, 4, tr.SEED, 0, 1)[0], tr.frame(none["scene"], osc, none["cam"], W, H, 4, tr.SEED, 0, 1)[0])


# ---- laws of the lookup ------------------------------------------------------------------------------------------------------
IMG = np.random.default_rng(9).uniform(0.0, 1.0, size=(5, 3, 3)).astype(F)


def test_repeat_of_u_plus_3_equals_u_for_dyadic_u():
    k = np.arange(0, 64, dtype=F) / F(64.0)
    uu, vv = [a.ravel() for a in np.meshgrid(k, k)]
    for filt in (0, 1):
        a = tr.lookup(IMG, filt, 0, uu, vv)
        b = tr.lookup(IMG, filt, 0, uu + F(3.0), vv - F(2.0))
        assert np.array_equal(a, b)


def test_clamp_outside_the_unit_square_returns_the_border_texel():
    H, W = IMG.shape[:2]
    v = np.array([0.1, 0.5, 0.9], F)
    for filt in (0, 1):
        assert np.array_equal(tr.lookup(IMG, filt, 1, np.full(3, -0.7, F), np.full(3, -3.0, F)), np.tile(IMG[H - 1, 0], (3, 1)))
        assert np.array_equal(tr.lookup(IMG, filt, 1, np.full(3, 1.7, F), np.full(3, 9.0, F)), np.tile(IMG[0, W - 1], (3, 1)))
    # nearest, clamp: left of 0 the first column at the row of v, right of 1 the last
    rows = np.minimum(H - 1, np.floor((F(1.0) - v) * F(H)).astype(int))
    assert np.array_equal(tr.lookup(IMG, 0, 1, np.full(3, -2.0, F), v), IMG[rows, 0])
    assert np.array_equal(tr.lookup(IMG, 0, 1, np.full(3, 2.0, F), v), IMG[rows, W - 1])


def test_bilinear_at_texel_centres_returns_the_texel():
    # sizes whose centres are exact in binary: (j + 0.5) / W * W - 0.5 = j with fx = 0
    img = np.random.default_rng(4).uniform(0.0, 1.0, size=(4, 8, 3)).astype(F)
    H, W = img.shape[:2]
    j, i = [a.ravel() for a in np.meshgrid(np.arange(W), np.arange(H))]
    u = (j.astype(F) + F(0.5)) / F(W)
    v = F(1.0) - (i.astype(F) + F(0.5)) / F(H)
    for wrp in (0, 1):
        assert np.array_equal(tr.lookup(img, 1, wrp, u, v), img[i, j])
    assert np.array_equal(tr.lookup(img, 0, 0, u, v), img[i, j])
    # a 1 x 1 image is its texel everywhere
    one = np.array([[[0.25, 0.5, 0.75]]], F)
    g = tr.eval_grid(3, 5)
    for wrp in (0, 1):
        assert np.array_equal(tr.lookup(one, 0, wrp, g[:, 0], g[:, 1]), np.tile(one[0, 0], (len(g), 1)))
        # (bilinear blends four copies of the texel with weights that sum to 1 only before rounding: within 2 ulp, not equal)
        assert np.allclose(tr.lookup(one, 1, wrp, g[:, 0], g[:, 1]), one[0, 0], rtol=3e-7, atol=0)


# ---- the lighting cases of tests/test_gpu_textures.py and tests/test_gpu_texture_instances.py: the replays' undecidable share -
@pytest.mark.parametrize("name", tr.LIGHTING_CASES + tr.INSTANCE_LIGHTING_CASES)
def test_lighting_cases_stay_within_the_replays_unstable_share(monkeypatch, name):
    """Undecidable over light samples (and misses, with an environment) of the cases of scenes C, D and E, as printed:
      C_mis_analytic 0 / 5776    C_nee_mesh 0 / 5740    C_mis_env 1 (share 0.0001)    C_nee_mesh_env 1 (0.0001)
      D_nee_analytic 0 / 5730    D_mis_mesh 0 / 5694    D_nee_analytic_env 1 (0.0001) D_mis_mesh_env 1 (0.0001)
      E_mis_analytic 0 / 3283    E_nee_mesh 0 / 3283    E_mis_env 0 / 3283            E_nee_mesh_env 0 / 3283
    against the cap lighting_replay.MAX_UNSTABLE = 0.005."""
    tr.patch_walk(monkeypatch)
    c, mode, fn = tr.lighting_case(name)
    rep = fn(c, orc.OracleScene(c["scene"].desc()))
    share = er.unstable_share(rep) if "env" in name else lr.unstable_share(rep)
    print(name, "light samples", rep.n_light_samples, "unstable", rep.n_unstable, "share", share)
    assert rep.n_light_samples > 1000
    assert share <= lr.MAX_UNSTABLE
    assert rep.stable.mean() >= 0.995
    if "mesh" in name and "env" not in name:
        print(name, "triangle samples", rep.n_triangle_samples)
        assert rep.n_triangle_samples >= 20      # the triangle lights are sampled
    # the textured albedo is in the replayed values: they differ from the untextured scene's
    if name == "A_mis_analytic":
        plain = tr.scene_a("none")
        monkeypatch.undo()
        ref = lr.replay_case(plain, "mis")
        assert np.abs(ref.value - rep.value).max() > 0.05
