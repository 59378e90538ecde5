"""Clustered light selection (include/prt.h "Clustered light selection", prt_set_light_selection) on one MI355X.

  1. prt_light_cluster_pmf (the render's own cluster_thresholds) equals the numpy float32 restatement of the contract bit
     for bit, on one cluster, on NEAR_FAR at 2 clusters and on bunny + quad + sphere at 64: random points, points inside a
     box, on a box face, 10^6 away and near 10^20 (D2 overflows: the fallback); and on two meshes 10^6 apart, where
     from beside one of them the other cluster's interval is empty (M_c = M_{c-1}).
  2. prt_sample_light on the same scenes: the light equals the replay's, the numbers are within the tolerances of
     test_gpu_mesh_lights.test_sample_light_matches_float64_for_triangles.
  3. Every sample of one-sample 320 x 240 frames against the float64 replay (tests/light_cluster_replay.py), the existing
     per-term tolerances unchanged, both lighting modes: NEAR_FAR, an emissive placed copy under a quad light, bunny_light
     with an environment, a textured ground.
  4. Routes bit-identical to one another: group of 3 ranks, 1 against 16 samples in flight; after Refit and UpdateInstances
     frames equal a fresh scene of the moved geometry.
  5. The default is untouched: never asked, "power", and "clustered" under the "analytic" mask give identical films through
     the existing shade instance.
  6. Unbiased: power, clustered and lighting off agree within the sampling error on bunny_light.
  7. Variance: the ratio clustered / power on NEAR_FAR's ground pixels agrees with the replay's R_ref."""
import numpy as np
import pytest

import closed_form as cf
import environment_replay as er
import light_cluster_replay as lcr
import lighting_replay as lr
import mesh_light_replay as mr
import texture_replay as tr
import util
from parallelraytracing_amd import scenes
from test_gpu_mesh_lights import _agree
from util import orc, prt

pytestmark = pytest.mark.gpu

SEED = 11
TWO24 = 1 << 24


def _renderer(c, mode="mis", selection="clustered", K=8, sif=16, group=False, sources="all", env=None, seed=mr.SEED):
    film = prt.Film(c["W"], c["H"])
    if group:
        r = prt.HipWavefrontGroupRenderer([0, 0, 0], max_depth=c["depth"], seed=seed)
    else:
        r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=seed)
    if sources is not None:
        r.set_light_sources(sources)
    if selection is not None:
        r.set_light_selection(selection, K)
    if env is not None:
        r.set_environment(env[0], env[1])
    r.Init(film, c["scene"], c["cam"])
    r.set_samples_in_flight(sif)
    r.set_lighting(mode)
    return r, film


def _one_cluster_scene():
    """A sphere light, a world-space emissive icosahedron and a rotated, scaled emissive placed copy above the ground."""
    sc = prt.Scene(preset=None, sky=cf.SKY)
    g = sc.AddLambertian(cf.GROUND_ALBEDO)
    e = sc.AddEmissive(cf.EMISSION)
    e2 = sc.AddEmissive((2.0, 3.0, 4.0))
    sc.AddQuad(20.0, 20.0, g, translation=(0.0, -1.0, 0.0))
    sc.AddCircle(0.5, e2, scale=(2.0, 2.0, 2.0), translation=(3.0, 3.0, 1.0))
    ico = prt.Mesh(scenes.asset("icosahedron.ply"))
    up = ico.copy()
    mat, inv = scenes.make_transform((1, 1, 1), (0, 0, 0), (-2.0, 4.0, 0.5))
    up.transform(mat, inv)
    sc.AddMesh(up, e)
    sc.AddInstance(ico, e2, scale=1.7, euler_deg=(25.0, 40.0, 10.0), translation=(1.0, 5.0, -1.0))
    return sc


def _bunny_quad_sphere_scene():
    """An emissive 2,000-triangle bunny, a quad light and a sphere light above the ground."""
    sc = prt.Scene(preset=None, sky=cf.SKY)
    g = sc.AddLambertian(cf.GROUND_ALBEDO)
    e = sc.AddEmissive((4.0, 3.0, 2.0))
    e2 = sc.AddEmissive((6.0, 8.0, 12.0))
    e3 = sc.AddEmissive(cf.EMISSION)
    sc.AddQuad(20.0, 20.0, g, translation=(0.0, -1.0, 0.0))
    sc.AddCircle(0.25, e2, scale=(2.0, 2.0, 2.0), translation=(-4.0, 1.0, 2.0))
    sc.AddQuad(1.0, 1.0, e3, euler_deg=(180.0, 0.0, 0.0), translation=(5.0, 4.0, -3.0))
    sc.AddMesh(scenes.refined("bunny.ply", 2000), e)
    return sc


def _scene_case(name):
    if name == "one_cluster":
        return dict(scene=_one_cluster_scene(), K=1)
    if name == "near_far":
        return dict(scene=lcr.near_far()["scene"], K=2)
    return dict(scene=_bunny_quad_sphere_scene(), K=64)


SCENES = ("one_cluster", "near_far", "bunny_quad_sphere")


@pytest.fixture(scope="module", params=SCENES)
def ctx(request):
    s = _scene_case(request.param)
    W, H = 64, 48
    c = dict(scene=s["scene"], cam=cf.camera(prt, "ground", W, H), W=W, H=H, depth=5)
    r, _ = _renderer(c, K=s["K"])
    t = lcr.read_tables(r)
    return dict(name=request.param, r=r, tables=t, scene=s["scene"], K=s["K"])


def _points(t, rng):
    lo, hi = t["lo"].astype(np.float64), t["hi"].astype(np.float64)
    K = len(lo)
    pick = lambda n: rng.integers(0, K, n)   # noqa: E731
    rnd = rng.uniform(-12.0, 12.0, (2000, 3))
    c = pick(500)
    inside = lo[c] + rng.uniform(0.0, 1.0, (500, 3)) * (hi[c] - lo[c])
    c = pick(500)
    face = lo[c] + rng.uniform(0.0, 1.0, (500, 3)) * (hi[c] - lo[c])
    ax, side = rng.integers(0, 3, 500), rng.integers(0, 2, 500)
    face[np.arange(500), ax] = np.where(side == 1, hi[c, ax], lo[c, ax])
    d = rng.normal(size=(500, 3))
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * 1e6 * rng.uniform(0.5, 2.0, (500, 1))
    d = rng.normal(size=(500, 3))
    huge = d / np.linalg.norm(d, axis=1, keepdims=True) * 1e20 * rng.uniform(0.5, 2.0, (500, 1))
    return dict(random=rnd, inside=inside, face=face, far=far, huge=huge)


def test_cluster_pmf_equals_the_float32_restatement_bit_for_bit(ctx):
    r, t = ctx["r"], ctx["tables"]
    K = r.light_cluster_info().n_clusters
    assert K == (ctx["K"] if ctx["name"] != "one_cluster" else 1)
    if ctx["name"] == "bunny_quad_sphere":
        assert (t["n_members"] == 1).sum() >= 2          # the quad and the sphere sit alone
    pts = _points(t, np.random.default_rng(17))
    for kind, p in pts.items():
        x = p.astype(np.float32)
        got = r.light_cluster_pmf(x)
        want = lcr.thresholds(t, x)
        assert got.shape == want.shape == (len(x), K)
        assert np.array_equal(got, want), (ctx["name"], kind, int((got != want).any(1).sum()))
        assert np.all(got[:, -1] == TWO24) and np.all(np.diff(got.astype(np.int64), axis=1) >= 0)
        if kind == "huge" and K > 1:
            phi = t["phi"].astype(np.float64)
            P = np.diff(np.concatenate([np.zeros((len(x), 1)), got.astype(np.float64)], axis=1), axis=1) / TWO24
            assert np.all(np.abs(P - phi[None, :]) <= 2.0 ** -22), kind                  # the fallback: P_c = phi_c
        if kind == "inside" and K > 1:
            assert (np.diff(got.astype(np.int64), axis=1) > 0).any()
    x = np.random.default_rng(19).uniform(-12.0, 12.0, (max(util.WORKSPACE_COUNTS), 3)).astype(np.float32)
    for n in util.WORKSPACE_COUNTS:
        assert np.array_equal(r.light_cluster_pmf(x[:n]), lcr.thresholds(t, x[:n])), (ctx["name"], n)


def test_cluster_pmf_with_a_cluster_that_is_never_drawn():
    """Two emissive icosahedra 10^6 apart, two clusters: from a point beside one of them the other's interval is empty
    (M_c = M_{c-1}), and the device and the restatement agree on that too."""
    sc = prt.Scene(preset=None, sky=cf.SKY)
    g = sc.AddLambertian(cf.GROUND_ALBEDO)
    e = sc.AddEmissive(cf.EMISSION)
    sc.AddQuad(20.0, 20.0, g, translation=(0.0, -1.0, 0.0))
    ico = prt.Mesh(scenes.asset("icosahedron.ply"))
    v, nr, idx = ico.GetVertices(), ico.GetNormals(), ico.GetIndices()
    for tx in (0.0, 1.0e6):
        sc.AddMesh(prt.Mesh(vertices=(v + np.array([tx, 1.0, 0.0], np.float32)).astype(np.float32), normals=nr, indices=idx), e)
    W, H = 64, 48
    r, _ = _renderer(dict(scene=sc, cam=cf.camera(prt, "ground", W, H), W=W, H=H, depth=5), K=2)
    t = lcr.read_tables(r)
    assert r.light_cluster_info().n_clusters == 2 and list(t["n_members"]) == [20, 20]
    rng = np.random.default_rng(3)
    near = rng.uniform(-12.0, 12.0, (1000, 3))
    x = np.concatenate([near, near + np.array([1.0e6, 0.0, 0.0]), rng.uniform(-2.0e6, 2.0e6, (1000, 3))]).astype(np.float32)
    got = r.light_cluster_pmf(x)
    assert np.array_equal(got, lcr.thresholds(t, x))
    # the far cluster's interval is empty, or one unit of 2^-24 where the near one's share rounds below 1
    assert np.all(got[:1000, 0] >= TWO24 - 1) and (got[:1000, 0] == TWO24).sum() > 500
    assert np.all(got[1000:2000, 0] <= 1) and (got[1000:2000, 0] == 0).sum() > 500
    assert ((got[2000:, 0] > 0) & (got[2000:, 0] < TWO24)).any()


def test_sample_light_matches_the_replay(ctx):
    r, t, sc = ctx["r"], ctx["tables"], ctx["scene"]
    lights = lcr.light_set(sc, t)
    prim, _ = r.light_info()
    assert np.array_equal(prim.astype(np.int64), lights.prim)
    rng = np.random.default_rng(5)
    n = 20000
    o = np.column_stack([rng.uniform(-8, 8, n), np.full(n, 1.5), rng.uniform(-8, 8, n)]).astype(np.float32)
    d = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (n, 1))
    o[:, 1] = 6.0 if ctx["name"] == "one_cluster" else 1.5
    hits = r.closest_hit(o, d)
    ground = hits["prim"] == 0
    assert ground.sum() > 0.8 * n
    hits, d = hits[ground], d[ground]
    n = len(hits)
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    alb = np.asarray(sc.materials[0].rgb[:], np.float32).astype(np.float64)
    for mode in ("mis", "nee"):
        r.set_lighting(mode)
        out = r.sample_light(d, hits, keys)
        x = hits["position"].astype(np.float64)
        nrm = hits["normal"].astype(np.float64)
        s = lcr.sample_lights(lights, x, nrm, keys, mode)
        ok = s["valid"]
        assert ok.sum() > 0.5 * n
        assert np.array_equal(out["light"][ok], s["light"][ok].astype(np.uint32))      # no band: cluster and member are equal
        assert np.all(out["light"][~ok] == 0xFFFFFFFF)
        contrib = alb * lights.Le[s["light"]] * s["f"][:, None]
        np.testing.assert_allclose(out["dir"][ok], s["w"][ok], atol=2e-6)
        np.testing.assert_allclose(out["tmax"][ok], s["tmax"][ok], rtol=1e-5)
        ok = ok & (s["cos_l"] >= mr.COS_MIN) & (s["margin_band"] >= 1e-5)
        c = 8.0 * mr.U / np.maximum(s["cos_l"], mr.COS_MIN)

        def close(got, want, rtol, atol=0.0, sel=ok):
            err = np.abs(got[sel].astype(np.float64) - want[sel])
            lim = atol + (rtol + c[sel]).reshape((-1,) + (1,) * (want.ndim - 1)) * np.abs(want[sel])
            assert np.all(err <= lim), float((err / np.maximum(lim, 1e-300)).max())

        close(out["pdf_light"], s["pdf_l"], 1e-5)
        np.testing.assert_allclose(out["pdf_bsdf"][ok], s["pb"][ok], rtol=1e-5, atol=1e-7)
        close(out["w_light"], s["wl"], 1e-5, 1e-6)
        close(out["contrib"], contrib, 1e-5, 1e-6)
        pb, pl = s["pb"], s["pdf_l"]
        both = ok & (pb > 0) & (pl > 0)
        wb = lcr.hit_weight(lights, lights.prim[s["light"]], x, s["w"], s["t_light"] ** 2, pb, mode)[0]
        if mode == "mis":
            np.testing.assert_allclose(out["w_light"][both] + out["w_bsdf"][both], 1.0, atol=2e-6)
            close(out["w_bsdf"], wb, 1e-4, 1e-6, sel=both)
        else:
            assert np.all(out["w_bsdf"][both] == 0.0) and np.all(out["w_light"][both] == 1.0)
            assert np.all(wb[both] == 0.0)


# ---- 3. every sample against the replay ---------------------------------------------------------------------------------------
def _replay_case(name):
    """-> (case, K, env or None, replay function of (case, mode, tables, osc), check function)"""
    if name == "NEAR_FAR":
        c = dict(lcr.near_far(320, 240), depth=5)
        return c, 2, None, lambda c, mode, t, osc: lcr.replay_case(c, mode, t, osc=osc), "mesh"
    if name == "placed":
        return mr.case("placed"), 8, None, lambda c, mode, t, osc: lcr.replay_case(c, mode, t, osc=osc), "mesh"
    if name == "bunny_light_env":
        c = dict(mr.case("bunny_light"), sources="all", env="sun", light_share=0.5)

        def rep(c, mode, t, osc):
            with lcr.clustered(t):
                return er.replay_case(c, mode, osc=osc)
        return c, 8, (er.named_map("sun"), 0.5), rep, "env"
    if name == "textured_ground":
        c, _, _ = tr.lighting_case("B_mis_mesh")

        def rep(c, mode, t, osc):
            with lcr.clustered(t):
                return mr.replay_case(c, mode, osc=osc, sources="all")
        return c, 8, None, rep, "mesh"
    raise ValueError(name)


@pytest.mark.parametrize("name", ("NEAR_FAR", "placed", "bunny_light_env", "textured_ground"))
def test_every_sample_matches_the_float64_replay(record_property, monkeypatch, name):
    c, K, env, replay, kind = _replay_case(name)
    if name == "textured_ground":
        tr.patch_walk(monkeypatch)
    osc = orc.OracleScene(c["scene"].desc())
    for mode in ("mis", "nee"):
        r, film = _renderer(c, mode, K=K, env=env)
        assert r.light_cluster_info().active == 1
        t = lcr.read_tables(r)
        rep = replay(c, mode, t, osc)
        r.reset_stats()
        frames = mr.render_samples(r, film, mr.SAMPLES)
        r.synchronize()
        assert "k_shade_nee_clus" in r.shade_instance()
        if kind == "env":
            assert r.environment_info().t_env == int(rep.t_env) and rep.t_env > 0
            rec = er.check_against_gpu(rep, frames, r.light_stats())
        else:
            rec = mr.check_gpu(rep, frames, r.light_stats(), r.light_info(), r.light_intervals())
        rec.update(case=name, mode=mode)
        record_property("light_cluster_replay", rec)
        assert rec["compared"] >= 0.995 * len(rep.pix)
        del r


# ---- 4. routes ------------------------------------------------------------------------------------------------------------------
def test_other_routes_are_bit_identical():
    c = mr.case("placed")
    r, film = _renderer(c, "mis")
    ref = mr.render_samples(r, film, mr.SAMPLES)
    tables = lcr.read_tables(r)
    del r
    r, film = _renderer(c, "mis", sif=1)
    got = mr.render_samples(r, film, mr.SAMPLES)
    for s in mr.SAMPLES:
        assert np.array_equal(got[s].view(np.uint32), ref[s].view(np.uint32)), ("sif 1", s)
    del r
    g, film = _renderer(c, "mis", group=True)
    got = mr.render_samples(g, film, mr.SAMPLES, clear=g.Clear)
    for s in mr.SAMPLES:
        assert np.array_equal(got[s].view(np.uint32), ref[s].view(np.uint32)), ("group", s)
    gt = dict(g.light_clusters())
    gt["cluster"], gt["inner_width"] = g.light_cluster_members()
    for k in tables:
        assert np.array_equal(tables[k], gt[k]), k
    for rank in range(3):
        assert g.light_cluster_info(rank).active == 1
    x = np.random.default_rng(2).uniform(-5, 5, (64, 3)).astype(np.float32)
    assert np.array_equal(g.light_cluster_pmf(x, rank=2), lcr.thresholds(tables, x))
    del g
    # the selection switched on after Init gives the same frames
    r, film = _renderer(c, "mis", selection=None)
    r.set_light_selection("clustered", 8)
    got = mr.render_samples(r, film, mr.SAMPLES)
    for s in mr.SAMPLES:
        assert np.array_equal(got[s].view(np.uint32), ref[s].view(np.uint32)), ("late", s)


def _frames(r, film, n=2):
    film.Clear()
    r.frame_index = 0
    r.ProgressiveRender(n)
    r.download()
    return film.accum.copy()


def test_refit_and_instance_update_equal_a_fresh_scene():
    base = scenes.refined("bunny.ply", 2000)
    v = base.GetVertices().copy()
    v[:, 0] += 0.03 * np.sin(3.0 * v[:, 1])
    v *= np.float32(1.1)
    moved = prt.Mesh(vertices=v, normals=base.GetNormals(), indices=base.GetIndices())
    ico = prt.Mesh(scenes.asset("icosahedron.ply"))

    def scene(mesh, shift):
        """shift None: the world mesh `mesh` alone (prt_refit_meshes takes no scene with placed copies); otherwise the
        bunny is a fixed world mesh and an emissive placed copy sits where `shift` puts it."""
        sc = prt.Scene(preset=None, sky=cf.SKY)
        g = sc.AddLambertian(cf.GROUND_ALBEDO)
        e = sc.AddEmissive((4.0, 3.0, 2.0))
        e2 = sc.AddEmissive((6.0, 8.0, 12.0))
        sc.AddQuad(20.0, 20.0, g, translation=(0.0, -1.0, 0.0))
        sc.AddCircle(0.25, e2, scale=(2.0, 2.0, 2.0), translation=(-2.0, 0.2, 1.0))
        sc.AddMesh(mesh, e)
        if shift is not None:
            sc.AddInstance(ico, e2, scale=0.5 + 0.2 * shift, euler_deg=(10.0, 25.0 + 40.0 * shift, 0.0), translation=(2.5 - 4.0 * shift, 0.5 + shift, 1.0))
        return sc
    W, H = 96, 54
    cam = prt.Camera(position=(2.0, 1.5, 3.0), width=W, height=H)

    def ctx_of(sc):
        return _renderer(dict(scene=sc, cam=cam, W=W, H=H, depth=5), "mis", K=8, seed=3)
    fresh = {}
    for key, sc in (("refit", scene(moved, None)), ("update", scene(base, 1.0))):
        r, film = ctx_of(sc)
        fresh[key] = (lcr.read_tables(r), _frames(r, film))
        del r
    r, film = ctx_of(scene(base, None))
    before = lcr.read_tables(r)
    _frames(r, film)
    r.Refit(scene(moved, None))
    t = lcr.read_tables(r)
    assert not np.array_equal(before["lo"], t["lo"])
    for k in t:
        assert np.array_equal(t[k], fresh["refit"][0][k]), ("refit", k)
    assert np.array_equal(_frames(r, film).view(np.uint32), fresh["refit"][1].view(np.uint32))
    del r
    r, film = ctx_of(scene(base, 0.0))
    before = lcr.read_tables(r)
    _frames(r, film)
    r.UpdateInstances(scene(base, 1.0), "refit")
    t = lcr.read_tables(r)
    assert not np.array_equal(before["lo"], t["lo"])
    for k in t:
        assert np.array_equal(t[k], fresh["update"][0][k]), ("update", k)
    assert np.array_equal(_frames(r, film).view(np.uint32), fresh["update"][1].view(np.uint32))


# ---- 5. the default --------------------------------------------------------------------------------------------------------------
def test_the_default_is_untouched():
    c = mr.case("placed", 160, 120)
    films, names = {}, {}
    for label, kw in (("never", dict(selection=None)), ("power", dict(selection="power")), ("never_analytic", dict(selection=None, sources=None)),
                      ("clustered_analytic", dict(selection="clustered", sources="analytic"))):
        r, film = _renderer(c, "mis", **kw)
        films[label] = _frames(r, film, 4)
        names[label] = r.shade_instance()
        assert r.light_cluster_info().active == 0
        del r
    assert np.array_equal(films["never"].view(np.uint32), films["power"].view(np.uint32))
    assert np.array_equal(films["never_analytic"].view(np.uint32), films["clustered_analytic"].view(np.uint32))
    assert names["never"] == names["power"] == "k_shade_nee_mesh<true, false>"
    assert names["never_analytic"] == names["clustered_analytic"] == "k_shade_nee<true, false>"
    r, film = _renderer(c, "mis")
    clus = _frames(r, film, 4)
    assert r.shade_instance() == "k_shade_nee_clus<true, false>" and not np.array_equal(clus, films["never"])


# ---- 6. unbiased -----------------------------------------------------------------------------------------------------------------
def test_power_clustered_and_off_agree():
    W, H, S = 96, 64, 256
    c = dict(mr.case("bunny_light", W, H))
    X = {}
    for label, mode, sel in (("off", "off", None), ("power", "mis", "power"), ("clustered", "mis", "clustered")):
        for k, seed in enumerate((SEED, SEED + 500)):
            r, film = _renderer(c, mode, selection=sel, K=32, sif=64, seed=seed)
            r.ProgressiveRender(S)
            r.download()
            X[label, k] = film.accum.reshape(-1, 3).astype(np.float64).sum(1) / S
            del r
    _agree(X, W, pairs=(("power", "clustered"), ("clustered", "off"), ("power", "off")), label="bunny_light clusters")


# ---- 7. variance -----------------------------------------------------------------------------------------------------------------
def test_variance_ratio_agrees_with_the_replay(record_property):
    c = lcr.near_far()
    gp = lcr.ground_pixels(c)
    S, G = 64, 8
    r0, _ = _renderer(c, "nee", K=2)
    tables = lcr.read_tables(r0)
    del r0
    rp = mr.replay_case(c, "nee", samples=range(S), stability=False, pix=gp)
    rc = lcr.replay_case(c, "nee", tables, samples=range(S), stability=False, pix=gp)
    R_ref, se_ref, _ = lcr.variance_ratio(lcr.luminance(rp.value).reshape(S, len(gp)).T, lcr.luminance(rc.value).reshape(S, len(gp)).T, G)

    def moments(sel):
        """Per group: (A, Q) [n_ground] from the film statistics of S / G samples."""
        r, film = _renderer(c, "nee", selection=sel, K=2, sif=8)
        r.set_film_statistics(True)
        out = []
        for g in range(G):
            film.Clear()
            r.frame_index = g * (S // G)
            r.ProgressiveRender(S // G)
            a, q = r.film_statistics()
            out.append((a.reshape(-1)[gp].astype(np.float64), q.reshape(-1)[gp].astype(np.float64)))
        return out

    def var_sum(A, Q, n):
        return float(((Q - A * A / n) / (n - 1)).sum())
    mp, mc = moments("power"), moments("clustered")
    per = S // G
    rs = np.array([var_sum(*mc[g], per) / var_sum(*mp[g], per) for g in range(G)])
    tot = lambda m: var_sum(sum(a for a, _ in m), sum(q for _, q in m), S)   # noqa: E731
    R_gpu, se_gpu = tot(mc) / tot(mp), float(rs.std(ddof=1) / np.sqrt(G))
    rec = dict(R_gpu=round(R_gpu, 4), se_gpu=round(se_gpu, 4), R_ref=round(R_ref, 4), se_ref=round(se_ref, 4))
    record_property("light_cluster_variance", rec)
    print(rec, flush=True)
    assert R_ref + 4 * se_ref < 1
    assert abs(R_gpu - R_ref) <= 4 * np.sqrt(se_gpu ** 2 + se_ref ** 2), rec
