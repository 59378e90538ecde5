"""Every sample of frames lit by an environment image against the float64 replay (tests/environment_replay.py) on one MI355X.

Per case and mode (mis, nee): Init, set_environment, set_lighting, then per sample index s (0, 1, 2, 5): film Clear,
frame_index = s, ProgressiveRender(1), download.  160 x 120, depth 5.  Every stable pixel sample must lie within the
tolerance lighting_replay.py defines (ABS_TOL, DIR_ULPS, TMAX_REL taken unchanged; sin(theta) of a sampled direction in the
place of a light's cosine, see environment_replay.py), the share of undecidable samples (the existing rules plus misses
within 2^-12 texel of a texel edge) must stay within MAX_UNSTABLE = 0.005, the shadow-ray and occluded counts must match the
replay's to within the number of undecidable samples, light_info() must carry the factor (2^32 - T_e) / 2^32 and
sample_light() must agree per vertex (light id, direction, pdfs, both weights).

Cases (environment_replay.case): bunny_env (the sun map alone on ground + bunny: T_e = 2^32), DEFAULT_sun (the sun map plus
the preset's quad and sphere lights), placed_mesh (placed copies, one an emitter, with the MESH bit set: the threshold rule),
blackrows (black first and last rows, black texels at both ends of a row), share0 / share1 (light_share 0 and 1; the others
run at 0.5).  One case also runs as a 3-rank group on the one GPU and with 64 samples in flight, and a 4-sample call equals
the fp32 sum of four one-sample frames.

Figures, measured on an MI355X (76,800 pixel samples per case and mode; no stable sample outside its tolerance anywhere; the
shadow-ray and occluded counts equal the replay's exactly in every row):

  case         mode  compared  left out  worst err / tol  shadow rays  occluded  environment samples
  bunny_env    mis     76,746        54           0.1149       52,248       721               53,780
  bunny_env    nee     76,746        54           0.2309       52,248       721               53,780
  DEFAULT_sun  mis     76,754        46           0.1558       55,661    20,471               28,858
  DEFAULT_sun  nee     76,754        46           0.1542       55,661    20,471               28,858
  placed_mesh  mis     76,751        49           0.1667       49,957     2,275               25,995
  placed_mesh  nee     76,751        49           0.1949       49,957     2,275               25,995
  blackrows    mis     76,737        63           0.1488       42,015     8,260               28,858
  blackrows    nee     76,737        63           0.1588       42,015     8,260               28,858
  share0       mis     76,752        48           0.2047       55,259     6,276                    0
  share0       nee     76,752        48           0.1936       55,259     6,276                    0
  share1       mis     76,756        44           0.1196       56,098    34,620               57,536
  share1       nee     76,756        44           0.2307       56,098    34,620               57,536

The replay side alone (CPU): per case 51,680 to 57,536 light samples, 58,336 to 76,432 misses of which 43 to 52 within the edge
margin, undecidable share 0.04 to 0.05 % (cap 0.5 %), 99.92 to 99.94 % of the pixel samples stable."""
import numpy as np
import pytest

import environment_replay as er
import lighting_replay as lr
import mesh_light_replay as mr
from util import orc, prt

pytestmark = pytest.mark.gpu


def _renderer(c, mode, sif=16, group=False):
    film = prt.Film(c["W"], c["H"])
    if group:
        r = prt.HipWavefrontGroupRenderer([0, 0, 0], max_depth=c["depth"], seed=lr.SEED)
    else:
        r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=lr.SEED)
    if c["sources"] == "all":
        r.set_light_sources("all")
    r.set_environment(er.named_map(c["env"]), c["light_share"])     # before the scene: it stays across Init
    r.Init(film, c["scene"], c["cam"])
    r.set_samples_in_flight(sif)
    r.set_lighting(mode)
    return r, film


@pytest.mark.parametrize("name", er.CASES)
def test_every_sample_matches_the_float64_replay(record_property, name):
    c = er.case(name)
    osc = orc.OracleScene(c["scene"].desc())
    for mode in ("mis", "nee"):
        rep = er.replay_case(c, mode, osc=osc)
        r, film = _renderer(c, mode)
        info = r.environment_info()
        assert info.t_env == int(rep.t_env)
        r.reset_stats()
        frames = lr.render_samples(r, film, lr.SAMPLES)
        r.synchronize()
        rec = er.check_against_gpu(rep, frames, r.light_stats())
        rec.update(case=name, mode=mode)
        record_property("environment_replay", rec)
        assert rec["compared"] >= 0.995 * len(rep.pix)
        prim, pmf = r.light_info()
        assert np.array_equal(np.asarray(prim, np.int64), rep.lights.prim)
        np.testing.assert_allclose(np.asarray(pmf, np.float64), rep.lights.pmf, rtol=1e-6, atol=0)
        if name in ("bunny_env", "share1"):
            assert rep.n_env_samples == rep.n_light_samples > 10000
        if name == "share0":
            assert rep.n_env_samples == 0 and rep.n_light_samples > 10000
        if name in ("DEFAULT_sun", "placed_mesh", "blackrows"):
            assert 0.3 * rep.n_light_samples < rep.n_env_samples < 0.7 * rep.n_light_samples
        del r


@pytest.mark.parametrize("name", ["DEFAULT_sun", "placed_mesh", "blackrows"])
def test_sample_light_matches_per_vertex(name):
    c = er.case(name)
    env = er.case_env(c)
    ls = mr.MeshLightSet(c["scene"], c["sources"])
    te = env.t_env(ls.n)
    ls.pmf = ls.pmf * ((er.TWO32 - te) / er.TWO32)
    rng = np.random.default_rng(5)
    n = 20000
    o = np.column_stack([rng.uniform(-8, 8, n), np.full(n, 6.0), rng.uniform(-8, 8, n)]).astype(np.float32)
    d = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (n, 1))
    for mode in ("mis", "nee"):
        r, _ = _renderer(c, mode)
        hits = r.closest_hit(o, d)
        lam = np.array([m.type for m in c["scene"].materials])[hits["material_id"]] == prt.capi.MAT_LAMBERTIAN
        lam &= hits["prim"] >= 0
        assert lam.sum() > 0.5 * n
        keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        out = r.sample_light(d, hits, keys)
        x = hits["position"].astype(np.float64)
        nrm = hits["normal"].astype(np.float64)
        to_env = er.env_selected(keys, te) & lam
        s = er.env_terms(env, te, nrm, keys, mode)
        ok = to_env & s["valid"] & (s["cos_l"] >= er.COS_MIN)
        assert ok.sum() > 0.2 * n
        assert np.all(out["light"][to_env & s["valid"]] == er.LIGHT_ENVIRONMENT)
        assert np.all(out["light"][to_env & ~s["valid"]] == 0xFFFFFFFF)
        assert np.all(out["light"][lam & ~to_env] != er.LIGHT_ENVIRONMENT)
        assert np.all(np.isinf(out["tmax"][ok]))
        np.testing.assert_allclose(out["dir"][ok], s["w"][ok], atol=2e-6)
        c_ = 8.0 * er.U / np.maximum(s["cos_l"], er.COS_MIN)

        def close(got, want, rtol, atol=0.0, sel=ok):
            err = np.abs(got[sel].astype(np.float64) - want[sel])
            lim = atol + (rtol + c_[sel]) * np.abs(want[sel])
            assert np.all(err <= lim), float((err / np.maximum(lim, 1e-300)).max())

        close(out["pdf_light"], s["pdf_l"], 1e-5)
        close(out["pdf_bsdf"], s["pb"], 1e-5, atol=1e-6)
        close(out["w_light"], s["wl"], 1e-4, atol=1e-6)
        # the weight of a miss along the sampled direction: the render's own lookup of fl32(w) (stable directions)
        w32 = out["dir"]
        i, j, edge = er.lookup64(env, w32)
        wb, sin_t, _ = er.miss_weight(env, te, w32, i, j, s["pb"], mode)
        st = ok & (edge > er.EDGE) & (s["pb"] > 0)
        close(out["w_bsdf"], wb, 1e-4, atol=1e-6, sel=st)
        # the other lights' samples carry the factor in pdf_light
        oth = lam & ~to_env
        so = mr.sample_lights(ls, x, nrm, keys, mode)
        ko = oth & so["valid"] & ~so["sel_band"] & (so["cos_l"] >= er.COS_MIN) & (so["margin_band"] > 1e-3)
        assert ko.sum() > 0.1 * n
        err = np.abs(out["pdf_light"][ko] - so["pdf_l"][ko])
        assert np.all(err <= (1e-5 + 8.0 * er.U / so["cos_l"][ko]) * so["pdf_l"][ko])
        del r


@pytest.mark.parametrize("route", ["group3", "sif64"])
def test_replay_holds_on_other_routes(route):
    c = er.case("DEFAULT_sun")
    rep = er.replay_case(c, "mis")
    if route == "group3":
        g, film = _renderer(c, "mis", group=True)
        frames = lr.render_samples(g, film, lr.SAMPLES, clear=g.Clear)
        er.check_against_gpu(rep, frames, g.light_stats())
    else:
        r, film = _renderer(c, "mis", sif=64)
        r.reset_stats()
        frames = lr.render_samples(r, film, lr.SAMPLES)
        er.check_against_gpu(rep, frames, r.light_stats())


def test_samples_add_up_in_sample_order():
    """The film of one 4-sample call is the fp32 sum, in sample order, of the four one-sample frames the replay pins."""
    c = er.case("DEFAULT_sun")
    r, film = _renderer(c, "mis")
    frames = lr.render_samples(r, film, range(4))
    film.Clear()
    r.frame_index = 0
    r.ProgressiveRender(4)
    r.download()
    acc = np.zeros_like(film.accum)
    for s in range(4):
        acc += frames[s]
    assert np.array_equal(acc.view(np.uint32), film.accum.view(np.uint32))
