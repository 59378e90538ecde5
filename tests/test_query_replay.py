"""The reference side of the radiance-query tests alone (no GPU): tests/query_rays.py's rays, started through the walkers'
`start=`, make a yardstick one can believe before a kernel is involved.

  * The walker started from caller-supplied rays is OracleScene.trace: delivered radiance bit for bit and the segment count of
    EVERY ray, on every scene the oracle covers and every family, non-unit first directions and rays that start inside
    geometry included.  OracleScene.trace takes no PrtSampling, so under roulette and clamp (0, 2, 1.5) the walker is held
    to it on the rays roulette cannot touch (paths of at most two segments: the first roulette draw follows the second
    segment's scatter), where it must deliver min(L, 1.5) bit for bit; every other ray delivers at most the clamp (a
    roulette draw advances the state, so the rest of such a path is another path); and a film's own camera rays, handed in
    through `start=`, must give OracleScene.render's film under that PrtSampling bit for bit.
  * `start=None` is the pixel walker: the same camera rays through `start=` give the same records.
  * The undecidable share of every (case, family, mode) the GPU test runs is within lighting_replay.MAX_UNSTABLE = 0.005: a
    condition on the inputs (a family or a seed that broke it would be changed, never the cap or the stability rules).
  * Coverage, from the reference's own record: first hits > N / 8, light samples >= 1000, occluded shadow rays where the case
    has blockers, a path at the depth limit (on `resting` and `bunny_light` the ground plane is the only scatterer, so no ray
    whatever has a path of more than two segments: there the longest path is asserted to be exactly that); back-face first
    hits of `inside` on specular and CORNELL >= 50; first vertices of `gap` inside the sphere light's margin >= 20 and outside
    >= 1000; weighted emissions under MIS >= 20.
  * Wrong estimators are told apart on the ray clouds (lighting_replay.separated_share: more than 1 % of the stable rays move
    by more than 10 x their tolerance): pb_kept on specular (MIS), wb_no_pmf on DEFAULT (MIS), tmax_no_eps on penumbra (NEE),
    and wb_camera, the caller's own segment being weighted, on each of the three.

Measured (N = 4099 rays per family; share = undecidable samples / light samples (and misses, under an environment image)):

  case                   family  first hits  back-face  light samples  occluded  share (worse mode)  weighted (mis)  at depth limit
  penumbra               shell         3224        385           3210       859             0.00000             161              18
  penumbra               inside        1696         63           1764       353             0.00000              45              20
  penumbra               scaled        3224        385           3210       859             0.00000             161              18
  specular               shell         3560       1438           1591       734             0.00000             294              14
  specular               inside        2826        397           1503       563             0.00000             286             281
  DEFAULT_rr_clamp       shell         3224        138           2332       322             0.00000             406              41
  DEFAULT_rr_clamp       scaled        3224        138           2331       322             0.00000             405              37
  RANDOM_BALLS_SMALL     shell         3478         19           3628       298             0.00000              28              35
  CORNELL                inside        2615        753           3798        56             0.00053              48              37
  resting                gap           4099          0           4054         0             0.00197            3801               0   margin: 45 inside, 4054 outside
  placed_power           shell         3090        364           3049       300             0.00066             269              46
  placed_clustered       shell         3090        382           3012       557             0.00100             227              55
  bunny_light_power      shell         3134          1           2615      1308             0.00076             179               0
  bunny_light_clustered  shell         3098          0           2574      1221             0.00233             183               0
  env_DEFAULT_sun        shell         3326        149           2482      1012             0.00099            2131              57
  env_DEFAULT_sun        scaled        3326        149           2479      1006             0.00099            2128              54
  env_placed_mesh        shell         3111        425           3005       370             0.00080            2502              54
  env_blackrows          shell         3315        147           2396       350             0.00081            1786              54
  tex_A_mis_analytic     shell         3162        378           3007       152             0.00033             216             151
  tex_B_mis_mesh         shell         3496        370           3822       517             0.00026             265             289
  tex_B_nee_mesh_env     shell         3509        408           3872       546             0.00042            2852             302
  bunny                  inside        1982        116           2110       334             0.00047             102              99

Three samples per ray by ray index (samples 2, 3, 4):
  penumbra mis: light samples 9618, share 0.00000, rays stable in all three samples 4099
  penumbra nee: light samples 9618, share 0.00000, rays stable in all three samples 4099
  placed_clustered mis: light samples 9094, share 0.00011, rays stable in all three samples 4098
  placed_clustered nee: light samples 9094, share 0.00011, rays stable in all three samples 4098
  tex_B_nee_mesh_env mis: light samples 11549, share 0.00052, rays stable in all three samples 4090
  tex_B_nee_mesh_env nee: light samples 11549, share 0.00052, rays stable in all three samples 4090

Wrong estimators:
  pb_kept on specular (shell+inside, mis): separated share 0.0224
  wb_no_pmf on DEFAULT_rr_clamp (shell, mis): separated share 0.0990
  tmax_no_eps on penumbra (shell+inside, nee): separated share 0.1364
  wb_camera on specular (shell+inside, mis): separated share 0.2817
  wb_camera on DEFAULT_rr_clamp (shell, mis): separated share 0.2479
  wb_camera on penumbra (shell+inside, mis): separated share 0.0654"""
import functools

import numpy as np
import pytest

import lighting_replay as lr
import query_rays as qr
from parallelraytracing_amd.capi import PrtSampling
from util import orc

N = qr.N
ALL = qr.LIT + tuple((r["name"], f) for r in qr.CPU_ONLY for f in r["families"])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def tables(name):
    return qr.host_tables(qr.case(name)) if qr.row(name)["selection"] == "clustered" else None


@functools.lru_cache(maxsize=None)
def replayed(name, family, mode):
    return qr.replay(qr.case(name), qr.rays(name, family), mode, tables=tables(name))


def test_the_families_are_what_they_say():
    for name, family in ALL:
        o, d, st = qr.rays(name, family)
        assert o.shape == d.shape == (N, 3) and st.shape == (N,) and o.dtype == d.dtype == np.float32 and st.dtype == np.uint32
        assert N % 64 and N % 256
        l2 = (d.astype(np.float64) ** 2).sum(1)
        if family == "scaled":
            so, sd, sst = qr.rays(name, "shell")
            assert np.array_equal(o, so) and np.array_equal(st, sst)
            k = np.sqrt(l2)
            for s in set(qr.SCALES):
                assert (np.abs(k - s) < 1e-6 * s).sum() > N // 8, (name, s)
            assert (np.abs(l2 - 1.0) > 2.0 ** -20).sum() > N // 3
        else:
            assert np.all(np.abs(l2 - 1.0) < 2.0 ** -21), (name, family)     # unit as fp32 makes them: inside the lookup's band
    assert len(set(qr.family_seed(n, f) for n, f in ALL if f != "scaled")) == len([1 for n, f in ALL if f != "scaled"])


def test_scaled_sphere_directions_stay_clear_of_texel_edges():
    """The reference of the first-segment lookup test alone: on the lognormal 32 x 64 map at least 99 % of the 4099 directions,
    at each length, lie farther than EDGE from a texel edge in the float64 mapping of the float64-normalised direction."""
    import environment_replay as er
    env = er.EnvMap(er.named_map("lognormal"), 0.5)
    u = qr.sphere_directions()
    texels = set()
    for k in (0.125, 1.0, 3.7):
        d = (u * np.float32(k)).astype(np.float32).astype(np.float64)
        i, j, edge = er.lookup64(env, d / np.sqrt((d * d).sum(1))[:, None])
        assert (edge > er.EDGE).sum() >= 0.99 * N, k
        texels |= set(zip(i.tolist(), j.tolist()))
        # handed over as given, a short direction reaches only the rows around the horizon and a long one mostly the poles
        i0, _, _ = er.lookup64(env, d)
        assert k == 1.0 or (i0 != i).mean() > 0.8, k
    assert len(texels) > 0.7 * env.H * env.W        # the directions cover the map


# ---- the walker from caller-supplied rays is the oracle's trace -------------------------------------------------------------
ORACLE_ROWS = tuple((n, f) for n, f in ALL if not qr.row(n)["textured"] and qr.row(n)["selection"] == "power")


@pytest.mark.parametrize("name,family", ORACLE_ROWS)
def test_walker_from_caller_rays_equals_oracle_trace(name, family):
    c = qr.case(name)
    o, d, st = qr.rays(name, family)
    idx = np.arange(N)
    zeros = np.zeros(N, np.int64)
    walk = functools.partial(lr.walk, c["scene"], c["osc"], c["cam"], 1, 1, c["depth"], qr.SEED, idx, zeros, use_bvh=c["use_bvh"],
                             start=(o, d, st))
    verts, delivered, last, segs = walk(sampling=(0, 0, 0.0))
    assert np.array_equal(bits(verts[0]["o"]), bits(o)) and np.array_equal(bits(verts[0]["d"]), bits(d))    # as given
    assert np.array_equal(verts[0]["key"], st)
    L, seg, _ = qr.oracle_trace(c, o, d, st)
    bad = np.nonzero((bits(L) != bits(delivered)).any(1) | (seg != last + 1))[0]
    assert bad.size == 0, (name, family, bad[:8], L[bad[:2]], delivered[bad[:2]], seg[bad[:4]], last[bad[:4]] + 1)
    assert segs == int(seg.sum())
    # roulette and clamp: the oracle's trace has neither; what it still pins
    _, d_rr, last_rr, _ = walk(sampling=qr.RR_CLAMP)
    short = seg <= 2
    assert short.sum() > N // 8
    clamped = np.minimum(L, np.float32(qr.RR_CLAMP[2]))
    assert np.array_equal(bits(d_rr[short]), bits(clamped[short])) and np.array_equal(last_rr[short], last[short])
    assert np.all(d_rr <= np.float32(qr.RR_CLAMP[2]))
    print(f"\n{name} {family}: segments {segs}, at most two segments {int(short.sum())}, moved by roulette {int((last_rr != last).sum())}")


@pytest.mark.parametrize("name", ["DEFAULT", "specular"])
def test_camera_rays_through_start_are_the_pixel_walker_and_the_oracles_film(name):
    W, H = 24, 18
    c = lr.case(name, W, H)
    osc = orc.OracleScene(c["scene"].desc())
    pix = np.arange(W * H)
    samples = (2, 3)
    apix = np.tile(pix, len(samples))
    asamp = np.repeat(samples, len(pix))
    o, d = orc.camera_rays(c["cam"].desc(), (pix % W).astype(np.float32) + np.float32(0.5), (pix // W).astype(np.float32) + np.float32(0.5))
    for smp in ((0, 0, 0.0), qr.RR_CLAMP):
        walk = functools.partial(lr.walk, c["scene"], osc, c["cam"], W, H, c["depth"], qr.SEED, apix, asamp, smp, use_bvh=c["use_bvh"])
        _, got, last, segs = walk(start=(o, d))
        _, want, wlast, wsegs = walk()
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(last, wlast) and segs == wsegs
        total = 0
        for s in samples:
            a, w, rays = osc.render(c["cam"].desc(), W, H, spp=1, first_sample=s, max_depth=c["depth"], seed=qr.SEED, iterative=True,
                                    use_bvh=c["use_bvh"], n_threads=lr.n_threads_default(), sampling=PrtSampling(*smp))
            total += rays
            assert np.array_equal(bits(a.reshape(-1, 3)), bits(got[asamp == s])), (name, smp, s)
        assert total == segs
        if smp[1]:
            assert (got <= np.float32(smp[2])).all() and len(np.unique(got, axis=0)) > 8


def test_states_need_one_sample():
    c = qr.case("penumbra")
    o, d, st = qr.rays("penumbra", "shell")
    with pytest.raises(AssertionError):
        lr.walk(c["scene"], c["osc"], c["cam"], 1, 1, 2, qr.SEED, np.tile(np.arange(4), 2), np.repeat((0, 1), 4), start=(o, d, st))


# ---- the undecidable share and the coverage of everything the GPU test runs -----------------------------------------------
@pytest.mark.parametrize("name,family", ALL)
def test_unstable_share_and_coverage(record_property, name, family):
    c = qr.case(name)
    rw = c["row"]
    o, d, st = qr.rays(name, family)
    first = c["osc"].closest_hit(o, d, use_bvh=c["use_bvh"], n_threads=lr.n_threads_default())
    hit = first["prim"] >= 0
    back = hit & (first["front_face"] == 0)
    assert hit.sum() > N // 8, (name, family, int(hit.sum()))
    for mode in qr.MODES:
        r = replayed(name, family, mode)
        share = qr.unstable_share(c, r)
        rec = dict(case=name, family=family, mode=mode, first_hits=int(hit.sum()), back_face=int(back.sum()), light_samples=r.n_light_samples,
                   shadow_rays=r.shadow_rays, occluded=r.shadow_occluded, unstable=r.n_unstable, indifferent=r.n_indifferent,
                   share=round(share, 5), unstable_rays=r.n_unstable_samples, weighted=r.n_weighted,
                   depth_limit=int((r.last == c["depth"] - 1).sum()))
        if family == "gap":
            g = first["prim"] == 0
            D = np.linalg.norm(first["position"][g].astype(np.float64) - r.lights.c[0], axis=1)
            inside = D <= r.lights.R[0] * (1.0 + lr.SPHERE_MARGIN)
            rec.update(inside_margin=int(inside.sum()), outside_margin=int((~inside).sum()))
            assert rec["inside_margin"] >= 20 and rec["outside_margin"] >= 1000, rec
        print(rec, flush=True)
        record_property("query_replay", rec)
        assert share <= lr.MAX_UNSTABLE, rec
        assert r.stable.sum() >= 0.995 * N, rec
        assert r.n_light_samples >= 1000, rec
        assert r.shadow_occluded > 0 or not rw["blockers"], rec
        if rw["longest"] is None:
            assert rec["depth_limit"] >= 1, rec
        else:       # the scene's only scatterer is the ground plane: no ray at all has a path of more than two segments
            assert rw["longest"] < c["depth"] and int(r.last.max()) + 1 == rw["longest"], rec
        assert mode != "mis" or r.n_weighted >= 20, rec
        if family == "inside" and name in ("specular", "CORNELL"):
            assert rec["back_face"] >= 50, rec
        if name.startswith("env_") or name.endswith("_env"):
            assert 0.3 * r.n_light_samples < r.n_env_samples < 0.7 * r.n_light_samples, rec


@pytest.mark.parametrize("name", qr.MULTI_SAMPLE)
def test_unstable_share_of_the_multi_sample_calls(name):
    """Seeds by ray index: samples (2, 3, 4) of every ray, as the GPU test's samples = 3, first_sample = 2 calls run them."""
    c = qr.case(name)
    o, d, _ = qr.rays(name, "shell")
    for mode in qr.MODES:
        r = qr.replay(c, (o, d), mode, samples=(2, 3, 4), tables=tables(name))
        assert np.array_equal(r.samp, np.repeat((2, 3, 4), N)) and np.array_equal(r.pix, np.tile(np.arange(N), 3))
        stable = r.stable.reshape(3, N).all(0)
        print(f"\n{name} {mode}: light samples {r.n_light_samples}, share {qr.unstable_share(c, r):.5f}, rays stable in all three samples "
              f"{int(stable.sum())}")
        assert qr.unstable_share(c, r) <= lr.MAX_UNSTABLE and stable.sum() >= 0.995 * N


# ---- wrong estimators are told apart on the ray clouds -----------------------------------------------------------------------
SEPARATES = (("pb_kept", "specular", "mis"), ("wb_no_pmf", "DEFAULT_rr_clamp", "mis"), ("tmax_no_eps", "penumbra", "nee"),
             ("wb_camera", "specular", "mis"), ("wb_camera", "DEFAULT_rr_clamp", "mis"), ("wb_camera", "penumbra", "mis"))


@pytest.mark.parametrize("wrong,name,mode", SEPARATES)
def test_wrong_estimators_are_told_apart_on_the_clouds(wrong, name, mode):
    c = qr.case(name)
    fams = [f for f in ("shell", "inside") if f in c["row"]["families"]]
    o, d, st = (np.concatenate([qr.rays(name, f)[k] for f in fams]) for k in range(3))
    right = qr.replay(c, (o, d, st), mode)
    other = qr.replay(c, (o, d, st), mode, wrong=wrong, stability=False)
    share = lr.separated_share(right, other, 10.0)
    print(f"\n{wrong} on {name} ({'+'.join(fams)}, {mode}): separated share {share:.4f}")
    assert share > 0.01, (wrong, name, mode, share)
