"""The radiance queries (include/prt.h "Radiance query": prt_radiance, prt_radiance_lit) over rays the caller chose, held to the
float64 per-path replays and to the oracle on one MI355X.  Rays, cases and the comparison: tests/query_rays.py; the reference
side alone (caps, coverage, wrong estimators): tests/test_query_replay.py.  Every family is 4099 rays: 17 blocks of the step
kernel, so both stream compactions and the slot-keyed shadow records cross block boundaries.

a. The lit query, value by value.  Per row of query_rays.ROWS, family and mode (mis, nee), with rng_state given: every stable
   ray within the replay's own tolerance (no exception), compared >= 0.995 N, shadow rays and occluded shadow rays within the
   number of undecidable samples of the replay's, segments equal to the replay's per ray, rng_state and segments equal to the
   unlit query's, and the unlit query equal to OracleScene.trace bit for bit (final state included) where the oracle covers
   the scene, elsewhere to the mode "off" replay's fp32 walker bit for bit (misses within EDGE of a texel edge left out).
b. Seeds by ray index: samples = 3, first_sample = 2, no states (3 x 4099 paths in one launch, 49 blocks) against the three
   replay values added in ascending sample order, tolerance summed plus 4 U sum |value|; the same under radiance_chunk = 1.
c. The unlit query where the oracle is blind (textures, environment image) against the mode "off" replays: bit for bit on
   every ray whose miss is not within EDGE of a texel edge, segments on all rays.
d. Non-unit directions against the oracle: the `scaled` family on CORNELL, DEFAULT+, MATERIAL_TEST and COPIES at max_depth 1,
   2 and 5: sum, segments and final rng_state bit for bit, no exclusions.
e. Non-unit directions under an environment image: a miss of the caller's own segment reads the texel of the normalised
   direction (the first-segment lookup rule).  An empty scene under the lognormal 32 x 64 map, 4099 unit directions each
   queried as k d, k in (0.125, 1, 3.7), lit and unlit, both modes: env.rgb at lookup64 of the float64-normalised direction,
   bit for bit, on the directions farther than EDGE from a texel edge (at least 99 % of them); at k = 1 every ray is bit for
   bit prt_environment_eval of the same direction, as before the rule.  Then DEFAULT_sun with the `scaled` family against
   the replay: unlit here, lit in both modes as a row of (a).

Measured on an MI355X, 4099 rays per row ("x3": 3 samples per ray, a ray compared only if all three are stable).  No stable
ray lies outside its tolerance in any row, and the query's shadow-ray and occluded counts equal the replay's exactly in every
row (the slack of unstable + indifferent samples is not used).  On CORNELL most light samples are indifferent (grazing samples
below the absolute tolerance): the counts say little there, the per-ray values carry the case.

  case                   family    mode  compared  left out  err / tol  shadow rays  occluded  indifferent
  penumbra               shell     mis       4099         0     0.0430         2883       859            0
  penumbra               shell     nee       4099         0     0.0441         2883       859            0
  penumbra               inside    mis       4099         0     0.0400         1624       353            0
  penumbra               inside    nee       4099         0     0.0455         1624       353            0
  penumbra               scaled    mis       4099         0     0.0430         2883       859            0
  penumbra               scaled    nee       4099         0     0.0441         2883       859            0
  specular               shell     mis       4099         0     0.0335         1591       734            0
  specular               shell     nee       4099         0     0.0456         1591       734            0
  specular               inside    mis       4099         0     0.0351         1503       563            0
  specular               inside    nee       4099         0     0.0397         1503       563            0
  DEFAULT_rr_clamp       shell     mis       4099         0     0.0407         2177       322            0
  DEFAULT_rr_clamp       shell     nee       4099         0     0.0426         2177       322            0
  DEFAULT_rr_clamp       scaled    mis       4099         0     0.0413         2176       322            0
  DEFAULT_rr_clamp       scaled    nee       4099         0     0.0405         2176       322            0
  RANDOM_BALLS_SMALL     shell     mis       4099         0     0.0274         3536       298            0
  RANDOM_BALLS_SMALL     shell     nee       4099         0     0.0265         3536       298            0
  CORNELL                inside    mis       4097         2     0.0397         2687        56         2118
  CORNELL                inside    nee       4097         2     0.0368         2687        56         2118
  resting                gap       mis       4095         4     0.1712         4054         0            0
  resting                gap       nee       4095         4     0.1776         4054         0            0
  placed_power           shell     mis       4097         2     0.0458         2746       300            0
  placed_power           shell     nee       4097         2     0.0485         2746       300            0
  placed_clustered       shell     mis       4096         3     0.0434         2735       557            0
  placed_clustered       shell     nee       4096         3     0.0503         2735       557            0
  bunny_light_power      shell     mis       4097         2     0.0344         2615      1308            0
  bunny_light_power      shell     nee       4097         2     0.0393         2615      1308            0
  bunny_light_clustered  shell     mis       4093         6     0.0375         2574      1221            0
  bunny_light_clustered  shell     nee       4093         6     0.0492         2574      1221            0
  env_DEFAULT_sun        shell     mis       4094         5     0.0352         2334      1012            1
  env_DEFAULT_sun        shell     nee       4094         5     0.0377         2334      1012            1
  env_DEFAULT_sun        scaled    mis       4094         5     0.0352         2330      1006            1
  env_DEFAULT_sun        scaled    nee       4094         5     0.0377         2330      1006            1
  env_placed_mesh        shell     mis       4094         5     0.1708         2720       370            0
  env_placed_mesh        shell     nee       4094         5     0.1990         2720       370            0
  env_blackrows          shell     mis       4095         4     0.0338         1757       350            0
  env_blackrows          shell     nee       4095         4     0.0994         1757       350            0
  tex_A_mis_analytic     shell     mis       4098         1     0.0392         2704       152            1
  tex_A_mis_analytic     shell     nee       4098         1     0.0386         2704       152            1
  tex_B_mis_mesh         shell     mis       4098         1     0.0454         3248       517            1
  tex_B_mis_mesh         shell     nee       4098         1     0.0427         3248       517            1
  tex_B_nee_mesh_env     shell     mis       4096         3     0.2023         3305       546            1
  tex_B_nee_mesh_env     shell     nee       4096         3     0.2294         3305       546            1
  penumbra               shell x3  mis       4099         0     0.1653         8667      2614            0
  penumbra               shell x3  nee       4099         0     0.1653         8667      2614            0
  placed_clustered       shell x3  mis       4098         1     0.1347         8238      1771            2
  placed_clustered       shell x3  nee       4098         1     0.1347         8238      1771            2
  tex_B_nee_mesh_env     shell x3  mis       4090         9     0.2123         9865      1683            1
  tex_B_nee_mesh_env     shell x3  nee       4090         9     0.2282         9865      1683            1

(c) tex_B_nee_mesh_env: 4096 compared, 3 left out, 3284 misses; env_DEFAULT_sun: 4095 compared, 4 left out, 2588 misses.
(e) before the first-segment lookup rule 3739 of the 4099 directions read a wrong texel at k = 0.125 and 3976 at k = 3.7, in
every mode and through both entry points (0 at k = 1), and 159 rays of DEFAULT_sun's `scaled` family differed; with it, none."""
import numpy as np
import pytest

import environment_replay as er
import light_cluster_replay as lcr
import query_rays as qr
from util import orc, prt

pytestmark = pytest.mark.gpu

F = np.float32
N = qr.N


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def renderer(c):
    """A context for case c: sources, selection, environment image and sampling as the row says; lighting still off."""
    rw = c["row"]
    r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=qr.SEED)
    if rw["sources"] == "all":
        r.set_light_sources("all")
    if rw["selection"] == "clustered":
        r.set_light_selection("clustered", qr.CLUSTERS)
    if c["env"] is not None:
        r.set_environment(c["env"].rgb, c["env"].light_share)
    r.Init(prt.Film(9, 7), c["scene"], c["cam"])
    if any(c["sampling"]):
        assert tuple(c["sampling"]) == qr.RR_CLAMP
        r.set_sampling(rr_depth=qr.RR_CLAMP[1], clamp=qr.RR_CLAMP[2])
    tables = None
    if rw["selection"] == "clustered":
        assert r.light_cluster_info().active == 1
        tables = lcr.read_tables(r)
    if rw["textured"]:
        assert r.texture_info().n_textured_materials > 0
    return r, tables


# ---- a. the lit query, value by value ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,family", qr.LIT)
def test_lit_query_matches_the_float64_replay(record_property, name, family):
    c = qr.case(name)
    o, d, st = qr.rays(name, family)
    r, tables = renderer(c)
    unlit = r.radiance(o, d, rng_state=st, return_info=True)[1]
    if c["row"]["oracle"]:
        L, seg, fin = qr.oracle_trace(c, o, d, st)
        bad = np.nonzero((bits(unlit["sum"]) != bits(L)).any(1) | (unlit["segments"] != seg) | (unlit["rng_state"] != fin))[0]
        assert bad.size == 0, (name, family, bad[:8], unlit["sum"][bad[:2]], L[bad[:2]])
    else:       # roulette and clamp, textures, an environment image: the mode "off" replay's fp32 walker, bit for bit
        off = qr.replay(c, (o, d, st), "off")
        keep = ~getattr(off, "miss_unstable", np.zeros(N, bool))
        bad = np.nonzero(keep & (bits(unlit["sum"]) != bits(off.delivered)).any(1))[0]
        assert bad.size == 0 and keep.sum() >= 0.995 * N, (name, family, bad[:8], unlit["sum"][bad[:2]], off.delivered[bad[:2]])
        assert np.array_equal(unlit["segments"], qr.segments(off))
    for mode in qr.MODES:
        r.set_lighting(mode)
        info = r.radiance(o, d, rng_state=st, return_info=True, lighting=True)[1]
        rep = qr.replay(c, (o, d, st), mode, tables=tables)
        if c["env"] is not None:
            assert r.environment_info().t_env == int(rep.t_env) > 0
        print(f"\n{name} {family} {mode}: ", end="")
        rec = qr.check_lit(c, rep, info["sum"], info)
        rec.update(case=name, family=family, mode=mode)
        record_property("query_replay", rec)
        assert info["shadow_rays"] > 0 and rep.n_light_samples >= 1000
        assert np.array_equal(info["segments"], unlit["segments"]) and np.array_equal(info["rng_state"], unlit["rng_state"]), (name, mode)
    assert np.array_equal(st, qr.rays(name, family)[2])        # the caller's states are not advanced in place


# ---- b. seeds by ray index, several samples ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qr.MULTI_SAMPLE)
def test_samples_by_ray_index_add_up_to_the_replays(record_property, name):
    c = qr.case(name)
    o, d, _ = qr.rays(name, "shell")
    r, tables = renderer(c)
    for mode in qr.MODES:
        r.set_lighting(mode)
        r.set_param("radiance_chunk", 0)
        info = r.radiance(o, d, samples=3, first_sample=2, return_info=True, lighting=True)[1]
        rep = qr.replay(c, (o, d), mode, samples=(2, 3, 4), tables=tables)
        print(f"\n{name} shell {mode} x3: ", end="")
        rec = qr.check_lit(c, rep, info["sum"], info, n_samples=3)
        rec.update(case=name, family="shell x3", mode=mode)
        record_property("query_replay", rec)
        r.set_param("radiance_chunk", 1)
        one = r.radiance(o, d, samples=3, first_sample=2, return_info=True, lighting=True)[1]
        qr.check_lit(c, rep, one["sum"], one, n_samples=3)
        assert np.array_equal(bits(one["sum"]), bits(info["sum"])) and np.array_equal(one["segments"], info["segments"])
        assert (one["shadow_rays"], one["shadow_occluded"]) == (info["shadow_rays"], info["shadow_occluded"])
    r.set_param("radiance_chunk", 0)


# ---- c. the unlit query where the oracle is blind ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", qr.UNLIT_BLIND)
def test_unlit_query_matches_the_off_replay(name):
    c = qr.case(name)
    o, d, st = qr.rays(name, "shell")
    r, _ = renderer(c)
    rep = qr.replay(c, (o, d, st), "off")
    assert rep.shadow_rays == 0 and rep.n_light_samples == 0
    keep = ~rep.miss_unstable
    assert keep.sum() >= 0.995 * N and rep.n_misses > N // 8
    for lighting in (False, True):                  # the unlit entry point, and the lit one with the mode off
        info = r.radiance(o, d, rng_state=st, return_info=True, lighting=lighting)[1]
        err = np.abs(info["sum"].astype(np.float64) - rep.value)
        bad = np.nonzero(keep & ((err > rep.tol).any(1) | (bits(info["sum"]) != bits(rep.delivered)).any(1)))[0]
        assert bad.size == 0, (name, lighting, bad[:8], info["sum"][bad[:3]], rep.delivered[bad[:3]])
        assert np.array_equal(info["segments"], qr.segments(rep)), name
    print(f"\n{name} off: compared {int(keep.sum())}, left out {int((~keep).sum())}, misses {rep.n_misses}, segments {rep.segments}")


# ---- d. non-unit directions against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qr.SCALED_ORACLE)
def test_scaled_directions_equal_the_oracle_bit_for_bit(name):
    scene = qr.make_scene(name)
    osc = orc.OracleScene(scene.desc())
    o, d, st = qr.scaled_oracle_rays(name)
    l2 = (d.astype(np.float64) ** 2).sum(1)
    assert (l2 < 0.02).sum() > N // 8 and (l2 > 13.0).sum() > N // 8 and (np.abs(l2 - 1.0) < 1e-6).sum() > N // 3
    assert (osc.closest_hit(o, d, use_bvh=False)["prim"] >= 0).sum() > N // 8
    r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=qr.SEED)
    r.Init(prt.Film(9, 7), scene, prt.Camera(width=9, height=7))
    for depth in (1, 2, 5):
        L, seg, fin = np.empty((N, 3), F), np.empty(N, np.uint32), np.empty(N, np.uint32)
        for i in range(N):
            L[i], seg[i], fin[i] = osc.trace(o[i], d[i], depth, int(st[i]), iterative=True, use_bvh=False)
        info = r.radiance(o, d, rng_state=st, max_depth=depth, return_info=True)[1]
        bad = np.nonzero((bits(info["sum"]) != bits(L)).any(1) | (info["segments"] != seg) | (info["rng_state"] != fin))[0]
        assert bad.size == 0, (name, depth, bad[:8], info["sum"][bad[:2]], L[bad[:2]], info["segments"][bad[:4]], seg[bad[:4]])
        if depth == 5:
            assert (seg == 5).any() and (seg == 1).any()


# ---- e. non-unit directions under an environment image -----------------------------------------------------------------------
def test_first_segment_miss_reads_the_texel_of_the_normalised_direction(record_property):
    env = er.EnvMap(er.named_map("lognormal"), 0.5)
    assert (env.H, env.W) == (32, 64)
    u = qr.sphere_directions()
    o = np.zeros((N, 3), F)
    r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=qr.SEED)
    r.set_environment(env.rgb, env.light_share)
    r.Init(prt.Film(9, 7), prt.Scene(preset=None), prt.Camera(width=9, height=7))
    unit = r.environment_eval(u)["rgb"]
    wrong = {}
    for k in (0.125, 1.0, 3.7):
        d = (u * F(k)).astype(F)
        d64 = d.astype(np.float64)
        i, j, edge = er.lookup64(env, d64 / np.sqrt((d64 * d64).sum(1))[:, None])
        keep = edge > er.EDGE
        assert keep.sum() >= 0.99 * N                       # the reference alone
        want = env.rgb[i, j]
        for mode in ("off",) + qr.MODES:
            r.set_lighting(mode)
            for lighting in (False, True):
                info = r.radiance(o, d, return_info=True, lighting=lighting)[1]
                bad = keep & (bits(info["sum"]) != bits(want)).any(1)
                wrong[(k, mode, lighting)] = int(bad.sum())
                assert (info["segments"] == 1).all()
                if k == 1.0:                                # unit callers see what they saw: the render's own lookup
                    assert np.array_equal(bits(info["sum"]), bits(unit)), (mode, lighting)
    print(f"\nwrong texels of {N} (k, mode, lit entry point): {wrong}")
    record_property("first_segment_lookup", {str(k): v for k, v in wrong.items()})
    assert not any(wrong.values()), wrong


def test_first_segment_miss_of_scaled_rays_follows_the_off_replay():
    """DEFAULT_sun, the `scaled` family, lighting off (lit in both modes: test_lit_query_matches_the_float64_replay's row)."""
    name = "env_DEFAULT_sun"
    c = qr.case(name)
    o, d, st = qr.rays(name, "scaled")
    r, _ = renderer(c)
    off = qr.replay(c, (o, d, st), "off")
    first_miss = c["osc"].closest_hit(o, d, use_bvh=c["use_bvh"])["prim"] < 0
    l2 = (d.astype(np.float64) ** 2).sum(1)
    assert (first_miss & (np.abs(l2 - 1.0) > 0.5)).sum() > 100          # scaled rays that miss on their own segment
    keep = ~off.miss_unstable
    assert keep.sum() >= 0.995 * N
    for lighting in (False, True):
        info = r.radiance(o, d, rng_state=st, return_info=True, lighting=lighting)[1]
        bad = np.nonzero(keep & (bits(info["sum"]) != bits(off.delivered)).any(1))[0]
        assert bad.size == 0, (lighting, bad[:8], info["sum"][bad[:3]], off.delivered[bad[:3]])
        assert np.array_equal(info["segments"], qr.segments(off))
