"""The bake's statistics and block-adaptive sampling on the GPU (include/prt.h "Bake statistics and adaptive sampling";
bake_irradiance_adaptive, bake_block_select).

1. Select: bake_block_select equals the replay (tests/bake_adaptive_replay.py) exactly on synthetic moments built to hit
   every branch, on maps smaller than a block, with partial blocks, exact, and with several compaction strides.
2. The loop: count, sums, moments, mean, coverage and info equal the replay's loop over per-sample values rebuilt from the
   public pieces (bake_rays, bake_light_samples, occluded, radiance), bit for bit, in every chunking.
3. The headline property: the texels that end with count n hold bake_irradiance(samples=n) there, bit for bit.
4. A mix of counts is really produced on a scene with umbra, penumbra and open light.
5. Degenerate ends: a constant sky stops at min_spp; max_spp == min_spp is the uniform bake; a tiny threshold caps everything.
6. The gutter fill acts on the mean alone.
7. Nothing else moves: film, statistics, instance names, the next render and a plain bake; no allocation in a second call.
8. The device form equals the host form; the workspace regrows from a small map to a larger one and back."""
import functools

import numpy as np
import pytest

import bake_adaptive_replay as ar
import bake_replay as br
from util import prt
from test_gpu_bake import bits, renderer, scene_of
from test_gpu_bake_light import configure, target_scene

pytestmark = pytest.mark.gpu

F = np.float32


# ---- 1. select on synthetic moments ---------------------------------------------------------------------------------------
def _synthetic(H, W, coverage, seed):
    """Moments of 8 samples per texel, most of them converged at threshold 0.1, with every branch of the rule planted"""
    rng = np.random.default_rng(seed)
    n = H * W
    count = np.full(n, 8, F)
    base = rng.uniform(0.2, 2.0, n).astype(F)
    A = (base * F(8)).astype(F)
    Q = (base * base * F(8)).astype(F)                  # V ~ 0: converged
    blk = ar.block_of(H, W).ravel()
    cov = (np.asarray(coverage) == 1).ravel()
    noisy = rng.random(n) < 0.02                        # a few unconverged texels, covered or not
    Q[noisy] = (Q[noisy] * F(3)).astype(F)
    count[rng.random(n) < 0.01] = 1                     # count < 2
    count[rng.random(n) < 0.005] = 0
    nan_at = np.nonzero(rng.random(n) < 0.01)[0]
    A[nan_at] = np.nan                                  # NaN moments with count >= 2: converged by the rule's comparisons
    for k, v in enumerate((0.1, 0.3, 0.7, 0.9, 1.7, 2.3, 0.6, 1.1)):      # constants: Q / n may round below m^2
        t = (k * 37 + 5) % n
        a = q = F(0)
        for _ in range(8):
            a, q = F(a + F(v)), F(q + F(F(v) * F(v)))
        count[t], A[t], Q[t] = 8, a, q
    return count.reshape(H, W), A.reshape(H, W), Q.reshape(H, W), blk, cov


def _coverage_of(name, H, W):
    return np.array(br.reference(name, H, W)["coverage"], np.uint8)


@pytest.mark.parametrize("name,size", [("square", (3, 5)), ("cube_atlas", (11, 13)), ("copy_atlas", (16, 24)), ("cube_atlas", (40, 72)),
                                       ("synthetic", (264, 264))])
def test_block_select_equals_the_replay_on_every_branch(name, size):
    H, W = size
    r = prt.HipWavefrontRenderer(device=0)              # a device and a context: no scene, no film
    if name == "synthetic":                             # 33 x 33 = 1089 blocks: the block compaction runs two strides
        rng = np.random.default_rng(12)
        coverage = (rng.random((H, W)) < 0.5).astype(np.uint8)
        coverage[np.isin(ar.block_of(H, W), rng.choice(1089, 300, replace=False))] = 0
        coverage[rng.random((H, W)) < 0.01] = 2         # filled texels of a dilated map: not covered
    else:
        coverage = _coverage_of(name, H, W)
    count, A, Q, blk, cov = _synthetic(H, W, coverage, 5)
    nb = ar.block_count(H, W)
    covered_blocks = set(np.unique(blk[cov]).tolist())
    if name == "cube_atlas" and size == (40, 72):
        assert len(covered_blocks) < nb                 # some blocks have no covered texel
    # planted by position: the last lane of a covered block is its only unconverged texel; an uncovered texel is the only
    # unconverged one of its block
    flat = lambda a: a.reshape(-1)
    last = None
    for b in sorted(covered_blocks):
        t = np.nonzero(blk == b)[0]
        if cov[t[-1]] and (t[-1] // W) % 8 == 7 and (t[-1] % W) % 8 == 7:
            flat(count)[t], flat(A)[t], flat(Q)[t] = 8, 8.0, 8.0
            flat(Q)[t[-1]] = 80.0
            last = b
            break
    lone = None
    for b in range(nb):
        t = np.nonzero(blk == b)[0]
        if b != last and (~cov[t]).any() and cov[t].any():
            flat(count)[t], flat(A)[t], flat(Q)[t] = 8, 8.0, 8.0
            flat(Q)[t[~cov[t]][0]] = 80.0
            lone = b
            break
    thr, floor = 0.1, 0.0
    un = ar.unconverged(count, A, Q, thr, floor).ravel()
    d = flat(Q).astype(np.float64) / 8.0 - (flat(A).astype(np.float64) / 8.0) ** 2
    assert (d[flat(count) == 8] < 0).any(), "no texel whose Q / n rounds below m^2"
    assert not un[np.isnan(flat(A)) & (flat(count) >= 2)].any() and un[flat(count) < 2].all()
    rng = np.random.default_rng(8)
    shuffled = rng.permutation(nb).astype(np.uint32)
    prevs = [None, shuffled, shuffled[: nb // 2], np.zeros(0, np.uint32), np.arange(nb, dtype=np.uint32)[::-1].copy()]
    for prev in prevs:
        want_b, want_t = ar.select(coverage, count, A, Q, prev, thr, floor)
        got_b, got_t = r.bake_block_select(coverage, count, A, Q, thr, floor, prev=prev)
        assert np.array_equal(got_b, want_b), (name, size, None if prev is None else len(prev), got_b[:8], want_b[:8])
        assert np.array_equal(got_t, want_t), (name, size, len(got_t), len(want_t))
    all_b, all_t = ar.select(coverage, count, A, Q, None, thr, floor)
    print(f"select {name} {H}x{W}: {len(all_b)} of {nb} blocks active ({len(covered_blocks)} hold covered texels), {len(all_t)} texels listed")
    if last is not None:
        assert last in all_b.tolist()
    if lone is not None:
        assert lone not in all_b.tolist()
    if H * W >= 40 * 72:
        assert last is not None and lone is not None and 0 < len(all_b) < len(covered_blocks)
    assert set(all_b.tolist()) <= covered_blocks


# ---- 2. the loop against the public pieces --------------------------------------------------------------------------------
def _sample_values(r, kw, H, W, s, variant, cov):
    """[H * W, 3]: the value of sample s of every texel, from the public functions; -> (values, segments, shadow rays)"""
    ray = r.bake_rays(size=(H, W), sample=s, **kw)
    o, d, st = ray["o"].reshape(-1, 3)[cov], ray["d"].reshape(-1, 3)[cov], ray["rng_state"].ravel()[cov]
    out = np.zeros((H * W, 3), F)
    if variant == "texel":
        ls = r.bake_light_samples(size=(H, W), sample=s, **kw)
        tmax, w, contrib = ls["tmax"].ravel()[cov], ls["dir"].reshape(-1, 3)[cov], ls["contrib"].reshape(-1, 3)[cov]
        p = r.bake_surface(size=(H, W), **kw)["position"].reshape(-1, 3)[cov]
        occ = r.occluded(p, w, tmax)
        e = np.where(((tmax > 0) & ~occ)[:, None], contrib, F(0)).astype(F)
        _, q = r.radiance(o, d, rng_state=st, samples=1, return_info=True, lighting=True, pb=ls["ray_pb"].ravel()[cov])
        out[cov] = (q["sum"] + e).astype(F)
        return out, q["segments"].astype(np.int64), q["shadow_rays"] + int((tmax > 0).sum())
    _, q = r.radiance(o, d, rng_state=st, samples=1, return_info=True, lighting=variant == "lit")
    out[cov] = q["sum"]
    return out, q["segments"].astype(np.int64), q.get("shadow_rays", 0)


def _setup(case):
    """-> (renderer, target keywords, variant, bake keywords, (H, W), (min, step, max), threshold, noise_floor).  The
    thresholds are inputs chosen so that the loop has something to decide: with them the replay over the device's per-sample
    values ends with the counts {2, 5, 8, 10} (texel), {2, 4, 6, 8} (lit_small), {4, 6, 8} (lit), {11} after two passes
    (unlit_tiny) and {7, 11} (unlit)."""
    if case == "texel":          # Cornell box, the cube's atlas: rows of blocks without a covered texel
        sc, kw, _ = target_scene("cornell")
        r, _ = renderer(sc)
        configure(r, "cornell", "mis")
        return r, kw, "texel", dict(lighting=True, texel_light=True), (40, 72), (2, 3, 10), 0.6, 0.01
    if case in ("lit_small", "lit"):      # the placed copy, textured
        sc, kw, _ = target_scene("copy")
        r, _ = renderer(sc)
        configure(r, "copy", "mis")
        return r, kw, "lit", dict(lighting=True), (11, 13) if case == "lit_small" else (16, 24), (2, 2, 8), 0.6 if case == "lit_small" else 0.3, 0.01
    sc, _ = br.ff_scene()                # unlit: the square under the emissive quad
    r, _ = renderer(sc)
    kw = dict(mesh=0, uvs=br.square_mesh().GetUVs())
    return r, kw, "unlit", dict(), (3, 5) if case == "unlit_tiny" else (11, 13), (3, 4, 12), 0.6 if case == "unlit_tiny" else 0.9, 0.01


CASES = ("texel", "lit_small", "lit", "unlit_tiny", "unlit")


@functools.lru_cache(maxsize=None)
def _reference(case):
    """The replay's loop over the device's own per-sample values; computed once, shared, never written to"""
    r, kw, variant, bake_kw, (H, W), (lo, step, hi), thr, floor = _setup(case)
    cov = r.bake_surface(size=(H, W), **kw)["coverage"]
    on = cov.ravel() != 0
    per = [_sample_values(r, kw, H, W, 1 + s, variant, on) for s in range(hi)]        # first_sample = 1
    values = np.stack([p[0] for p in per])
    want = ar.run(cov, values, lo, step, hi, thr, floor)
    cnt = want["count"].ravel()[on].astype(np.int64)
    want["segments"] = int(sum(per[s][1][cnt > s].sum() for s in range(hi)))
    want["shadow_rays"] = None
    if variant != "unlit":       # (the query reports its shadow rays per call, not per ray: only a uniform outcome adds up here)
        want["shadow_rays"] = sum(p[2] for p in per[: int(cnt.max())]) if (cnt == cnt[0]).all() else None
    for a in want.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    values.setflags(write=False)
    return r, kw, bake_kw, (H, W), (lo, step, hi), thr, floor, cov, want, values


def _same(got, want, cov):
    bad = [k for k, w in (("sum", "rgb_sum"), ("count", "count"), ("sum_y", "sum_y"), ("sum_y2", "sum_y2")) if not np.array_equal(bits(got[k]), bits(want[w]))]
    if not np.array_equal(bits(got["mean"]), bits(ar.mean(want["rgb_sum"], want["count"]))):
        bad.append("mean")
    if not np.array_equal(got["coverage"], cov):
        bad.append("coverage")
    if got["adaptive"] != want["info"]:
        bad.append(("adaptive", got["adaptive"], want["info"]))
    return bad


@pytest.mark.parametrize("case", CASES)
def test_the_loop_equals_the_replay_over_the_public_pieces(case):
    r, kw, bake_kw, (H, W), (lo, step, hi), thr, floor, cov, want, _ = _reference(case)
    on = cov != 0
    hist = dict(zip(*np.unique(want["count"][on], return_counts=True)))
    print(f"{case} {H}x{W} thr {thr}: counts {hist}, info {want['info']}")
    assert on.sum() >= 10 and want["rgb_sum"].any() and want["info"]["passes"] >= 2
    assert len(hist) >= 2 or case == "unlit_tiny"        # (one block: one count)
    for chunk in (1, 3, 0):
        r.set_param("bake_chunk", chunk)
        got = r.bake_irradiance_adaptive(size=(H, W), threshold=thr, min_spp=lo, step_spp=step, max_spp=hi, noise_floor=floor, first_sample=1,
                                         **bake_kw, **kw)
        assert _same(got, want, cov) == [], (case, chunk, _same(got, want, cov))
        assert not got["count"][~on].any() and not got["sum"][~on].any() and not got["sum_y2"][~on].any()
        assert np.array_equal(bits(got["irradiance"]), bits(got["mean"] * F(np.pi)))
        info = got["info"]
        assert info["rays"] == want["info"]["texel_samples"] == int(got["count"].sum(dtype=np.float64)) and info["n_covered"] == on.sum()
        assert info["segments"] == want["segments"]
        if want["shadow_rays"] is not None:
            assert info["shadow_rays"] == want["shadow_rays"]
        assert (info["shadow_rays"] > 0) == bool(bake_kw)
    r.set_param("bake_chunk", 0)
    noise = prt.bake_noise(got["count"], got["sum_y"], got["sum_y2"], floor)
    assert np.array_equal(bits(noise), bits(ar.noise(want["count"], want["sum_y"], want["sum_y2"], floor))) and not noise[~on].any()


# ---- 3. the headline property ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("texel", "lit", "unlit"))
def test_a_texel_with_count_n_is_that_texel_of_the_uniform_n_sample_bake(case):
    r, kw, bake_kw, (H, W), (lo, step, hi), thr, floor, cov, want, _ = _reference(case)
    got = r.bake_irradiance_adaptive(size=(H, W), threshold=thr, min_spp=lo, step_spp=step, max_spp=hi, noise_floor=floor, first_sample=1,
                                     **bake_kw, **kw)
    on = cov != 0
    counts = np.unique(got["count"][on]).astype(int)
    assert counts.min() >= lo and counts.max() <= hi
    for n in counts:
        _, uni = r.bake_irradiance(size=(H, W), samples=int(n), first_sample=1, return_info=True, **bake_kw, **kw)
        at = on & (got["count"] == n)
        assert np.array_equal(bits(got["sum"][at]), bits(uni["sum"][at])), (case, n, int(at.sum()))


# ---- 4. a mix is really produced ------------------------------------------------------------------------------------------
def shadow_scene():
    """The 2 x 2 square under the emissive quad of the form-factor case, with an occluder 0.04 above the map's top-left block
    (rows 0..7, columns 0..7 of a 16 x 24 map: x in [-1, -1/3], z in [-1, 0]) that overhangs it by 0.25: that block lies in the
    umbra (every value 0), the blocks beside it hold the penumbra, the far ones see the whole emitter."""
    sc, _ = br.ff_scene()
    sc.AddQuad(1.1667, 1.5, sc.AddLambertian((0.5, 0.5, 0.5)), translation=(-0.6667, 0.04, -0.5))
    return sc


# threshold 0.3 with noise_floor 0.01, chosen by running the replay's loop over the device's own per-sample values of this
# scene (mis + texel light, depth 2, 16 x 24, min 4 / step 4 / max 16, first_sample 0, seed 11).  Counts per block, row-major:
#   threshold 0.2: 4 16 16 / 16 16 16     0.25: 4 16 16 / 16 12 12     0.3: 4 16 12 / 12 8 12 (one block capped)
#   0.4 and 0.5: 4 16 8 / 8 8 8           0.7: 4 16 4 / 4 4 4
MIX_THRESHOLD = 0.3


def test_umbra_penumbra_and_open_light_give_a_mix_of_counts():
    r, _ = renderer(shadow_scene(), depth=2)
    r.set_lighting("mis")
    kw = dict(mesh=0, uvs=br.square_mesh().GetUVs())
    got = r.bake_irradiance_adaptive(size=(16, 24), threshold=MIX_THRESHOLD, min_spp=4, step_spp=4, max_spp=16, lighting=True, texel_light=True, **kw)
    on = got["coverage"] == 1
    assert on.all()
    blk = ar.block_of(16, 24)
    per_block = [np.unique(got["count"][blk == b]) for b in range(6)]
    print("mix: counts per block", [c.tolist() for c in per_block], got["adaptive"])
    assert all(len(c) == 1 for c in per_block)                              # a block's texels share their count
    assert len(np.unique(got["count"])) >= 3
    assert got["adaptive"]["blocks_capped"] >= 1 and (np.concatenate(per_block) == 4).any()
    assert per_block[0].tolist() == [4] and not got["sum"][blk == 0].any()   # the umbra: every value is 0, variance 0
    assert got["adaptive"]["min_texel_spp"] == 4 and got["adaptive"]["max_texel_spp"] == 16
    assert got["adaptive"]["blocks_converged"] + got["adaptive"]["blocks_capped"] == 6


# ---- 5. degenerate ends ---------------------------------------------------------------------------------------------------
def test_a_constant_sky_stops_everything_at_min_spp():
    sc, target, _ = scene_of("square")
    r, _ = renderer(sc)
    uv = br.shape("square")["mesh"].GetUVs()
    got = r.bake_irradiance_adaptive(size=(11, 13), uvs=uv, threshold=0.01, min_spp=4, step_spp=4, max_spp=16, noise_floor=0.0, **target)
    on = got["coverage"] == 1
    assert on.sum() > 100 and (got["count"][on] == 4).all()
    assert got["adaptive"] == dict(passes=0, blocks=4, blocks_converged=4, blocks_capped=0, min_texel_spp=4, max_texel_spp=4,
                                   texel_samples=4 * int(on.sum()))
    _, uni = r.bake_irradiance(size=(11, 13), uvs=uv, samples=4, return_info=True, **target)
    assert np.array_equal(bits(got["sum"]), bits(uni["sum"])) and got["sum"].any()


def test_max_equal_min_is_the_uniform_bake_with_statistics():
    r, kw, bake_kw, (H, W), _, thr, floor, cov, _, values = _reference("texel")
    got = r.bake_irradiance_adaptive(size=(H, W), threshold=thr, min_spp=5, step_spp=0, max_spp=5, first_sample=1, dilate=1, **bake_kw, **kw)
    irr, uni = r.bake_irradiance(size=(H, W), samples=5, first_sample=1, return_info=True, **bake_kw, **kw)
    on = cov != 0
    assert np.array_equal(bits(got["sum"]), bits(uni["sum"])) and (got["count"][on] == 5).all() and not got["count"][~on].any()
    assert got["adaptive"] == dict(passes=0, blocks=ar.block_count(H, W), blocks_converged=0, blocks_capped=0, min_texel_spp=5, max_texel_spp=5,
                                   texel_samples=5 * int(on.sum()))
    for k in ("rays", "segments", "shadow_rays", "shadow_occluded", "n_covered"):
        assert got["info"][k] == uni["info"][k], k
    st = (np.zeros((H * W, 3), F), np.zeros(H * W, F), np.zeros(H * W, F), np.zeros(H * W, F))
    ar.add_samples(st, values[:5])
    assert np.array_equal(bits(got["sum_y"].ravel()[on.ravel()]), bits(st[2][on.ravel()]))
    assert np.array_equal(bits(got["sum_y2"].ravel()[on.ravel()]), bits(st[3][on.ravel()]))


def test_a_tiny_threshold_caps_everything():
    r, kw, bake_kw, (H, W), (lo, step, hi), _, _, cov, _, values = _reference("unlit")
    want = ar.run(cov, values, lo, step, hi, 1e-6, 0.0)
    got = r.bake_irradiance_adaptive(size=(H, W), threshold=1e-6, min_spp=lo, step_spp=step, max_spp=hi, noise_floor=0.0, first_sample=1, **kw)
    on = cov != 0
    assert _same(got, want, cov) == []
    assert (got["count"][on] == hi).all() and got["adaptive"]["blocks_capped"] == got["adaptive"]["blocks"] == 4
    assert got["adaptive"]["blocks_converged"] == 0 and got["adaptive"]["passes"] == 3      # 3 + 4 + 4 + 1


# ---- 6. gutter fill -------------------------------------------------------------------------------------------------------
def test_the_gutter_fill_acts_on_the_mean_alone():
    r, kw, bake_kw, (H, W), (lo, step, hi), thr, floor, cov, want, _ = _reference("texel")
    got = r.bake_irradiance_adaptive(size=(H, W), threshold=thr, min_spp=lo, step_spp=step, max_spp=hi, noise_floor=floor, first_sample=1,
                                     dilate=2, **bake_kw, **kw)
    assert len(np.unique(want["count"][cov != 0])) >= 2          # neighbouring texels do have different counts
    cov2, mean2, filled = br.dilate(cov, ar.mean(want["rgb_sum"], want["count"]), 2)
    assert filled > 50 and np.array_equal(got["coverage"], cov2) and np.array_equal(bits(got["mean"]), bits(mean2))
    assert got["info"]["n_filled"] == filled
    for k, w in (("sum", "rgb_sum"), ("count", "count"), ("sum_y", "sum_y"), ("sum_y2", "sum_y2")):
        assert np.array_equal(bits(got[k]), bits(want[w])), k
    assert not got["count"][cov2 == 2].any()


# ---- 7. nothing else moves ------------------------------------------------------------------------------------------------
def _state(r, film):
    r.download()
    return (film.accum.copy(), film.weights.copy(), bytes(r.stats()), dict(r.batch_instances()), bytes(r.light_stats())) + \
        tuple(a.copy() for a in r.film_statistics())


def test_an_adaptive_bake_leaves_the_film_and_the_next_calls_alone():
    def run(with_bake):
        sc, kw, _ = target_scene("cornell")
        r, film = renderer(sc)
        r.set_lighting("mis")
        r.set_light_sources("all")
        r.set_film_statistics(True)
        r.ProgressiveRender(2)
        before = _state(r, film)
        got = None
        if with_bake:
            call = lambda: r.bake_irradiance_adaptive(size=(16, 24), threshold=0.3, min_spp=2, step_spp=2, max_spp=6, dilate=1, lighting=True,
                                                      texel_light=True, **kw)
            got = call()
            calls = prt.device_memory_info()[1]
            again = call()
            assert prt.device_memory_info()[1] == calls              # the second identical call allocates nothing
            assert all(np.array_equal(bits(got[k]), bits(again[k])) for k in ("sum", "count", "sum_y", "sum_y2", "mean"))
            r.bake_block_select(got["coverage"], got["count"], got["sum_y"], got["sum_y2"], 0.3)
        after = _state(r, film)
        _, plain = r.bake_irradiance(size=(16, 24), samples=3, lighting=True, texel_light=True, return_info=True, **kw)
        r.ProgressiveRender(2)
        r.download()
        return before, after, film.accum.copy(), film.weights.copy(), plain["sum"], got

    b0, a0, film0, w0, plain0, _ = run(False)
    b1, a1, film1, w1, plain1, got = run(True)
    for x, y in zip(b1, a1):          # across the bake itself
        assert (np.array_equal(bits(x), bits(y)) if isinstance(x, np.ndarray) else x == y)
    assert np.array_equal(bits(film0), bits(film1)) and np.array_equal(w0, w1)    # the render after it
    assert np.array_equal(bits(plain0), bits(plain1)) and plain0.any()            # a plain bake after it
    assert got["sum"].any() and got["adaptive"]["passes"] >= 1


# ---- 8. device form -------------------------------------------------------------------------------------------------------
def test_the_torch_form_equals_the_host_form_and_the_workspace_regrows():
    sc, kw, _ = target_scene("cornell")
    r, _ = renderer(sc)
    configure(r, "cornell", "mis")
    args = dict(threshold=0.3, min_spp=2, step_spp=3, max_spp=7, lighting=True, texel_light=True, dilate=1, **kw)
    host = {}
    for size in ((11, 13), (40, 72), (11, 13)):          # small, larger, back
        got = r.bake_irradiance_adaptive(size=size, **args)
        if size in host:
            assert all(np.array_equal(bits(got[k]), bits(host[size][k])) for k in ("sum", "count", "sum_y", "sum_y2", "mean"))
            assert np.array_equal(got["coverage"], host[size]["coverage"])
        host[size] = got
        dev = r.bake_irradiance_adaptive(size=size, out="torch", **args)
        assert dev["sum"].is_cuda and dev["coverage"].dtype.is_floating_point is False
        for k in ("sum", "count", "sum_y", "sum_y2", "mean", "irradiance"):
            assert np.array_equal(bits(dev[k].cpu().numpy()), bits(got[k])), (size, k)
        assert np.array_equal(dev["coverage"].cpu().numpy(), got["coverage"])
        assert dev["adaptive"] == got["adaptive"] and dev["info"]["segments"] == got["info"]["segments"]
        assert got["adaptive"]["passes"] >= 1 and got["sum"].any()
