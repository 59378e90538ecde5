"""CPU-side tests of the temporal reprojection's contract (include/prt.h "Temporal reprojection") through its numpy
restatement (tests/temporal_replay.py): a static scene keeps every hit pixel's history, a disocclusion takes none and returns
its inputs, the deliberately wrong variants are told apart, and what the history is worth in front of the a-trous filter.

Quality fixture (test_denoise_replay.py's): camera (5, 5, 8) toward the origin, 44 x 28, depth 5, seed 3.  Eight frames of ONE
oracle sample each (sample index = frame index), the camera orbiting 2 degrees per frame about the vertical axis through the
origin, the oracle's own centre-ray features per frame.  Temporal then a-trous (both with their defaults) at the last frame
against the oracle's 1024-sample target at the last camera; the baseline is the a-trous filter alone on the last one-sample
frame.  MSE ratios (temporal + a-trous) / (a-trous alone) measured by this file on the CPU:
    CORNELL 0.850, LIGHT_TEST 0.241, DEFAULT 0.158, MATERIAL_TEST 0.327
(CORNELL's one-sample frames are fireflies on black: a firefly stays in the history at 1 / N' of its height, so the temporal
mean alone, MSE 0.876, is worse there than the last one-sample frame, 0.226; both filters together still beat the a-trous
filter alone, 0.579 against 0.681.)
Every preset whose ratio is below 1 is gated at min(1, 1.5 x its measured ratio): the margin covers nothing but a later change
of the defaults."""
import functools
import math

import numpy as np
import pytest

import adaptive_replay as ar
import denoise_replay as dr
import temporal_replay as tr
import util
from util import prt

F = np.float32
FX = dict(cam_pos=(5.0, 5.0, 8.0), W=44, H=28, depth=5, seed=3, frames=8, orbit_deg=2.0, target_spp=1024)
MEASURED = {"CORNELL": 0.850, "LIGHT_TEST": 0.241, "DEFAULT": 0.158, "MATERIAL_TEST": 0.327}


def orbit(pos, deg):
    """pos turned deg degrees about the vertical axis through the origin (what prt_render --orbit-deg does per frame)."""
    a = math.radians(deg)
    x, y, z = pos
    return (x * math.cos(a) + z * math.sin(a), y, -x * math.sin(a) + z * math.cos(a))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F else a.dtype)


def one_sample_frame(osc, scene, pos, sample):
    W, H = FX["W"], FX["H"]
    cam = prt.Camera(position=pos, width=W, height=H)
    f = osc.render(cam.desc(), W, H, spp=1, first_sample=sample, max_depth=FX["depth"], seed=FX["seed"], iterative=True, n_threads=8)[0]
    A, Q = ar.moments([f])
    feat = dr.oracle_features(osc, scene, cam.desc(), W, H)
    K = tr.basis(pos, cam.front, W, H)
    return dict(c=f.astype(F), n=np.ones((H, W), F), A=A, Q=Q, feat=feat, K=K, cam=cam)


@functools.lru_cache(maxsize=None)
def quality(preset):
    scene = prt.Scene(preset)
    osc = util.oracle_scene(scene)
    W, H = FX["W"], FX["H"]
    hist, Kprev, pos, out, fr = None, None, FX["cam_pos"], None, None
    for i in range(FX["frames"]):
        fr = one_sample_frame(osc, scene, pos, i)
        ft = fr["feat"]
        out = tr.reproject(Kprev if Kprev is not None else fr["K"], fr["c"], fr["n"], fr["A"], fr["Q"], ft["prim"], ft["position"], ft["normal"],
                           history=hist, guard=False)
        hist = tr.next_history(out, ft["position"], ft["normal"], ft["prim"])
        Kprev = fr["K"]
        if i + 1 < FX["frames"]:
            pos = orbit(pos, FX["orbit_deg"])
    ft = fr["feat"]
    target = osc.render(fr["cam"].desc(), W, H, spp=FX["target_spp"], first_sample=FX["frames"], max_depth=FX["depth"], seed=FX["seed"],
                        iterative=True, n_threads=8)[0].astype(np.float64) / FX["target_spp"]
    both, _ = dr.denoise(out["c"], out["var"], ft["albedo"], ft["normal"], ft["position"], ft["prim"], guard=False)
    _, var1 = dr.film_inputs(fr["c"], fr["n"], fr["A"], fr["Q"])
    alone, _ = dr.denoise(fr["c"], var1, ft["albedo"], ft["normal"], ft["position"], ft["prim"], guard=False)
    mse = lambda a: float(np.mean((a.astype(np.float64) - target) ** 2))  # noqa: E731
    return dict(noisy=mse(fr["c"]), temporal=mse(out["c"]), both=mse(both), alone=mse(alone), status=float(out["status"].mean()), out=both)


@pytest.mark.parametrize("preset", ["CORNELL", "LIGHT_TEST", "DEFAULT", "MATERIAL_TEST"])
def test_history_in_front_of_the_filter_lowers_the_mse(preset):
    r = quality(preset)
    ratio = r["both"] / r["alone"]
    print(f"{preset}: one-sample MSE {r['noisy']:.4e}, a-trous alone {r['alone']:.4e}, temporal alone {r['temporal']:.4e}, "
          f"temporal + a-trous {r['both']:.4e}, ratio {ratio:.3f}, status 1 on {r['status']:.3f} of the pixels")
    assert np.isfinite(r["out"]).all()
    assert MEASURED[preset] < 1.0    # (a preset measured at or above 1 would be a reported counter-example, not a gate)
    assert ratio < min(1.0, 1.5 * MEASURED[preset]), ratio


def test_at_least_two_presets_are_gated():
    assert sum(1 for v in MEASURED.values() if v < 1.0) >= 2


# ---- identity ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def static_frame(which):
    W, H = FX["W"], FX["H"]
    if which == "CORNELL":
        scene, pos = prt.Scene("CORNELL"), FX["cam_pos"]
    else:
        scene, pos = prt.scenes.mesh_scene(prt.Mesh(prt.scenes.asset("bunny.ply"))), (2.0, 1.5, 3.0)
    osc = util.oracle_scene(scene)
    return one_sample_frame(osc, scene, pos, 0)


@pytest.mark.parametrize("which", ["CORNELL", "bunny"])
def test_a_static_scene_keeps_every_hit_pixel(which):
    """Same basis, static scene: every hit pixel has status 1, and N' = min(hn + n, max_history) where hn is uniform.
    "Exactly" holds where fp32 makes it hold: the contract's Nh = (sum of b * hn) / (sum of b) in its pinned order is hn itself
    when hn is a power of two (scaling by one commutes with every rounding), and for any hn once max_history caps it.  For
    another uniform hn the quotient carries the roundings of the four products: measured here, N' is off by one ulp on 20 of
    859 (CORNELL) and 9 of 843 (bunny) hit pixels at hn = 5, never by more; that case is held to one ulp."""
    fr = static_frame(which)
    ft = fr["feat"]
    H, W = fr["n"].shape
    rng = np.random.default_rng(2)
    hit = ft["prim"] >= 0
    assert hit.sum() > 100
    for hn_value, maxh, exact in ((1.0, 32.0, True), (4.0, 32.0, True), (16.0, 1000.0, True), (31.5, 32.0, True), (3.0, 1.0, True),
                                  (5.0, 32.0, False), (3.0, 32.0, False)):
        hist = dict(hc=rng.uniform(0, 2, (H, W, 3)).astype(F), hn=np.full((H, W), F(hn_value)), h1=rng.uniform(0.5, 1, (H, W)).astype(F),
                    h2=rng.uniform(1, 2, (H, W)).astype(F), hP=ft["position"], hN=ft["normal"], hprim=ft["prim"])
        out = tr.reproject(fr["K"], fr["c"], fr["n"], fr["A"], fr["Q"], ft["prim"], ft["position"], ft["normal"], history=hist, max_history=maxh,
                           guard=False)
        assert (out["status"][hit] == 1).all(), (which, int((out["status"][hit] == 0).sum()))   # every hit pixel, no exclusions
        assert (out["status"][~hit] == 0).all()
        want = np.minimum(F(hn_value) + fr["n"], F(maxh)).astype(F)
        if exact:
            assert np.array_equal(bits(out["n"][hit]), bits(want[hit])), (hn_value, maxh)
        else:
            assert (np.abs(out["n"][hit] - want[hit]) <= np.spacing(want[hit])).all(), (hn_value, maxh)


# ---- disocclusion -----------------------------------------------------------------------------------------------------------
def geometrically_revealed(K, cur, hist):
    """The wall pixels of the current frame whose point, projected into the previous camera in float64, has a 2 x 2 bilinear
    footprint that lies in the image and holds front-plane pixels only: the wall there was hidden in the previous frame.  The
    footprint is taken one pixel wider than floor / floor + 1 on each side, so that it does not depend on how the fp32 contract
    rounds a coordinate next to an integer."""
    H, W = cur["n"].shape
    v = cur["Pprev"].astype(np.float64) - np.asarray(K["pos"], np.float64)
    z = v @ np.asarray(K["front"], np.float64)
    x, y = v @ np.asarray(K["right"], np.float64), v @ np.asarray(K["up"], np.float64)
    t = float(K["tan_fov_y"])
    with np.errstate(all="ignore"):
        fx = ((x / z) / ((W / H) * t) + 1) * 0.5 * W - 0.5
        fy = (1 - (y / z) / t) * 0.5 * H - 0.5
    ok = (cur["prim"] == 0) & (z > 0) & (fx >= 1) & (fx < W - 2) & (fy >= 1) & (fy < H - 2)
    ix, iy = np.where(ok, np.floor(fx), 1).astype(int), np.where(ok, np.floor(fy), 1).astype(int)
    front = hist["hprim"] == 1
    covered = np.ones((H, W), bool)
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            covered &= front[iy + dy, ix + dx]
    return ok & covered


def test_a_disocclusion_takes_no_history_and_returns_its_inputs():
    K, cur, hist = tr.two_planes()
    out = tr.reproject(K, **cur, history=hist)   # (guard on: this fixture is one the GPU is compared on bit for bit)
    kind = out["kind"]
    hit = cur["prim"] >= 0
    counts = {name: int((kind == k).sum()) for name, k in (("status 1", 1), ("behind", 2), ("off-screen", 3), ("disoccluded", 4))}
    counts["miss"] = int((~hit).sum())
    print(counts)
    assert all(v > 0 for v in counts.values()), counts                     # no case is vacuous
    assert np.array_equal(out["status"] == 1, kind == 1)
    # the newly revealed pixels, from the fixture's geometry alone (float64, nothing of the replay): wall (prim 0) now, and
    # in the previous frame the front plane (hprim 1) covers every pixel of the 2 x 2 footprint their point projects into
    revealed = geometrically_revealed(K, cur, hist)
    assert revealed.sum() > 20
    none = out["status"] == 0
    assert none[revealed].all(), int((~none[revealed]).sum())
    assert (kind[revealed] == 4).all()                                       # ... refused by the tap tests, not for leaving the screen
    assert none[~hit].all() and none[kind == 2].all() and none[kind == 3].all()
    n = cur["n"]
    m1, m2 = (cur["A"] / n).astype(F), (cur["Q"] / n).astype(F)
    _, var = dr.film_inputs(np.zeros_like(cur["c"]), n, cur["A"], cur["Q"])
    for name, want in (("c", cur["c"]), ("n", n), ("m1", m1), ("m2", m2), ("var", var)):
        assert np.array_equal(bits(out[name][none]), bits(want[none])), name
    # and the pixels that do take history differ from their inputs
    assert not np.array_equal(out["c"][kind == 1], cur["c"][kind == 1])


def test_no_history_at_all_returns_the_inputs():
    K, cur, _ = tr.two_planes()
    out = tr.reproject(K, **cur, history=None)
    assert (out["status"] == 0).all() and np.array_equal(bits(out["c"]), bits(cur["c"])) and np.array_equal(bits(out["n"]), bits(cur["n"]))


def test_wrong_variants_are_told_apart():
    """On two_planes() (44 x 28): without the plane test the revealed wall takes the front plane's history; without the
    normal test (at plane_tol 0.05, where the corner's taps pass the plane test) the back wall takes the side wall's; the
    nearest tap instead of the bilinear four changes nearly every reprojected pixel."""
    K, cur, hist = tr.two_planes()
    n_pix = cur["n"].size
    ref = tr.reproject(K, **cur, history=hist)
    changed = lambda o, r: float((bits(o["c"]) != bits(r["c"])).any(axis=-1).sum()) / n_pix  # noqa: E731
    no_plane = tr.reproject(K, **cur, history=hist, variant="no_plane")
    assert changed(no_plane, ref) > 0.10 and (no_plane["status"] != ref["status"]).sum() > 100
    ref5 = tr.reproject(K, **cur, history=hist, plane_tol=0.05)
    no_normal = tr.reproject(K, **cur, history=hist, plane_tol=0.05, variant="no_normal")
    assert changed(no_normal, ref5) > 0.015
    nearest = tr.reproject(K, **cur, history=hist, variant="nearest")
    assert changed(nearest, ref) > 0.5


def test_the_guard_passes_on_the_fixtures_and_refuses_subnormals():
    for kw, cfg in [(dict(), {}), (dict(hn_value=0.0), {}), (dict(fov_y=0.7), {})] + [(dict(W=w, H=h, **fx), cfg) for _, w, h, fx, cfg in tr.GPU_FIXTURES]:
        K, cur, hist = tr.two_planes(**kw)
        info = {}
        tr.reproject(K, **cur, history=hist, info=info, **cfg)
        assert info["below_guard"] == 0, (kw, cfg)
    K, cur, hist = tr.two_planes()
    hist["h1"] = np.full_like(hist["h1"], F(2.0 ** -125))
    with pytest.raises(AssertionError):
        tr.reproject(K, **cur, history=hist)
    info = {}
    tr.reproject(K, **cur, history=hist, guard=False, info=info)
    assert info["below_guard"] > 0


def test_the_variance_follows_the_blended_moments():
    K, cur, hist = tr.two_planes(hn_value=4.0)
    out = tr.reproject(K, **cur, history=hist)
    st = out["status"] == 1
    m1, m2, n = out["m1"][st].astype(np.float64), out["m2"][st].astype(np.float64), out["n"][st].astype(np.float64)
    want = (np.maximum(0.0, m2 - m1 * m1) / np.maximum(n - 1.0, 1.0)).astype(F)
    assert np.array_equal(bits(out["var"][st]), bits(want)) and (out["n"][st] == 6).all() and (out["var"][st] >= 0).all()


def test_the_previous_surface_rule_inverts_a_motion():
    rng = np.random.default_rng(4)
    from util import orc
    M0 = orc.make_transform((0.125, 0.125, 0.125), (10.0, 40.0, -20.0), (1.0, 2.0, -3.0))
    M1 = orc.make_transform((0.125, 0.125, 0.125), (-30.0, 5.0, 60.0), (1000.0, -2.0, 4.0))
    local = rng.uniform(-1, 1, (50, 3)).astype(F)
    nl = tr.normalize3(rng.normal(size=(50, 3)).astype(F))
    P1, N1 = tr.transform_point(np.asarray(M1[0], F).ravel(), local), tr.normalize3(tr.lin(np.asarray(M1[0], F).ravel(), nl))
    prim = np.arange(50, dtype=np.int32) + 7
    prim[::5] = 3     # not in the copy's range: stays
    Pp, Np = tr.prev_surface(P1, N1, prim, [7], [60], [np.asarray(M1[1], F).ravel()], [np.asarray(M0[0], F).ravel()])
    P0, N0 = tr.transform_point(np.asarray(M0[0], F).ravel(), local), tr.normalize3(tr.lin(np.asarray(M0[0], F).ravel(), nl))
    moved = prim >= 7
    assert np.allclose(Pp[moved], P0[moved], atol=2e-3) and np.allclose(Np[moved], N0[moved], atol=1e-4)   # (1000 away: ulp 6e-5, through a 1/8 scale)
    assert np.array_equal(Pp[~moved], P1[~moved]) and np.array_equal(Np[~moved], N1[~moved])
