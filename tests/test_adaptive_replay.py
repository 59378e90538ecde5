"""CPU-side tests of film statistics and tile-adaptive sampling (include/prt.h "Film statistics and adaptive sampling"):
the exported stopping rule against its float64 restatement (tests/adaptive_replay.py), every refusal of prt_render_adaptive
on a host-only context, the ctypes struct sizes, and the gate conditions of the fixtures the GPU tests replay (the two 44 x 28
ones below, and FIXTURE_WIDE, whose tile lists span several trips of the compaction kernel).

Fixtures (adaptive_replay.FIXTURE): CORNELL at threshold 0.10 and DEFAULT at 0.15, (5, 5, 8) camera toward the origin,
44 x 28 film, depth 4, seed 3, first_sample 0, 8 / 8 / 96 samples, noise floor 0.01.  The replay over the oracle's per-sample
frames (the throughput form and the recursive tracer give the same counts) stops CORNELL's 24 tiles 4 at 8, 4 at 16, 1 at 32
and 15 at 96 samples, smallest decision margin 5.6e-3; DEFAULT's 5 at 8, 2 at 72, 2 at 80 and 15 at 96, margin 8.8e-5."""
import ctypes as C
import functools

import numpy as np
import pytest

import adaptive_replay as ar
import util
from util import prt

capi = prt.capi
NAN, INF = float("nan"), float("inf")
INVALID, NO_DEVICE = 1, 2  # PRT_ERR_INVALID, PRT_ERR_NO_DEVICE


def _rule(n, A, Q, thr, floor):
    return bool(capi.lib().prt_adaptive_unconverged(float(n), float(A), float(Q), float(thr), float(floor)))


def test_exported_rule_equals_the_restatement_on_random_inputs():
    rng = np.random.default_rng(11)
    n = rng.integers(2, 400, 4000).astype(np.float32)
    mean = rng.uniform(0.0, 3.0, 4000)
    spread = rng.uniform(0.0, 2.0, 4000) * (rng.random(4000) < 0.8)
    A = (n * mean).astype(np.float32)
    Q = (n * (mean * mean + spread * spread)).astype(np.float32)
    thr = rng.choice([0.0, 0.01, 0.05, 0.1, 0.5, 1e9], 4000).astype(np.float32)
    floor = rng.choice([0.0, 0.01, 1.0], 4000).astype(np.float32)
    floor[(thr == 0) & (floor == 0)] = np.float32(0.01)
    want = ar.unconverged(n, A, Q, thr, floor)
    got = np.array([_rule(*v) for v in zip(n, A, Q, thr, floor)])
    assert np.array_equal(got, want)
    assert want.any() and not want.all()


@pytest.mark.parametrize("n,A,Q,thr,floor,want", [
    (0, 0, 0, 0.1, 0.01, True), (1, 0.5, 0.25, 0.1, 0.01, True), (1, 0.5, 0.25, 1e9, 0.01, True),   # n < 2
    (2, 1.0, 0.5, 0.1, 0.01, False),        # two equal samples: V = 0
    (2, 1.0, 1.0, 0.1, 0.01, True),         # samples 0 and 1
    (3, 0.3, np.float32(0.03) * np.float32(0.9999), 0.1, 0.01, False),  # Q / n < m^2 from rounding: V clamps to 0
    (16, 0, 0, 0.1, 0.01, False), (16, 0, 0, 0.1, 0.0, False), (16, 0, 0, 0.0, 0.01, False),        # a black pixel
    (16, 8.0, 8.0, 0.0, 0.01, True),        # threshold 0: any variance is too much
    (16, 8.0, 4.0, 0.0, 0.01, False),       # ... and none is not
    (16, 8.0, 8.0, 1e9, 0.01, False), (16, 8.0, 8.0, INF, 0.01, False),
])
def test_exported_rule_on_edge_inputs(n, A, Q, thr, floor, want):
    assert _rule(n, A, Q, thr, floor) == want
    assert bool(ar.unconverged(n, A, Q, thr, floor)) == want


def test_struct_sizes_and_symbols():
    assert C.sizeof(capi.PrtAdaptive) == 20 and C.sizeof(capi.PrtAdaptiveInfo) == 32
    assert capi.PrtAdaptiveInfo.pixel_samples.offset == 24
    for name in ("prt_set_film_statistics", "prt_film_statistics_read", "prt_film_noise_read", "prt_adaptive_unconverged",
                 "prt_render_adaptive", "prt_group_set_film_statistics", "prt_group_render_adaptive"):
        assert name in capi.SIGNATURES and getattr(capi.lib(), name)


def _host(stats=True):
    r = prt.HipWavefrontRenderer(device=-1, max_depth=4)
    if stats:
        r.set_film_statistics(True)
    return r


def _call(r, min_spp=8, step=8, max_spp=32, thr=0.1, floor=0.01, depth=4):
    cfg = capi.PrtAdaptive(min_spp, step, max_spp, thr, floor)
    info = capi.PrtAdaptiveInfo()
    return capi.lib().prt_render_adaptive(r._ctx, C.byref(cfg), depth, 0, 0, C.byref(info))


REFUSALS = [
    ("nan threshold", dict(thr=NAN)), ("negative threshold", dict(thr=-0.1)), ("nan floor", dict(floor=NAN)),
    ("negative floor", dict(floor=-1e-3)), ("both zero", dict(thr=0.0, floor=0.0)), ("max < min", dict(min_spp=8, max_spp=7)),
    ("step 0, max > min", dict(step=0, min_spp=8, max_spp=9)), ("depth 0", dict(depth=0)), ("depth 65", dict(depth=65)),
]


@pytest.mark.parametrize("what,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_on_a_host_only_context(what, kw):
    r = _host()
    assert _call(r, **kw) == INVALID, what
    assert capi.lib().prt_last_error(r._ctx)


def test_statistics_off_is_refused_and_valid_settings_reach_the_device_check():
    assert _call(_host(stats=False)) == INVALID
    r = _host()
    assert capi.lib().prt_get_film_statistics(r._ctx) == 1
    assert _call(r) == NO_DEVICE                                   # nothing wrong with the settings: there is no device
    assert _call(r, step=0, min_spp=8, max_spp=8) == NO_DEVICE      # step 0 is fine when max == min
    assert _call(r, thr=0.0) == NO_DEVICE and _call(r, floor=0.0) == NO_DEVICE and _call(r, thr=INF) == NO_DEVICE
    assert capi.lib().prt_render_adaptive(r._ctx, None, 4, 0, 0, None) == INVALID
    assert capi.lib().prt_render_adaptive(None, None, 4, 0, 0, None) == INVALID
    r.set_film_statistics(False)
    assert capi.lib().prt_get_film_statistics(r._ctx) == 0 and _call(r) == INVALID
    with pytest.raises(prt.PrtError):
        r.render_adaptive(0.1)


@functools.lru_cache(maxsize=None)
def fixture_replay(preset, iterative=True):
    fx = ar.FIXTURE
    osc = util.oracle_scene(prt.Scene(preset))
    cam = prt.Camera(position=fx["cam_pos"], width=fx["W"], height=fx["H"]).desc()

    @functools.lru_cache(maxsize=None)
    def frame(s):
        return osc.render(cam, fx["W"], fx["H"], spp=1, first_sample=s, max_depth=fx["depth"], seed=fx["seed"],
                          iterative=iterative, n_threads=8)[0]

    rp = ar.Replay(fx["W"], fx["H"], frame)
    return rp, rp.run(fx["min_spp"], fx["step_spp"], fx["max_spp"], ar.FIXTURE_THRESHOLDS[preset], fx["noise_floor"])


@pytest.mark.parametrize("preset,stops", [("CORNELL", {8: 4, 16: 4, 32: 1, 96: 15}), ("DEFAULT", {8: 5, 72: 2, 80: 2, 96: 15})])
def test_fixture_gate_conditions(preset, stops):
    fx = ar.FIXTURE
    rp, out = fixture_replay(preset)
    u, c = np.unique(out["counts"], return_counts=True)
    assert dict(zip(u.tolist(), c.tolist())) == stops
    counts = out["counts"]
    assert (counts == fx["min_spp"]).any() and (counts == fx["max_spp"]).any()
    assert ((counts > fx["min_spp"]) & (counts < fx["max_spp"])).any()
    assert out["margins"].size and out["margins"].min() >= 1e-9   # one rounding in float64 (1.1e-16) cannot flip a tile
    assert np.array_equal(rp.n, rp.count_map(counts))
    info = out["info"]
    assert info["tiles_converged"] + info["tiles_capped"] == info["tiles_local"] == 24
    assert info["pixel_samples"] == int(rp.n.sum()) and info["min_tile_spp"] == 8 and info["max_tile_spp"] == 96
    # the recursive tracer's frames decide every tile the same way
    assert np.array_equal(fixture_replay(preset, iterative=False)[1]["counts"], counts)


def test_replay_partition_and_continuation():
    """Three ranks decide their own tiles: the same counts; and a finished frame continued with min_spp = 0 and a later
    first_sample only ever adds to tiles that were capped."""
    fx = ar.FIXTURE
    rp, out = fixture_replay("CORNELL")
    osc = util.oracle_scene(prt.Scene("CORNELL"))
    cam = prt.Camera(position=fx["cam_pos"], width=fx["W"], height=fx["H"]).desc()
    frame = functools.lru_cache(maxsize=None)(lambda s: osc.render(cam, fx["W"], fx["H"], spp=1, first_sample=s, max_depth=fx["depth"],
                                                                    seed=fx["seed"], iterative=True, n_threads=8)[0])
    rp3 = ar.Replay(fx["W"], fx["H"], frame)
    out3 = rp3.run(fx["min_spp"], fx["step_spp"], fx["max_spp"], 0.10, fx["noise_floor"], ranks=3)
    assert np.array_equal(out3["counts"], out["counts"]) and np.array_equal(rp3.accum, rp.accum)
    assert [I["tiles_local"] for I in out3["per_rank"]] == [8, 8, 8]
    assert out3["info"]["pixel_samples"] == out["info"]["pixel_samples"]
    more = rp3.run(0, 8, 16, 0.10, fx["noise_floor"], first_sample=96)
    assert (more["counts"][out["counts"] < 96] == 0).all() and more["counts"].max() == 16


@functools.lru_cache(maxsize=None)
def wide_replay(ranks=1):
    fx = ar.FIXTURE_WIDE
    osc = util.oracle_scene(prt.Scene(fx["preset"]))
    cam = prt.Camera(position=fx["cam_pos"], width=fx["W"], height=fx["H"]).desc()
    frame = functools.lru_cache(maxsize=None)(lambda s: osc.render(cam, fx["W"], fx["H"], spp=1, first_sample=s, max_depth=fx["depth"],
                                                                    seed=fx["seed"], iterative=True, n_threads=16)[0])
    rp = ar.Replay(fx["W"], fx["H"], frame)
    return rp, rp.run(fx["min_spp"], fx["step_spp"], fx["max_spp"], fx["threshold"], fx["noise_floor"], ranks=ranks)


def test_wide_fixture_gate_conditions():
    """FIXTURE_WIDE (444 x 348, 2464 tiles, CORNELL at threshold 0.2, 4 / 4 / 32 samples) is worth running only while its tile
    lists span trips of 1024 flags, shrink, and are ragged.  Conditions on the inputs: should the oracle ever move them,
    choose another fixture.  Measured: 7 passes; selects of 2464, 1858, 1568, 1520, 1511, 1509, 1509, 1509 tiles; 955 tiles
    converged, 1509 at the cap; up to 219 runs of consecutive tiles in a list."""
    fx = ar.FIXTURE_WIDE
    rp, out = wide_replay()
    assert len(rp.tiles) == 56 * 44 == 2464 and fx["W"] % 8 and fx["H"] % 8
    sel = out["selects"][0]
    print("selects", [(n_in, len(kept)) for n_in, kept in sel], "runs", [ar.runs(kept) for _, kept in sel], out["info"])
    assert sel[0][0] == 2464 and all(sel[i + 1][0] == len(sel[i][1]) for i in range(len(sel) - 1))
    assert sum(1 for n_in, kept in sel[1:] if n_in > 1024) >= 3          # a non-null prev and more than one trip
    assert sum(1 for n_in, kept in sel if len(kept) < n_in) >= 3          # the output is smaller than the input
    assert max(ar.runs(kept) for _, kept in sel) >= 100                   # ragged lists
    counts = out["counts"]
    assert len(np.unique(counts)) >= 3                                    # tiles stop at three or more sample counts
    assert (counts == fx["min_spp"]).any() and (counts == fx["max_spp"]).any()
    assert out["margins"].size and out["margins"].min() >= 1e-9          # one rounding in float64 cannot flip a tile
    info = out["info"]
    assert info["passes"] == len(sel) - 1 and info["tiles_converged"] + info["tiles_capped"] == 2464
    assert info["pixel_samples"] == int(rp.n.sum()) and np.array_equal(rp.n, rp.count_map(counts))
    # three ranks decide their own tiles: the same film, each rank's lists past one wave of 64 and ragged
    rp3, out3 = wide_replay(3)
    assert np.array_equal(out3["counts"], counts) and np.array_equal(rp3.accum, rp.accum)
    assert [I["tiles_local"] for I in out3["per_rank"]] == [822, 821, 821]
    assert all(len(s) >= 3 and s[1][0] > 64 for s in out3["selects"])
    assert sum(I["pixel_samples"] for I in out3["per_rank"]) == info["pixel_samples"]
