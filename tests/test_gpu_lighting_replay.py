"""Every sample of light-sampled frames against the float64 per-path replay (tests/lighting_replay.py) on one MI355X.

Per case and mode (mis, nee): Init, set_lighting, then per sample index s (0, 1, 2, 5): film Clear, frame_index = s,
ProgressiveRender(1), download.  Every stable pixel sample must lie within its tolerance of the replay (no exceptions), the
shadow-ray and occluded counts must match the replay's to within the number of samples it cannot decide, and light_info()
must give the float64 light set (pmf to 1e-6).  320 x 240, depth 5 to 8.  One case also runs as a 3-rank group on the one
GPU and with 1 and 64 samples in flight.

Cases (lighting_replay.case): DEFAULT (three lights of both kinds, pmf < 1), RANDOM_BALLS_SMALL (8 sphere lights, metal and
dielectric vertices, the primitive-BVH instance), LIGHT_TEST (11 sphere lights), CORNELL (a quad light in an enclosure),
penumbra (a quad light partly behind an analytic sphere and a quad), bunny (a mesh with interpolated normals under a rotated,
scaled quad light and a low sphere light), placed (copies in a two-level tree, one of them an emitter outside the light
set), specular (glass and rough metal between ground and light), resting (a sphere light almost on the ground, seen from
inside the gap: vertices on both sides of its margin), DEFAULT_rr_clamp_jitter (roulette from depth 1, clamp 1.0, jitter).

Measured on the MI355X (no stable sample outside its tolerance anywhere; the whole file 13 s of wall time, of which the
replay on 16 CPU threads is 0.35 to 0.66 s per case and mode and the four one-sample frames at most 0.2 s; shadow-ray counts
equal the replay's exactly except one occluded ray of 24,625 on RANDOM_BALLS_SMALL):

  case                     mode  compared  left out  worst err/tol  shadow rays  occluded   cpu s  gpu s
  DEFAULT                  mis     307184        16         0.0887       221391     24700    0.55   0.21
  DEFAULT                  nee     307184        16         0.0792       221391     24700    0.44   0.01
  RANDOM_BALLS_SMALL       mis     307192         8         0.1002       292422     24625    0.64   0.00
  RANDOM_BALLS_SMALL       nee     307192         8         0.0999       292422     24625    0.66   0.01
  LIGHT_TEST               mis     307198         2         0.0355       231616      1679    0.40   0.00
  LIGHT_TEST               nee     307198         2         0.0329       231616      1679    0.40   0.00
  CORNELL                  mis     307000       200         0.0546       121901         0    0.46   0.00
  CORNELL                  nee     307000       200         0.0544       121901         0    0.46   0.00
  penumbra                 mis     307199         1         0.0661       214235     37132    0.37   0.00
  penumbra                 nee     307199         1         0.0681       214235     37132    0.39   0.00
  bunny                    mis     307176        24         0.0937       193661     18556    0.45   0.01
  bunny                    nee     307176        24         0.0934       193661     18556    0.43   0.01
  placed                   mis     307195         5         0.0559       199297      9453    0.39   0.00
  placed                   nee     307195         5         0.0535       199297      9453    0.37   0.00
  specular                 mis     307199         1         0.0503       197070     74414    0.45   0.00
  specular                 nee     307199         1         0.0534       197070     74414    0.45   0.00
  resting                  mis     307168        32         0.1584       156200         0    0.34   0.00
  resting                  nee     307168        32         0.3639       156200         0    0.35   0.00
  DEFAULT_rr_clamp_jitter  mis     307187        13         0.0969       219717     24921    0.48   0.00
  DEFAULT_rr_clamp_jitter  nee     307187        13         0.1003       219717     24921    0.49   0.00

The routes (placed, mis; 3-rank group, 1 and 64 samples in flight): the same 307,195 samples, worst 0.0559 on each."""
import time

import numpy as np
import pytest

import lighting_replay as lr
from util import orc, prt

pytestmark = pytest.mark.gpu


def _renderer(c, mode, sif=16, group=False):
    film = prt.Film(c["W"], c["H"])
    if group:
        r = prt.HipWavefrontGroupRenderer([0, 0, 0], max_depth=c["depth"], seed=lr.SEED)
    else:
        r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=lr.SEED)
    r.Init(film, c["scene"], c["cam"])
    r.set_samples_in_flight(sif)
    r.set_lighting(mode)
    if c["sampling"] != (0, 0, 0.0):
        r.set_sampling(*c["sampling"])
    return r, film


@pytest.mark.parametrize("name", lr.CASES)
def test_every_sample_matches_the_float64_replay(record_property, name):
    c = lr.case(name)
    osc = orc.OracleScene(c["scene"].desc())
    for mode in ("mis", "nee"):
        t0 = time.time()
        rep = lr.replay_case(c, mode, osc=osc)
        t1 = time.time()
        r, film = _renderer(c, mode)
        r.reset_stats()
        frames = lr.render_samples(r, film, lr.SAMPLES)
        r.synchronize()
        t2 = time.time()
        rec = lr.check_against_gpu(rep, frames, r.light_stats(), r.light_info())
        rec.update(case=name, mode=mode, cpu_s=round(t1 - t0, 2), gpu_s=round(t2 - t1, 2))
        record_property("lighting_replay", rec)
        assert rec["compared"] >= 0.995 * len(rep.pix)
        del r


@pytest.mark.parametrize("route", ["group3", "sif1", "sif64"])
def test_replay_holds_on_other_routes(route):
    c = lr.case("placed")
    rep = lr.replay_case(c, "mis")
    if route == "group3":
        g, film = _renderer(c, "mis", group=True)
        frames = lr.render_samples(g, film, lr.SAMPLES, clear=g.Clear)
        lr.check_against_gpu(rep, frames, g.light_stats(), g.light_info())
    else:
        r, film = _renderer(c, "mis", sif=int(route[3:]))
        r.reset_stats()
        frames = lr.render_samples(r, film, lr.SAMPLES)
        lr.check_against_gpu(rep, frames, r.light_stats(), r.light_info())


def test_samples_add_up_in_sample_order():
    """The film of one 4-sample call is the fp32 sum, in sample order, of the four one-sample frames the replay pins."""
    c = lr.case("penumbra")
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
