"""The lit cases of tests/test_gpu_batch_instances.py on the CPU (no GPU): the replay of every untextured case alone stays within
the replays' cap on undecidable light samples, so that the GPU test compares (nearly) every pixel sample; and the scenes without
a bound texture are what the texture walker and the plain walker both replay."""
import numpy as np
import pytest

import batch_instance_cases as bc
import environment_replay as er
import lighting_replay as lr
import texture_replay as tr
from util import orc

CASES = [(n, False) for n in bc.LIT_CASES] + [(n, True) for n in bc.ODD_LIT_CASES]


@pytest.mark.parametrize("name,odd", CASES, ids=[n + ("_37x29" if o else "") for n, o in CASES])
def test_untextured_lighting_cases_stay_within_the_replays_unstable_share(name, odd):
    """Undecidable over light samples (and misses, with an environment), as printed, against the cap
    lighting_replay.MAX_UNSTABLE = 0.005:
      C_mis_analytic 0 / 5776    C_nee_mesh 0 / 5740    C_mis_env 1 (share 1.0e-4)       C_nee_mesh_env 1 (1.0e-4)
      D_nee_analytic 0 / 5730    D_mis_mesh 0 / 5694    D_nee_analytic_env 1 (1.0e-4)    D_mis_mesh_env 1 (1.0e-4)
      E_mis_analytic 0 / 3283    E_nee_mesh 0 / 3283    E_mis_env 0 / 3283               E_nee_mesh_env 0 / 3283
    (the light samples do not depend on an albedo: the counts are the textured cases' of tests/test_texture_replay.py); on the
    37 x 29 film: C_mis_analytic 0 / 5300, D_nee_analytic_env 0 / 5239, E_nee_mesh 0 / 2936, D_mis_mesh_env 0 / 5213."""
    c, mode, fn = bc.lit_case(name, odd=odd)
    assert not c["scene"].material_texture
    rep = fn(c, orc.OracleScene(c["scene"].desc()))
    share = er.unstable_share(rep) if "env" in name else lr.unstable_share(rep)
    print(name, (c["W"], c["H"]), "light samples", rep.n_light_samples, "unstable", rep.n_unstable, "share", share)
    assert rep.n_light_samples > 1000
    assert share <= lr.MAX_UNSTABLE
    assert rep.stable.mean() >= 0.995
    if "mesh" in name and "env" not in name:
        print(name, "triangle samples", rep.n_triangle_samples)
        assert rep.n_triangle_samples >= 20      # the triangle lights are sampled


def test_the_texture_walker_walks_an_untextured_scene_like_the_plain_walker():
    """tests/test_gpu_batch_instances.py takes its lighting-off frames of untextured scenes from texture_replay.frame: with no
    material bound to a texture its walker is lighting_replay.walk, record for record."""
    c = bc.scene("D")
    osc = orc.OracleScene(c["scene"].desc())
    pix = np.arange(c["W"] * c["H"])
    samp = np.zeros(len(pix), np.int64)
    a = tr.walk(c["scene"], osc, c["cam"], c["W"], c["H"], c["depth"], tr.SEED, pix, samp, (1, 1, 0.75), True)
    b = lr.walk(c["scene"], osc, c["cam"], c["W"], c["H"], c["depth"], tr.SEED, pix, samp, (1, 1, 0.75), True)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert len(a[0]) == len(b[0]) == c["depth"]
    for va, vb in zip(a[0], b[0]):
        assert np.array_equal(va["path"], vb["path"]) and np.array_equal(va["albedo"], vb["albedo"])
    cam = c["cam"].desc()
    want = osc.render(cam, c["W"], c["H"], spp=1, first_sample=0, max_depth=c["depth"], seed=tr.SEED, iterative=True, use_bvh=True,
                      n_threads=lr.n_threads_default(), sampling=None)
    f = tr.frame(c["scene"], osc, c["cam"], c["W"], c["H"], c["depth"], tr.SEED, 0, 1)
    assert np.array_equal(f[0].view(np.uint32), want[0].view(np.uint32)) and int(f[2].sum()) == want[2]


def test_split_threshold_stops_a_proper_subset_of_the_tiles():
    import adaptive_replay as ar
    c = bc.scene("E")
    osc = orc.OracleScene(c["scene"].desc())
    frames = [tr.frame(c["scene"], osc, c["cam"], c["W"], c["H"], c["depth"], tr.SEED, s, 1)[0] for s in range(12)]
    thr, n_stop, n_go = bc.split_threshold(frames, c["W"], c["H"], 4)
    assert n_stop > 0 and n_go > 0
    rp = ar.Replay(c["W"], c["H"], lambda s: frames[s])
    want = rp.run(4, 4, 12, thr, 0.01)
    print("threshold", thr, "stop", n_stop, "go on", n_go, "counts", np.unique(want["counts"], return_counts=True))
    assert (want["counts"] == 4).sum() == n_stop and (want["counts"] > 4).sum() == n_go
