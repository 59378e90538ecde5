"""Pixel-major path ids on the compact route (DESIGN §2 "Path ids"; csrc/prt_path_id.h).  A batch of compact primary rays with
at least 8 samples numbers its paths pixel * S + sample (prt_set_param("path_id_order", 1)) instead of sample * pixels + pixel
(0, and every other batch under either setting).  Only the numbering inside a batch changes: seeds, rays, the order in which a
pixel's samples are added to the film and the ray counts do not, so everything here is byte for byte: between the two settings,
against the oracle, and along the life of one context that reuses its primary stage, changes its batch size and switches the
order, against a context that does none of that.

Scenes: the bundled icosahedron refined to 2 k triangles, and the 30 k bunny, each on the ground quad under the emissive quad.
37 x 29 pixels = 5 x 4 tiles with partial tiles on both edges (1,280 local pixels: five k_raygen blocks, several k_accumulate
lanes outside the image); S = 8 (the smallest eligible batch), 64 (one sample group), 70 (a partial last group of 6: sample-major
slots under the batch's ids), 130 (two full groups and a partial one of 2), and 200 x 120 with S = 256 (6.1 M paths)."""
import functools

import numpy as np
import pytest

import util
from util import prt

pytestmark = pytest.mark.gpu

DEPTH, SEED = 5, 8
CAM_POS = (2.0, 1.5, 3.0)
STAGES = ("raygen", "shade0", "shade", "accumulate")
COMPACT_NAMES = ("k_raygen<false, false, false, true>", "k_shade<0, false, false, false, true>", "k_shade<0, false, false, false, false>",
                 "k_accumulate")


@functools.lru_cache(maxsize=None)
def _scene(name):
    mesh = prt.scenes.refined("icosahedron.ply", 2000) if name == "icosahedron" else prt.scenes.refined("bunny.ply", 30_000)
    return prt.scenes.mesh_scene(mesh)


def _cam(W, H):
    return prt.Camera(position=CAM_POS, width=W, height=H)


def _renderer(scene, W, H, S, order, params=(), setup=None, depth=DEPTH, **kw):
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=SEED, **kw)
    r.Init(prt.Film(W, H), _scene(scene), _cam(W, H))
    r.set_samples_in_flight(S)
    for k, v in params:
        r.set_param(k, v)
    if setup:
        setup(r)
    r.set_param("path_id_order", order)
    return r


def _state(r):
    r.download()
    st = r.stats()
    return (r.film.accum.tobytes(), r.film.weights.tobytes(), [int(x) for x in st.rays_per_depth], int(st.rays_total),
            tuple(r.batch_instances()[s] for s in STAGES))


def _render(scene, W, H, S, order, **kw):
    r = _renderer(scene, W, H, S, order, **kw)
    r.ProgressiveRender(S)
    return _state(r)


# (a) film and ray counts do not depend on the order
@pytest.mark.parametrize("scene,W,H,S", [("icosahedron", 37, 29, 8), ("icosahedron", 37, 29, 64), ("icosahedron", 37, 29, 70),
                                         ("icosahedron", 37, 29, 130), ("bunny", 37, 29, 70), ("bunny", 200, 120, 256)])
def test_film_and_ray_counts_equal_between_the_orders(scene, W, H, S):
    a, b = _render(scene, W, H, S, 0), _render(scene, W, H, S, 1)
    assert a[0] == b[0] and a[1] == b[1], "films differ"
    assert a[2] == b[2] and a[3] == b[3], (a[2:4], b[2:4])
    assert a[2][0] == S * W * H and np.frombuffer(a[0], np.float32).any()
    assert a[4] == b[4] == COMPACT_NAMES  # the eligible route, and the same instances under either order


# (up to 8 segments the pixel-major accumulate counts the paths' last segment indices per lane, beyond that by wave ballots as
# k_accumulate does: 8 is the last depth of the one, 9 and 12 take the other)
@pytest.mark.parametrize("depth", [1, 8, 9, 12])
def test_ray_counts_at_other_depths(depth):
    W, H, S = 37, 29, 70
    a, b = (_render("icosahedron", W, H, S, order, depth=depth) for order in (0, 1))
    assert a[:4] == b[:4]
    assert a[2][0] == S * W * H and not any(a[2][depth:]) and (depth == 1 or a[2][depth - 1] > 0)


# (the accumulate instance with film statistics is on the compact route too: k_accumulate_stat<false, false>)
def test_film_statistics_equal_between_the_orders():
    W, H, S = 37, 29, 70
    got = []
    for order in (0, 1):
        r = _renderer("icosahedron", W, H, S, order, setup=lambda r: r.set_film_statistics(True))
        r.ProgressiveRender(S)
        got.append(_state(r) + tuple(m.tobytes() for m in r.film_statistics()))
    assert got[0] == got[1]
    assert got[0][4] == COMPACT_NAMES[:3] + ("k_accumulate_stat<false, false>",)
    assert np.frombuffer(got[0][6], np.float32).any()


# (b) three ranks' tile maps on one device: 7 tiles for ranks 0 and 1, 6 for rank 2, partial tiles in each
def test_tiled_over_ranks():
    W, H, S = 37, 29, 70
    whole = _render("icosahedron", W, H, S, 0)
    a1 = np.frombuffer(whole[0], np.float32).reshape(H, W, -1)
    w1 = np.frombuffer(whole[1], np.float32).reshape(H, W)
    covered = np.zeros((H, W), bool)
    per_depth = [0] * len(whole[2])
    for rank in range(3):
        a, b = (_render("icosahedron", W, H, S, order, rank=rank, world_size=3) for order in (0, 1))
        assert a == b
        acc = np.frombuffer(b[0], np.float32).reshape(H, W, -1)
        w = np.frombuffer(b[1], np.float32).reshape(H, W)
        mine = w > 0
        assert mine.any() and not (covered & mine).any()
        assert np.array_equal(acc[mine], a1[mine]) and np.array_equal(w[mine], w1[mine]) and not acc[~mine].any()
        covered |= mine
        per_depth = [x + y for x, y in zip(per_depth, b[2])]
    assert covered.all() and per_depth == whole[2]


# (c) against the oracle, bit for bit as the big-batch parity tests compare (test_gpu_primary_walk.py)
def test_pixel_major_batch_equals_the_oracle():
    W, H, S = 37, 29, 70
    osc = util.oracle_scene(_scene("icosahedron"))
    acc, wts, rays = osc.render(_cam(W, H).desc(), W, H, spp=S, max_depth=DEPTH, seed=SEED, iterative=True, use_bvh=True, n_threads=8)
    got = _render("icosahedron", W, H, S, 1)
    assert got[0] == acc.tobytes() and got[1] == wts.tobytes() and got[3] == rays


# (d) one long-lived context with a still camera: reuse of the kept primary stage, another batch size, an instrumented batch,
# the order switched, a one-sample call; the film after every batch is that of a context that never reuses and never switches
def test_long_lived_context():
    W, H = 37, 29
    r = _renderer("bunny", W, H, 64, 1)
    ref = _renderer("bunny", W, H, 64, 0, params=(("primary_reuse", 0),))

    def batch(S, what):
        for x in (r, ref):
            x.set_samples_in_flight(S)
            x.ProgressiveRender(S)
        a, b = _state(r), _state(ref)
        assert a[0] == b[0] and a[1] == b[1], what
        assert a[2] == b[2] and a[3] == b[3], what

    batch(64, "the first batch builds the stage")
    assert r.primary_reuse() == (0, 0)
    batch(64, "the second batch starts from the kept pixel-major ids")
    assert r.primary_reuse() == (1, 1)
    batch(70, "another batch size: ids of another S")
    assert r.primary_reuse() == (0, 1)
    r.measure_traversal()  # an instrumented batch of its own size; adds nothing to the film
    batch(70, "after measure_traversal")
    assert r.primary_reuse() == (0, 1)
    r.set_param("path_id_order", 0)
    batch(64, "the order switched: sample-major ids, nothing kept is used")
    assert r.primary_reuse() == (0, 1)
    batch(64, "and kept again")
    assert r.primary_reuse() == (1, 2)
    batch(1, "a one-sample call")
    assert ref.primary_reuse() == (0, 0)


# (e) batches that are not eligible render the same film under setting 1 and launch the instances they always did
@pytest.mark.parametrize("name,setup,params,S", [
    ("jitter", lambda r: r.set_sampling(jitter=1), (), 70),
    ("lens", lambda r: r.set_lens(aperture=0.05, focus_distance=3.0), (), 70),
    ("clamp", lambda r: r.set_sampling(clamp=4.0), (), 70),
    ("full records", None, (("compact_primary", 0),), 70),
    ("few samples", None, (), 7),
])
def test_ineligible_batches_do_not_change(name, setup, params, S):
    W, H = 37, 29
    a, b = (_render("icosahedron", W, H, S, order, params=params, setup=setup) for order in (0, 1))
    assert a == b
    assert (a[4] == COMPACT_NAMES) == (name == "few samples")  # (compact, but sample-major slots and ids)
    assert np.frombuffer(a[0], np.float32).any()
