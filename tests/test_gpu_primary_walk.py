"""One walk per pixel of the shared primary ray (compact primary rays): without jitter all samples of a pixel
start with the same pixel-centre ray, so bounce 0's traversal runs over a list of front pixels (one ray per pixel) and
the first k_shade / k_primary_hit take a front path's hit from the pixel's list slot.  prt_set_param("primary_walk", 0)
restores one walk per sample.  Everything here is bit for bit: against the oracle, and between the two routes.

Scene: the 30 k bunny on the analytic ground under the analytic light, oblique camera, 52 x 37 pixels (partial 8x8 tiles
on both edges).  The frame holds front pixels that hit a triangle, front pixels that miss the mesh and end on the ground,
front pixels that miss everything, and back pixels (test_the_walk_happens_once_per_front_pixel checks the split)."""
import functools

import numpy as np
import pytest

import util
from util import orc, prt

pytestmark = pytest.mark.gpu

W, H, DEPTH, SEED = 52, 37, 5, 8
CAM_POS = (2.0, 1.5, 3.0)


@functools.lru_cache(maxsize=None)
def _scene():
    mesh = prt.scenes.refined("bunny.ply", 30_000)
    return mesh, prt.scenes.mesh_scene(mesh)


def _cam():
    return prt.Camera(position=CAM_POS, width=W, height=H)


@functools.lru_cache(maxsize=None)
def _oracle(spp):
    """(accum, weights, rays_total) of the oracle after `spp` samples; computed once per sample count, read-only."""
    osc = util.oracle_scene(_scene()[1])
    acc, wts, rays = osc.render(_cam().desc(), W, H, spp=spp, max_depth=DEPTH, seed=SEED, iterative=True, use_bvh=True,
                                n_threads=8)
    for a in (acc, wts):
        a.setflags(write=False)
    return acc, wts, rays


@functools.lru_cache(maxsize=None)
def _oracle_rays_per_depth(spp):
    """The oracle counts a render's segments in total.  Whether a path has a segment of index d does not depend on the
    depth limit as long as the limit is above d (the limit only stops the scatter of the last segment), so the segments of
    index d are the difference of the totals at limits d + 1 and d."""
    osc = util.oracle_scene(_scene()[1])
    totals = [0] + [osc.render(_cam().desc(), W, H, spp=spp, max_depth=k, seed=SEED, iterative=True, use_bvh=True,
                               n_threads=8)[2] for k in range(1, DEPTH)] + [_oracle(spp)[2]]
    return [totals[k + 1] - totals[k] for k in range(DEPTH)]


def _renderer(params=(), max_depth=DEPTH, **kw):
    film = prt.Film(W, H)
    r = prt.HipWavefrontRenderer(device=0, max_depth=max_depth, seed=SEED, **kw)
    r.Init(film, _scene()[1], _cam())
    for k, v in params:
        r.set_param(k, v)
    return r, film


def _render(calls, params=(), **kw):
    r, film = _renderer(params, **kw)
    r.set_samples_in_flight(max(calls))
    for c in calls:
        r.ProgressiveRender(c)
    r.download()
    st = r.stats()
    return film.accum.copy(), film.weights.copy(), int(st.rays_total), [int(x) for x in st.rays_per_depth]


# 1: a one-sample batch; 5: the sample-major branch; 8: the smallest pixel-major batch; 64: exactly one k_raygen sample
# group; 65: a second group of one sample (sample-major store inside a multi-group batch); 130: two full groups + a partial one
@pytest.mark.parametrize("S", [1, 5, 8, 64, 65, 130])
def test_one_batch_equals_the_oracle_bit_for_bit(S):
    acc, wts, rays = _oracle(S)
    a, w, n, per_depth = _render([S])
    assert np.array_equal(a, acc) and np.array_equal(w, wts)
    assert n == rays
    assert per_depth[:DEPTH] == _oracle_rays_per_depth(S) and not any(per_depth[DEPTH:])
    assert per_depth[0] == S * W * H


@pytest.mark.parametrize("extra", [(), (("primary_hit", 0),), (("exact_grids", 2),)], ids=["default", "nopixelhit", "exact"])
@pytest.mark.parametrize("S", [8, 65, 130])
def test_both_routes_agree(S, extra):
    per_sample = _render([S], (("primary_walk", 0),) + extra)
    per_pixel = _render([S], (("primary_walk", 1),) + extra)
    assert per_pixel[0].tobytes() == per_sample[0].tobytes() and per_pixel[1].tobytes() == per_sample[1].tobytes()
    assert per_pixel[2] == per_sample[2] and per_pixel[3] == per_sample[3]
    acc, wts, rays = _oracle(S)
    assert np.array_equal(per_pixel[0], acc) and np.array_equal(per_pixel[1], wts) and per_pixel[2] == rays


def test_tiled_over_ranks():
    """Three contexts (ranks 0-2 of 3) on the one GPU, 65 samples in one batch: each rank's tiles carry the single-rank
    frame's values, no rank touches another's pixels, and together they cover the frame."""
    S = 65
    a1, w1, n1, d1 = _render([S])
    covered = np.zeros((H, W), bool)
    n_rays = 0
    per_depth = [0] * len(d1)
    for rank in range(3):
        a, w, n, d = _render([S], rank=rank, world_size=3)
        mine = w > 0
        assert mine.any() and not (covered & mine).any()
        assert np.array_equal(a[mine], a1[mine]) and np.array_equal(w[mine], w1[mine])
        assert not a[~mine].any()
        covered |= mine
        n_rays += n
        per_depth = [x + y for x, y in zip(per_depth, d)]
    assert covered.all() and n_rays == n1 and per_depth == d1
    acc, wts, rays = _oracle(S)
    assert np.array_equal(a1, acc) and n1 == rays


def test_consecutive_batches():
    """65 + 65 + 1 samples: the list, its counter and the per-pixel records are rebuilt per batch, and the one-sample
    batch after big ones finds blank hit records."""
    acc, wts, rays = _oracle(131)
    a, w, n, _ = _render([65, 65, 1])
    assert np.array_equal(a, acc) and np.array_equal(w, wts) and n == rays


def _pixel_classes():
    """Counts of pixels by what the pixel-centre ray does, from the oracle's closest hits and a float64 slab test against
    the mesh bounds shrunk / grown by 2 % (so that rounding cannot move a pixel across): (hits a triangle, surely enters the
    root box and ends on the ground behind its entry, surely enters it and hits nothing, surely front, surely not front)."""
    mesh, scene = _scene()
    ys, xs = np.mgrid[0:H, 0:W]
    o, d = orc.camera_rays(_cam().desc(), (xs.ravel() + 0.5).astype(np.float32), (ys.ravel() + 0.5).astype(np.float32))
    h = util.oracle_scene(scene).closest_hit(o, d, use_bvh=True)
    V = mesh.GetVertices().astype(np.float64)
    c, e = (V.min(0) + V.max(0)) / 2, (V.max(0) - V.min(0)) / 2

    def enters(lo, hi):
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - o.astype(np.float64)) / d.astype(np.float64), (hi - o.astype(np.float64)) / d.astype(np.float64)
        tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
        return (tn <= tf) & (tf > 0), np.maximum(tn, 0.0)

    inside, t_in = enters(c - 0.98 * e, c + 0.98 * e)
    outside = ~enters(c - 1.02 * e, c + 1.02 * e)[0]
    n_analytic = len(scene.primitives)
    tri, miss = h["prim"] >= n_analytic, h["prim"] < 0
    ground = (h["prim"] >= 0) & ~tri
    behind = np.sqrt(h["d2"].astype(np.float64)) > 1.02 * t_in  # the analytic hit lies beyond the entry into the box
    sure_front = inside & (miss | tri | (ground & behind))
    return int(tri.sum()), int((inside & ground & behind).sum()), int((inside & miss).sum()), int(sure_front.sum()), int(outside.sum())


def test_the_walk_happens_once_per_front_pixel():
    """max_depth 1, one instrumented batch of 64 samples: rays_traversed (the rays handed to the traversal kernel) is the
    number of front pixels F with one walk per pixel and exactly 64 F with one walk per sample, and F splits the frame
    non-trivially: all four pixel classes are present."""
    S = 64
    got = {}
    for walk in (0, 1):
        r, _ = _renderer((("primary_walk", walk), ("measure_spp", S)), max_depth=1)
        st = r.measure_traversal()
        got[walk] = int(st.rays_traversed)
        assert int(st.samples) == S and int(st.rays_total) == S * W * H
    F = got[1]
    assert 0 < F < W * H
    assert got[0] == S * F
    n_tri, n_front_ground, n_front_miss, sure_front, sure_back = _pixel_classes()
    assert n_tri > 0 and n_front_ground > 0 and n_front_miss > 0 and sure_back > 0
    assert sure_front <= F <= W * H - sure_back
