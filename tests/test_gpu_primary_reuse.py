"""A still camera's primary stage kept across batches and calls (DESIGN §2 "One walk per pixel"; csrc/prt_primary_cache.h).
Without jitter and without a lens what a batch computes before its first k_shade does not depend on the sample index or the
seed, so a batch whose key equals the held one skips k_raygen, the bounce-0 walk and k_primary_hit.  The film must not know:
two contexts get the same call sequence, one with prt_set_param("primary_reuse", 1) and one with 0, and after EVERY call they
agree on the film (accum and weights as prt_film_read un-tiles film_local, byte for byte), on the per-depth ray counts and
rays_total, and on the prt_batch_instance names of every stage; the query (prt_primary_reuse) says which batches reused.

Scene: the bundled icosahedron refined to 2 k triangles on the ground quad under the emissive quad.  Films 40 x 24 and 67 x 35
(partial tiles on both edges; n_pix_local is a multiple of 64 by construction of the tile map, the image is not), max_depth 5,
S = 1 (a one-sample batch: no list, no hit records), 3 (sample-major slots), 64 (one k_raygen sample group), 70 (two groups).

primary_walk = 0 (one walk per sample): reuse is NOT offered to multi-sample batches (their hits are per path slot, n_paths of
them); a one-sample batch is the same route under either setting and reuses."""
import functools

import numpy as np
import pytest

import util
from util import prt

pytestmark = pytest.mark.gpu

DEPTH, SEED = 5, 8
FILMS = [(40, 24), (67, 35)]
BATCHES = [1, 3, 64, 70]
CAM_POS = (2.0, 1.5, 3.0)
STAGES = ("raygen", "shade0", "shade", "accumulate")


@functools.lru_cache(maxsize=None)
def _mesh():
    return prt.scenes.refined("icosahedron.ply", 2000)


def _scene():
    return prt.scenes.mesh_scene(_mesh())


@functools.lru_cache(maxsize=None)
def _moved_mesh():
    base = _mesh()
    v = base.GetVertices().copy()
    v[:, 0] += np.float32(0.05) * np.sin(np.float32(3.0) * v[:, 1])
    return prt.Mesh(vertices=v, normals=base.GetNormals(), indices=base.GetIndices())


def _cam(W, H, pos=CAM_POS):
    return prt.Camera(position=pos, width=W, height=H)


class Pair:
    """Two renderers on the one GPU under the same calls: [0] keeps the primary stage, [1] rebuilds it in every batch."""

    def __init__(self, W, H, S, scene=None, rank=0, world=1, params=()):
        self.rs = []
        for reuse in (1, 0):
            r = prt.HipWavefrontRenderer(device=0, max_depth=DEPTH, seed=SEED, rank=rank, world_size=world)
            r.Init(prt.Film(W, H), scene if scene is not None else _scene(), _cam(W, H))
            r.set_samples_in_flight(S)
            for k, v in params:
                r.set_param(k, v)
            r.set_param("primary_reuse", reuse)
            self.rs.append(r)

    def both(self, fn):
        return [fn(r) for r in self.rs]

    def state(self, r):
        r.download()
        st = r.stats()
        return (r.film.accum.tobytes(), r.film.weights.tobytes(), [int(x) for x in st.rays_per_depth], int(st.rays_total),
                tuple(r.batch_instances()[s] for s in STAGES))

    def check(self):
        a, b = self.both(self.state)
        assert a[0] == b[0] and a[1] == b[1], "films differ"
        assert a[2] == b[2] and a[3] == b[3], (a[2:4], b[2:4])
        assert a[4] == b[4], (a[4], b[4])
        assert self.rs[1].primary_reuse() == (0, 0)  # the switch is off there
        return a

    def render(self, spp):
        self.both(lambda r: r.ProgressiveRender(spp))
        return self.check()

    def reused(self):
        return self.rs[0].primary_reuse()[1]

    def active(self):
        return self.rs[0].primary_reuse()[0]


# (a) six equal calls: the first builds the stage, the other five start at their first k_shade
@pytest.mark.parametrize("S", BATCHES)
@pytest.mark.parametrize("W,H", FILMS)
def test_six_equal_calls_reuse_five_times(W, H, S):
    p = Pair(W, H, S)
    for call in range(6):
        p.render(S)
        assert p.reused() == call and p.active() == (1 if call else 0)
    assert p.rs[0].primary_reuse() == (1, 5)


# (b) one call split by samples_in_flight: the later batches of the same call reuse; a shorter last batch has a key of its own
@pytest.mark.parametrize("W,H", FILMS)
def test_batches_of_one_call(W, H):
    p = Pair(W, H, 3)
    p.render(9)  # 3 + 3 + 3
    assert p.reused() == 2 and p.active() == 1
    p.render(10)  # 3 + 3 + 3 + 1: the first three reuse, the one-sample batch rebuilds
    assert p.reused() == 5 and p.active() == 0
    p.render(7)  # 3 (after the one-sample batch: rebuilt) + 3 + 1
    assert p.reused() == 6 and p.active() == 0


def _env_image():
    rng = np.random.default_rng(3)
    return (rng.uniform(0.1, 1.0, size=(8, 16, 3))).astype(np.float32)


# (c) what must make the next batch rebuild the stage.  Each entry: (name, the change applied to both renderers, whether the
# batches that follow are eligible at all).  After the change the next call must not reuse; the one after must, where eligible.
def _changes(W, H, S):
    S2 = 5 if S != 5 else 6
    return [
        ("camera moved", lambda r: r.SetCamera(_cam(W, H, (1.5, 1.0, 3.2))), True, S),
        ("mesh refit", lambda r: r.Refit(prt.scenes.mesh_scene(_moved_mesh())), True, S),
        ("jitter on", lambda r: r.set_sampling(jitter=1), False, S),
        ("jitter off", lambda r: r.set_sampling(jitter=0), True, S),
        ("lens on", lambda r: r.set_lens(aperture=0.05, focus_distance=3.0), False, S),
        ("lens off", lambda r: r.set_lens(), True, S),
        ("S changed", lambda r: r.set_samples_in_flight(S2), True, S2),
        ("S back", lambda r: r.set_samples_in_flight(S), True, S),
        ("max_depth changed", lambda r: setattr(r, "max_depth", 4), True, S),
        ("film resized", lambda r: r.set_film(prt.Film(W + 9, H + 5)), True, S),
        ("environment set", lambda r: r.set_environment(_env_image()), False, S),
        ("environment removed", lambda r: r.set_environment(None), True, S),
        ("a set_param call", lambda r: r.set_param("exact_grids", 2), True, S),  # (and the exact-grid route from here on)
        ("measure_traversal", lambda r: r.measure_traversal(), True, S),
        ("film statistics on", lambda r: r.set_film_statistics(True), True, S),
        ("an adaptive pass with a tile list", "adaptive", True, S),
        ("film statistics off", lambda r: r.set_film_statistics(False), True, S),
    ]


@pytest.mark.parametrize("S", BATCHES)
@pytest.mark.parametrize("W,H", FILMS)
def test_every_change_rebuilds_once(W, H, S):
    p = Pair(W, H, S)
    p.render(S)
    p.render(S)
    assert p.reused() == 1
    for name, change, eligible, spp in _changes(W, H, S):
        if change == "adaptive":
            infos = p.both(lambda r: r.render_adaptive(1e-6, min_spp=spp, step_spp=spp, max_spp=2 * spp, noise_floor=1e-6))
            assert all(i.passes >= 1 for i in infos), name  # a listed pass ran: k_raygen_list overwrote the counters
            p.check()
        else:
            p.both(change)
        before = p.reused()
        p.render(spp)
        assert p.reused() == before and p.active() == 0, name
        p.render(spp)
        assert p.reused() == before + (1 if eligible else 0) and p.active() == (1 if eligible else 0), name


def test_instance_motion_never_reuses():
    """Placed copies take the two-level walk, which has no compact primary rays: nothing is kept, before or after a move."""
    def scene(dx):
        sc = prt.Scene(preset=None)
        ground = sc.AddLambertian((0.5, 0.5, 0.5))
        light = sc.AddEmissive((15.0, 15.0, 15.0))
        body = sc.AddLambertian((0.8, 0.8, 0.8))
        sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
        sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
        sc.AddInstance(_mesh(), body, translation=(-0.8 + dx, 0.0, 0.0))
        sc.AddInstance(_mesh(), body, scale=0.7, translation=(0.9, 0.0, 0.3 - dx))
        return sc
    sc = scene(0.0)
    p = Pair(67, 35, 3, scene=sc)
    first = p.render(3)
    p.render(3)
    sc.SetInstanceTransform(0, translation=(-0.5, 0.2, 0.0))
    p.both(lambda r: r.UpdateInstances(sc))
    moved = p.render(3)
    p.render(3)
    assert p.reused() == 0 and moved[0] != first[0]


# (d) three ranks' tile maps on one device
@pytest.mark.parametrize("S", [3, 70])
def test_tiled_over_ranks(S):
    W, H = 67, 35
    whole = Pair(W, H, S)
    for _ in range(3):
        ref = whole.render(S)
    a1 = np.frombuffer(ref[0], np.float32).reshape(H, W, -1)
    w1 = np.frombuffer(ref[1], np.float32).reshape(H, W)
    covered = np.zeros((H, W), bool)
    for rank in range(3):
        p = Pair(W, H, S, rank=rank, world=3)
        for _ in range(3):
            got = p.render(S)
        assert p.rs[0].primary_reuse() == (1, 2)
        a = np.frombuffer(got[0], np.float32).reshape(H, W, -1)
        w = np.frombuffer(got[1], np.float32).reshape(H, W)
        mine = w > 0
        assert mine.any() and not (covered & mine).any()
        assert np.array_equal(a[mine], a1[mine]) and np.array_equal(w[mine], w1[mine])
        covered |= mine
    assert covered.all()


# (e) one walk per sample
@pytest.mark.parametrize("S", [1, 3, 70])
def test_one_walk_per_sample(S):
    W, H = 67, 35
    per_sample = Pair(W, H, S, params=(("primary_walk", 0),))
    per_pixel = Pair(W, H, S)
    for _ in range(3):
        a = per_sample.render(S)
        b = per_pixel.render(S)
        assert a[:4] == b[:4]
    assert per_pixel.reused() == 2
    assert per_sample.reused() == (2 if S == 1 else 0)  # not offered to multi-sample batches (module docstring)


# (f) seed and first_sample differ between calls: they reach the first k_shade as arguments, the stage does not hold them
def test_seed_and_first_sample_change_and_reuse_still_applies():
    W, H, S = 40, 24, 3
    calls = [(8, 0), (9, 100), (8, 7), (1234567, 4000)]
    p = Pair(W, H, S)
    osc = util.oracle_scene(_scene())
    acc = wts = None
    rays = 0
    for k, (seed, first) in enumerate(calls):
        for r in p.rs:
            r.seed, r.frame_index = seed, first
        got = p.render(S)
        assert p.reused() == k
        acc, wts, n = osc.render(_cam(W, H).desc(), W, H, spp=S, first_sample=first, max_depth=DEPTH, seed=seed, iterative=True,
                                 use_bvh=True, n_threads=8, accum=acc, weights=wts)
        rays += n
        assert got[0] == acc.tobytes() and got[1] == wts.tobytes() and got[3] == rays
