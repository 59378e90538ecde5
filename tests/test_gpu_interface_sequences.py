"""One long-lived context through the whole interface, against the oracle (tests/interface_sequences.py holds the model).

tests/test_gpu_primary_reuse.py shows that every SETTER makes the next batch rebuild the held primary stage.  The other half of
the argument is that no entry point that is NOT a setter writes where the stage lives (d_pix, bounce 0's words of d_counts,
d_prim_pid / d_prim_list / d_prim_hit) although the queries share rb[0], d_work, d_counts, the spill buffer and the scratch with
a batch, and a large query frees and reallocates the path state between two batches.  Here a query stands between every two
batches that reuse, and each film is the oracle's:

Scene and shapes are those of tests/test_gpu_primary_reuse.py: the bundled icosahedron refined to 2 k triangles on the ground
quad under the emissive quad, films 40 x 24 and 67 x 35, max_depth 5, S = 1, 3, 64, 70.  Per (film, S) on ONE context: render S
twice, then for every interposed call: the call, its answer against its reference, render S.  After EVERY render film.accum and
film.weights equal the oracle's accumulation byte for byte (use_bvh=True), stats().rays_total equals the oracle's count, and
prt_primary_reuse says what the model says: 1 wherever no setter intervened (a spurious rebuild would go unnoticed otherwise),
0 after radiance_chunk (a prt_set_param) and after a measurement (an instrumented batch), 1 again on the batch after that; the
count of reused batches moves by exactly the batches the model marks.

None of the interposed calls bumps a generation (checked against csrc/prt_api.cpp: touch_scene / touch_camera are called by
prt_set_scene, prt_clone_scene, prt_refit_meshes, prt_set_instance_transforms, prt_set_camera, prt_set_lens, prt_set_film,
prt_set_film_statistics when the value changes, prt_set_sampling, prt_set_lighting, prt_set_light_sources,
prt_set_light_selection, prt_set_environment, prt_set_textures, prt_set_stream, prt_set_param, prt_set_variant and by whatever
fills the device scene anew; by no query, no read-back and not by prt_film_clear or prt_reset_stats).

References of the interposed calls: the oracle where it has the operation (closest_hit, trace, camera_rays, scatter_batch,
tonemap within its one lsb, the features from its closest hit); for denoise, temporal_step, the film statistics, the noise map
and tile_select the bytes of the same call on a TWIN: a context of its own that reaches the same film by its own renders with
primary_reuse 0 and no interposed query.  test_twins_agree establishes first that two such contexts agree with each other."""
import numpy as np
import pytest

import util  # noqa: F401  (puts the repository root on sys.path)
import fuzz_parity as fuzz
import interface_sequences as iseq
from interface_sequences import MUST, MUST_NOT
from util import prt

pytestmark = pytest.mark.gpu

DEPTH, SEED = iseq.DEPTH, iseq.SEED
# interposed calls that the oracle answers: (name, kind of fuzz.interface_query, rays; None: S * n_pix_local + 1000, more than the
# paths in flight, so that the path state regrows under the held stage)
RAY_QUERIES = [("camera_rays", "camera_rays", 257), ("closest_hit", "closest_hit", 257), ("closest_hit, regrowing", "closest_hit", None),
               ("closest_hit_device", "closest_hit_device", 257), ("occluded", "occluded", 1031), ("radiance", "radiance", 257),
               ("radiance, chunked", "radiance_chunked", 129), ("scatter", "scatter", 257), ("render_features", "render_features", 0)]
FILM_QUERIES = [("UpdateDisplay", "display", 0), ("download", "download", 0), ("stats / reset_stats", "stats", 0),
                ("kernel_occupancy", "occupancy", 0), ("bvh_read8", "bvh_read8", 0)]
MEASUREMENTS = [("measure_traversal", "measure_traversal", 0), ("measure_shade_divergence", "measure_shade_divergence", 0)]
# what the model must say of the batches after a call (the render right after it, the one after that)
AFTER = {"radiance_chunked": (MUST_NOT, MUST), "measure_traversal": (MUST_NOT, MUST), "measure_shade_divergence": (MUST_NOT, MUST)}


class Context:
    """One renderer and the model beside it; every render is held to the oracle and to the model's verdicts."""

    def __init__(self, W, H, S, scene=None, kind="directed", use_bvh=True, rank=0, world=1, reuse=1, model=True):
        scene = iseq.directed_scene() if scene is None else scene
        cam = iseq.camera(W, H, iseq.CAM_POS)
        self.r = prt.HipWavefrontRenderer(device=0, max_depth=DEPTH, seed=SEED, rank=rank, world_size=world)
        self.r.Init(prt.Film(W, H), scene, cam)
        self.r.set_samples_in_flight(S)
        self.S = S
        self.reused = 0
        self.m = None
        if not reuse:
            self.r.set_param("primary_reuse", 0)
        if model:
            self.m = iseq.Model(DEPTH, SEED)
            self.m.init(scene, kind, W, H, cam, use_bvh=use_bvh)
            self.m.set_samples_in_flight(S)

    def check_reuse(self, recs, what):
        """prt_primary_reuse after a call that ran the batches `recs`: the last batch's flag and the count of reused batches."""
        active, total = self.r.primary_reuse()
        must = sum(b["verdict"] == MUST for b in recs)
        free = sum(b["verdict"] == iseq.EITHER for b in recs)
        assert must <= total - self.reused <= must + free, (what, total - self.reused, [b["verdict"] for b in recs])
        self.reused = total
        if recs[-1]["verdict"] != iseq.EITHER:
            assert active == (1 if recs[-1]["verdict"] == MUST else 0), (what, active, recs[-1])

    def render(self, what, expect=None, k=None):
        r, m = self.r, self.m
        r.ProgressiveRender(k or self.S)
        recs = m.render(k or self.S)
        if expect is not None:
            assert [b["verdict"] for b in recs] == [expect], (what, recs)
        f = r.download()
        assert f.accum.tobytes() == m.acc.tobytes(), (what, int((f.accum != m.acc).any(axis=-1).sum()), "pixels differ from the oracle's")
        assert f.weights.tobytes() == m.wts.tobytes(), what
        assert int(r.stats().rays_total) == m.rays, (what, int(r.stats().rays_total), m.rays)
        self.check_reuse(recs, what)

    def query(self, name, kind, n):
        if n is None:
            n = self.S * self.r.local_tile_count() * 64 + 1000
        assert fuzz.interface_query(self.r, self.m, kind, n, rseed=len(name) + 7 * self.S) == [], name

    def clear(self):
        self.r.film.Clear()
        self.r.frame_index = 0
        self.m.clear()


def interpose(c, calls):
    for name, kind, n in calls:
        c.query(name, kind, n)
        for verdict in AFTER.get(kind, (MUST,)):
            c.render(f"after {name}", expect=verdict)


@pytest.mark.parametrize("S", iseq.BATCHES)
@pytest.mark.parametrize("W,H", iseq.FILMS)
def test_queries_between_batches_that_reuse(W, H, S):
    c = Context(W, H, S)
    c.render("first", expect=MUST_NOT)
    c.render("second", expect=MUST)
    interpose(c, RAY_QUERIES + FILM_QUERIES)
    c.clear()
    c.render("after film.Clear()", expect=MUST)
    interpose(c, MEASUREMENTS)
    assert c.reused == sum(b["verdict"] == MUST for b in c.m.log) > len(RAY_QUERIES + FILM_QUERIES)


@pytest.mark.parametrize("S", iseq.BATCHES)
@pytest.mark.parametrize("W,H", iseq.FILMS)
def test_setters_the_oracle_covers_between_queries(W, H, S):
    """Refit to a displaced mesh and back, SetCamera, max_depth, set_film, each with a query on either side: the batch after
    the setter rebuilds and its film is the oracle's of the NEW scene, camera, depth or film; the one after that reuses."""
    c = Context(W, H, S)
    c.render("first", expect=MUST_NOT)
    c.render("second", expect=MUST)

    def refit(displaced):
        scene = iseq.directed_scene(displaced=displaced)
        c.r.Refit(scene)
        c.m.refit(scene)

    def set_camera():
        cam = iseq.camera(c.m.W, c.m.H, (1.5, 1.0, 3.2))
        c.r.SetCamera(cam)
        c.m.set_camera(cam)

    def max_depth():
        c.r.max_depth = 4
        c.m.set_max_depth(4)

    def set_film():
        c.r.set_film(prt.Film(W + 9, H + 5))
        c.m.set_film(W + 9, H + 5)
        c.r.SetCamera(c.m.cam)

    for name, setter in (("Refit", lambda: refit(True)), ("Refit back", lambda: refit(False)), ("SetCamera", set_camera),
                         ("max_depth", max_depth), ("set_film", set_film)):
        c.query(f"closest_hit before {name}", "closest_hit", 257)
        setter()
        c.query(f"closest_hit after {name}", "closest_hit", 257)   # (of the new scene)
        c.render(f"after {name}", expect=MUST_NOT)
        c.query(f"radiance after {name}", "radiance", 129)
        c.render(f"the one after {name}", expect=MUST)


def test_a_one_launch_batch_between_two_batches_of_equal_size():
    """Found by the random sequences (fuzz_parity --interface, seed 1, case 158): with path_kernel set, a one-sample batch runs as
    ONE launch of the PATH instance, which returns before the held stage is looked at; the two-sample batch after it starts from
    the stage of the two-sample batch BEFORE it.  That is sound as long as the PATH launch writes nowhere the stage lives: the
    films say so.  (The model calls those batches "either": the route is the planner's business.)"""
    c = Context(40, 24, 2)
    c.r.set_param("path_kernel", 1)
    c.m.set_param("path_kernel", 1)
    for k in (2, 3, 2, 1, 1, 2, 5, 2):     # 2 | 2 + 1 | 2 | 1 | 1 | 2 | 2 + 2 + 1 | 2
        c.query(f"closest_hit before {k}", "closest_hit", 257)
        c.render(f"render {k}", k=k)
    assert iseq.EITHER in [b["verdict"] for b in c.m.log]


def _twin_calls(r):
    """The calls that only a twin can answer, on r's current film: name -> arrays."""
    n = r.download().weights.copy()
    sum_y, sum_y2 = r.film_statistics()
    lst, count, pixels = r.tile_select(n, sum_y, sum_y2, 0.05, 0.01)
    den, var = r.denoise(return_variance=True)
    tmp, tvar, hist = r.temporal_step(return_variance=True, return_history=True, denoise={})
    feats = r.render_features()
    return {"film_statistics": (sum_y, sum_y2), "noise_map": (r.noise_map(0.01),), "tile_select": (lst, np.array([count, pixels])),
            "denoise": (den, var), "temporal_step": (tmp, tvar, hist), "render_features": tuple(feats[k] for k in sorted(feats) if isinstance(feats[k], np.ndarray))}


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == len(b)


def _twin(W, H, S):
    t = Context(W, H, S, reuse=0, model=False)
    t.r.set_film_statistics(True)
    return t


def test_twins_agree():
    """Two fresh contexts under the same renders give the same bytes for every call that has no oracle, twice in a row (the
    temporal step carries its history from the first round into the second)."""
    W, H, S = 67, 35, 3
    a, b = _twin(W, H, S), _twin(W, H, S)
    for rnd in range(2):
        for t in (a, b):
            t.r.ProgressiveRender(S)
        ra, rb = _twin_calls(a.r), _twin_calls(b.r)
        for name in ra:
            assert _same(ra[name], rb[name]), (rnd, name)
        assert np.isfinite(ra["denoise"][0]).all() and ra["denoise"][0].any() and ra["film_statistics"][1].any()


@pytest.mark.parametrize("S", iseq.BATCHES)
@pytest.mark.parametrize("W,H", iseq.FILMS)
def test_film_calls_between_batches_that_reuse(W, H, S):
    """With film statistics on: film_statistics, noise_map, tile_select, denoise, temporal_step and the features against the
    twin's, then one adaptive pass: its listed batch does not reuse, the next whole-film batch rebuilds, the one after reuses."""
    c, t = Context(W, H, S), _twin(W, H, S)
    c.render("first", expect=MUST_NOT)
    c.r.set_film_statistics(True)
    c.m.set_film_statistics(True)
    c.render("after set_film_statistics", expect=MUST_NOT)
    t.r.ProgressiveRender(S)
    for name in ("film_statistics", "noise_map", "tile_select", "denoise", "temporal_step", "render_features"):
        c.render(f"before {name}", expect=MUST)
        t.r.ProgressiveRender(S)
        got, want = _twin_calls(c.r), _twin_calls(t.r)   # (every call of the set each time: the one named is the one just before the render)
        for k in got:
            assert _same(got[k], want[k]), (name, k)
            c.m.query(k)
        c.render(f"after {name}", expect=MUST)
        t.r.ProgressiveRender(S)
    infos = [x.r.render_adaptive(1e-6, min_spp=S, step_spp=S, max_spp=2 * S, noise_floor=1e-6) for x in (c, t)]
    assert infos[0].passes == 1 and bytes(infos[0]) == bytes(infos[1])
    recs = c.m.adaptive(S, S, 2 * S, 1)
    assert [b["verdict"] for b in recs] == [MUST, MUST_NOT]
    c.check_reuse(recs, "render_adaptive")                 # (the whole-film pass reused, the listed pass did not)
    fc, ft = c.r.download(), t.r.download()
    assert fc.accum.tobytes() == ft.accum.tobytes() and fc.weights.tobytes() == ft.weights.tobytes()
    assert _same(c.r.film_statistics(), t.r.film_statistics())
    c.clear()
    c.r.reset_stats()
    c.m.reset_stats()
    c.render("the whole-film batch after a listed pass", expect=MUST_NOT)
    c.render("the one after it", expect=MUST)


def test_placed_copies_never_reuse_and_stay_the_oracles():
    """Placed copies take the two-level walk: reuse is never offered.  The same queries between the batches; every film against
    the oracle's linear scan (use_bvh=False)."""
    W, H, S = 67, 35, 3
    c = Context(W, H, S, scene=iseq.copies_scene(), kind="copies", use_bvh=False)
    c.render("first")
    c.render("second")
    for name, kind, n in RAY_QUERIES + FILM_QUERIES + MEASUREMENTS:
        c.query(name, kind, n)
        c.render(f"after {name}")
        assert c.r.primary_reuse() == (0, 0), name
    sc = c.m.scene
    sc.SetInstanceTransform(0, translation=(-0.5, 0.2, 0.0))
    c.r.UpdateInstances(sc)
    c.m.update_instances(sc)
    c.query("closest_hit after the move", "closest_hit", 257)
    c.render("after UpdateInstances")
    assert c.r.primary_reuse() == (0, 0)


@pytest.mark.parametrize("S", [3, 70])
def test_three_ranks_on_one_device_with_queries_on_rank_one(S):
    """A tile map of three ranks (rank=, world_size=3) on one device; the queries go to rank 1 only.  After every round each
    rank's owned pixels equal the one-rank oracle film, the ranks' ray counts add up to the oracle's, and every rank reuses."""
    W, H = 67, 35
    whole = iseq.Model(DEPTH, SEED)
    whole.init(iseq.directed_scene(), "directed", W, H, iseq.camera(W, H, iseq.CAM_POS), use_bvh=True)
    whole.set_samples_in_flight(S)
    ranks = [Context(W, H, S, rank=k, world=3, model=False) for k in range(3)]
    ranks[1].m = whole

    def round_(what, expect_rank1):
        for x in ranks:
            x.r.ProgressiveRender(S)
        recs = whole.render(S)
        assert recs[-1]["verdict"] == expect_rank1, (what, recs)
        covered = np.zeros((H, W), bool)
        rays = 0
        for k, x in enumerate(ranks):
            f = x.r.download()
            mine = f.weights > 0
            assert mine.any() and not (covered & mine).any()
            assert f.accum[mine].tobytes() == whole.acc[mine].tobytes() and f.weights[mine].tobytes() == whole.wts[mine].tobytes(), (what, k)
            covered |= mine
            rays += int(x.r.stats().rays_total)
            want = (expect_rank1 == MUST) if k == 1 else (len(whole.log) > 1)
            assert x.r.primary_reuse()[0] == (1 if want else 0), (what, k)
        assert covered.all() and rays == whole.rays, (what, rays, whole.rays)

    round_("first", MUST_NOT)
    round_("second", MUST)
    for name, kind, n in RAY_QUERIES:
        ranks[1].query(name, kind, n)
        for verdict in AFTER.get(kind, (MUST,)):
            round_(f"after {name}", verdict)
