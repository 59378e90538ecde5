"""prt_tile_select (include/prt.h): the selection stage of prt_render_adaptive, k_tile_select + k_tile_compact, on
caller-supplied moments, against a few lines of numpy over adaptive_replay.unconverged and adaptive_replay.tiles.  Everything
is integers and booleans, so every comparison is exact.  The films are set with prt_set_film alone (no scene, no render);
their local tile counts sit on both sides of a wave of 64 flags, of k_tile_select's 4-tile blocks and of k_tile_compact's trips
of 1024 flags, where a rank inside a trip, the scan of the 16 wave totals and the carry across trips each decide an entry."""
import functools

import numpy as np
import pytest

import adaptive_replay as ar
from util import prt

pytestmark = pytest.mark.gpu

F = np.float32
CAPI = prt.capi
THR, FLOOR = 0.1, 0.01
N_DONE = F(2.0 ** 20)   # a converged pixel: n = 2^20, A = Q = 0 (V = 0, lhs = 0, and 0 > t^2 is false whatever t)
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
NONE = 0xFFFFFFFF

# local tile count -> (W, H) of a one-rank film; 9 of the 14 have partial tiles on the right and bottom edges
FILMS = {
    1: (5, 3), 63: (67, 51), 64: (64, 64), 65: (100, 37), 255: (136, 120), 256: (125, 123), 257: (2053, 3), 1023: (264, 248),
    1024: (250, 251), 1025: (328, 200), 2047: (707, 181), 2048: (512, 256), 2049: (5459, 20), 5005: (611, 517),
}
# rank 1 of 3: (W, H) -> local tile count.  190 = 3 * 63 + 1 tiles: rank 1 owns 63 and its last slot of the payload is absent;
# 3073 = 3 * 1024 + 1: 1024, absent; 3075 and 770 tiles: the last local tile lies in the partial bottom row (770: the corner);
# 2 tiles: one partial tile; 1 tile: no local tile at all
FILMS_RANK1 = {(147, 75): 63, (3507, 50): 1024, (597, 323): 1025, (275, 171): 257, (11, 5): 1, (8, 8): 0}


class Geometry:
    """The local tiles of rank `rank` of `world` on a W x H film: rects, pixels inside the image, the tile of every pixel."""

    def __init__(self, W, H, rank=0, world=1):
        self.W, self.H, self.rank, self.world = W, H, rank, world
        rects = np.array(ar.tiles(W, H), np.int64)[rank::world].reshape(-1, 4)
        self.x0, self.y0 = rects[:, 0], rects[:, 1]
        self.w, self.h = rects[:, 2] - rects[:, 0], rects[:, 3] - rects[:, 1]
        self.n_local = len(rects)
        self.inside = self.w * self.h
        self.tile_of = np.full((H, W), -1, np.int64)   # local tile index, -1: another rank's
        for lt, (x0, y0, x1, y1) in enumerate(rects):
            self.tile_of[y0:y1, x0:x1] = lt
        film = prt.Film(W, H)
        self.r = prt.HipWavefrontRenderer(device=0, rank=rank, world_size=world)
        self.r.set_film(film)
        assert self.r.local_tile_count() == self.n_local

    def converged_images(self):
        """(n, A, Q) with every owned pixel converged and every other pixel unconverged (those must be ignored)."""
        n = np.where(self.tile_of >= 0, N_DONE, F(0)).astype(F)
        return n, np.zeros((self.H, self.W), F), np.zeros((self.H, self.W), F)

    def reference(self, n, A, Q, prev, thr=THR, floor=FLOOR):
        """(list, count, pixels): a tile is active if any of its pixels inside the image is unconverged; list = prev[active]
        in the order of prev."""
        unc = ar.unconverged(n, A, Q, thr, floor) & (self.tile_of >= 0)
        active = np.bincount(self.tile_of[unc], minlength=self.n_local)[:self.n_local] > 0
        prev = np.arange(self.n_local) if prev is None else np.asarray(prev, np.int64)
        lst = prev[active[prev]]
        return lst, len(lst), int(self.inside[lst].sum()), active

    def check(self, n, A, Q, prev, thr=THR, floor=FLOOR, what=None):
        want, count, pixels, active = self.reference(n, A, Q, prev, thr, floor)
        got, g_count, g_pixels = self.r.tile_select(n, A, Q, thr, floor, prev)
        n_in = self.n_local if prev is None else len(prev)
        assert len(got) == n_in
        assert (g_count, g_pixels) == (count, pixels), (what, (g_count, g_pixels), (count, pixels))
        assert np.array_equal(got[:count], want), (what, np.flatnonzero(got[:count] != want)[:8])
        assert (got[count:] == NONE).all(), what   # nothing is written past the count
        return active


@functools.lru_cache(maxsize=None)
def _geometry(W, H):
    """(shared by the tests of one film: the pixel cases, the rule)"""
    return Geometry(W, H)


def _patterns(n_in, rng):
    """name -> bool[n_in]: which entries of the input list are on."""
    idx = np.arange(n_in)
    out = {"none": idx < 0, "all": idx >= 0}
    for i in sorted({0, 63, 64, 1023, 1024, n_in - 1}):
        if 0 <= i < n_in:
            out["only_%d" % i] = idx == i
    out["lane0_of_every_wave"] = idx % 64 == 0
    out["lane63_of_every_wave"] = idx % 64 == 63
    out["even"] = idx % 2 == 0
    out["odd"] = idx % 2 == 1
    for density in (0.02, 0.5, 0.98):
        out["random_%g" % density] = rng.random(n_in) < density
    return out


UNCONVERGED = [(0, 0, 0), (1, 0.5, 0.25), (16, 8, 8)]   # (n, A, Q): no sample, one sample, samples of 0 and 1 in equal parts


def _images_for(g, on_tiles, rng, whole_tiles=False):
    """Images in which exactly the local tiles `on_tiles` hold an unconverged pixel inside the image: ONE pixel, at a random
    inside position (whole_tiles: all of them)."""
    n, A, Q = g.converged_images()
    on_tiles = np.asarray(on_tiles, np.int64)
    if whole_tiles:
        sel = np.isin(g.tile_of, on_tiles)
        n[sel] = 0
        return n, A, Q
    px = g.x0[on_tiles] + rng.integers(0, 8, len(on_tiles)) % g.w[on_tiles]
    py = g.y0[on_tiles] + rng.integers(0, 8, len(on_tiles)) % g.h[on_tiles]
    kind = np.array(UNCONVERGED, F)[rng.integers(0, len(UNCONVERGED), len(on_tiles))]
    n[py, px], A[py, px], Q[py, px] = kind[:, 0], kind[:, 1], kind[:, 2]
    return n, A, Q


def _prev_modes(g, rng):
    """name -> prev: null, increasing random subsets of edge sizes (the largest below the tile count and one more, drawn),
    and a random permutation (never met in the loop: it pins "in their order" and the prev[i] indirection)."""
    L = g.n_local
    modes = {"null": None}
    below = [s for s in EDGE_SIZES if s < L]
    sizes = {below[-1], int(rng.choice(below))} if below else set()
    for s in sorted(sizes):
        modes["subset_%d" % s] = np.sort(rng.choice(L, s, replace=False)).astype(np.uint32)
    modes["permutation"] = rng.permutation(L).astype(np.uint32)
    return modes


def _run_patterns(g, seed):
    rng = np.random.default_rng(seed)
    seen_on = seen_off = 0
    for mode, prev in _prev_modes(g, rng).items():
        entries = np.arange(g.n_local) if prev is None else prev.astype(np.int64)
        for name, on in _patterns(len(entries), rng).items():
            n, A, Q = _images_for(g, entries[on], rng, whole_tiles=name == "all")
            active = g.check(n, A, Q, prev, what=(mode, name))
            assert np.array_equal(np.flatnonzero(active), np.sort(entries[on])), (mode, name)   # the input is what it says
            seen_on += int(on.sum())
            seen_off += int((~on).sum())
    assert seen_on and seen_off


@pytest.mark.parametrize("tiles", sorted(FILMS))
def test_selection_equals_the_reference(tiles):
    W, H = FILMS[tiles]
    g = Geometry(W, H)
    assert g.n_local == tiles
    _run_patterns(g, seed=tiles)


def test_half_of_the_films_have_partial_tiles_on_both_edges():
    partial = [t for t, (W, H) in FILMS.items() if W % 8 and H % 8]
    assert 2 * len(partial) >= len(FILMS)
    assert set(EDGE_SIZES) <= set(FILMS) and max(FILMS) >= 5000


@pytest.mark.parametrize("film", sorted(FILMS_RANK1))
def test_selection_on_rank_1_of_3(film):
    W, H = film
    g = Geometry(W, H, 1, 3)
    total = ((W + 7) // 8) * ((H + 7) // 8)
    assert g.n_local == FILMS_RANK1[film] and g.n_local != total
    if g.n_local == 0:   # a rank without tiles: an empty list, whatever the images hold
        n, A, Q = g.converged_images()
        got, count, pixels = g.r.tile_select(n, A, Q, THR, FLOOR)
        assert (len(got), count, pixels) == (0, 0, 0)
        return
    last = g.n_local - 1
    absent = g.n_local < (total + 2) // 3           # the rank's payload has a slot more than it has tiles
    assert absent or g.inside[last] < 64, "the last local tile is partial or absent"
    _run_patterns(g, seed=W)


# ---- pixels --------------------------------------------------------------------------------------------------------------------
PW, PH = 107, 93   # 14 x 12 tiles: 13 x 11 whole ones, a right column 3 wide, a bottom row 5 high


def test_one_unconverged_pixel_at_each_of_the_64_positions():
    g = _geometry(PW, PH)
    whole = np.flatnonzero(g.inside == 64)
    assert len(whole) == 13 * 11
    rng = np.random.default_rng(64)
    for kind in UNCONVERGED:
        chosen = np.sort(rng.choice(whole, 64, replace=False))
        n, A, Q = g.converged_images()
        for lane, lt in enumerate(chosen):
            y, x = g.y0[lt] + (lane >> 3), g.x0[lt] + (lane & 7)
            n[y, x], A[y, x], Q[y, x] = kind
        active = g.check(n, A, Q, None, what=kind)
        assert np.array_equal(np.flatnonzero(active), chosen)


def test_partial_tiles_count_only_pixels_inside_the_image():
    g = _geometry(PW, PH)
    partial = np.flatnonzero(g.inside < 64)
    assert sorted(set(g.inside[partial].tolist())) == [15, 24, 40]   # the corner, the right column, the bottom row
    # fully converged, partial tiles included: nothing is selected although the padding lanes are zero (n < 2)
    n, A, Q = g.converged_images()
    got, count, pixels = g.r.tile_select(n, A, Q, THR, FLOOR)
    assert count == 0 and pixels == 0 and (got == NONE).all()
    # the only unconverged pixel of every partial tile is its last pixel inside the image
    for lt in partial:
        n[g.y0[lt] + g.h[lt] - 1, g.x0[lt] + g.w[lt] - 1] = 1
    active = g.check(n, A, Q, None)
    assert np.array_equal(np.flatnonzero(active), partial)
    got, count, pixels = g.r.tile_select(n, A, Q, THR, FLOOR)
    assert count == len(partial) == 14 + 12 - 1 and pixels == int(g.inside[partial].sum()) == 11 * 24 + 13 * 40 + 15
    # ... and one at a time, each kind of partial tile: the flag is the tile's pixels inside the image
    for lt in (13, 14 * 11, 14 * 12 - 1):
        n, A, Q = g.converged_images()
        n[g.y0[lt] + g.h[lt] - 1, g.x0[lt] + g.w[lt] - 1] = 0
        got, count, pixels = g.r.tile_select(n, A, Q, THR, FLOOR)
        assert (count, pixels, int(got[0])) == (1, int(g.inside[lt]), lt)
    # every pixel of the image unconverged: all tiles, W * H pixels
    n[:] = 0
    got, count, pixels = g.r.tile_select(n, A, Q, THR, FLOOR)
    assert count == g.n_local and pixels == PW * PH and np.array_equal(got, np.arange(g.n_local))


def test_the_contexts_film_and_statistics_are_left_alone():
    W, H = ar.FIXTURE["W"], ar.FIXTURE["H"]
    film = prt.Film(W, H)
    r = prt.HipWavefrontRenderer(device=0, max_depth=3, seed=3)
    r.Init(film, prt.Scene("CORNELL"), prt.Camera(position=ar.FIXTURE["cam_pos"], width=W, height=H))
    r.set_film_statistics(True)
    r.ProgressiveRender(4)
    r.download()
    acc, wts = film.accum.copy(), film.weights.copy()
    A, Q = r.film_statistics()
    assert acc.any() and Q.any()
    zeros = np.zeros((H, W), F)
    got, count, pixels = r.tile_select(zeros, zeros, zeros, THR, FLOOR)          # not the film's own moments: all unconverged
    assert count == 24 and pixels == W * H
    got, count, pixels = r.tile_select(zeros + N_DONE, zeros, zeros, THR, FLOOR)  # ... and all converged
    assert count == 0
    want = ar.unconverged(wts, A, Q, THR, FLOOR)                                   # the film's own, handed in
    got, count, pixels = r.tile_select(wts, A, Q, THR, FLOOR)
    assert got[:count].tolist() == [i for i, (x0, y0, x1, y1) in enumerate(ar.tiles(W, H)) if want[y0:y1, x0:x1].any()]
    r.download()
    A2, Q2 = r.film_statistics()
    for a, b in ((film.accum, acc), (film.weights, wts), (A2, A), (Q2, Q)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the rule on the device ---------------------------------------------------------------------------------------------------------
RW, RH = 397, 195   # 50 x 25 = 1250 tiles, one decision each
RULE_CONFIGS = [(0.1, 0.01), (0.05, 0.0), (0.0, 0.01), (0.5, 1.0), (1e9, 0.01), (0.2, 0.01), (0.1, 0.0), (0.01, 0.01)]
RULE_N = (1, 2, 3, 7, 96, 2 ** 20)


def _host_rule(n, A, Q, thr, floor):
    fn = CAPI.lib().prt_adaptive_unconverged
    return np.array([bool(fn(float(a), float(b), float(c), float(thr), float(floor))) for a, b, c in zip(n, A, Q)])


def _boundary_q(n, A, thr, floor):
    """The float32 Q at which lhs is as close to t^2 as float32 allows: Q = n (t^2 (n - 1) + m^2), rounded once."""
    n64, A64 = np.asarray(n, np.float64), np.asarray(A, F).astype(np.float64)
    m = A64 / n64
    t = np.float64(F(thr)) * (m + np.float64(F(floor)))
    with np.errstate(over="ignore"):
        return (n64 * (t * t * (n64 - 1.0) + m * m)).astype(F)


def _rule_triples(thr, floor, count, rng):
    """(n, A, Q, boundary mask) of `count` decisions."""
    n = np.array(RULE_N, F)[np.arange(count) % len(RULE_N)]
    rng.shuffle(n)
    mean = rng.uniform(0.0, 3.0, count)
    spread = rng.uniform(0.0, 2.0, count) * (rng.random(count) < 0.7)   # 30 %: no spread, Q / n lands on either side of m^2
    A = (n.astype(np.float64) * mean).astype(F)
    Q = (n.astype(np.float64) * (mean * mean + spread * spread)).astype(F)
    kind = rng.integers(0, 10, count)
    below = kind == 0                                                    # Q / n < m^2 for certain: the clamp decides
    Q[below] = (Q[below] * F(0.999)).astype(F)
    black = kind == 1                                                    # A = 0: with noise_floor = 0, t = 0
    A[black] = 0
    Q[black] = np.where(rng.random(int(black.sum())) < 0.5, 0, Q[black]).astype(F)
    edge = (kind >= 5) & (n >= 2)                                        # built at the boundary, moved by -2 .. +2 ulp
    q = _boundary_q(n[edge], A[edge], thr, floor)
    for _ in range(2):
        q = np.nextafter(q, F(-np.inf))
    steps = rng.integers(0, 5, int(edge.sum()))
    for k in range(1, 5):
        q = np.where(steps >= k, np.nextafter(q, F(np.inf)), q).astype(F)
    Q[edge] = q
    edge &= np.isfinite(Q)
    return n, A, Q, edge


EQUALITY = {  # (thr, floor) -> [(n, A, Q)] with lhs == t^2 exactly: converged
    (0.5, 1.0): [(2, 2, 4), (3, 3, 9), (2, 6, 26)],
    (0.1, 0.0): [(2, 0, 0), (96, 0, 0)],
}


@pytest.mark.parametrize("config", range(len(RULE_CONFIGS)), ids=["thr%g_floor%g" % c for c in RULE_CONFIGS])
def test_the_device_rule_equals_the_host_rule_and_the_restatement(config):
    thr, floor = RULE_CONFIGS[config]
    g = _geometry(RW, RH)
    rng = np.random.default_rng(100 + config)
    tn, tA, tQ, edge = _rule_triples(thr, floor, g.n_local, rng)
    for i, (a, b, c) in enumerate(EQUALITY.get((thr, floor), [])):
        tn[i], tA[i], tQ[i], edge[i] = a, b, c, False
        lhs, t2 = ar.rule_terms(F(a), F(b), F(c), thr, floor)
        assert lhs == t2
    want = ar.unconverged(tn, tA, tQ, thr, floor)
    assert np.array_equal(_host_rule(tn, tA, tQ, thr, floor), want)
    for i in range(len(EQUALITY.get((thr, floor), []))):
        assert not want[i]   # equality counts as converged
    # one test pixel per tile, at a random inside position; every other pixel converged
    n, A, Q = g.converged_images()
    px = g.x0 + rng.integers(0, 8, g.n_local) % g.w
    py = g.y0 + rng.integers(0, 8, g.n_local) % g.h
    n[py, px], A[py, px], Q[py, px] = tn, tA, tQ
    got, count, pixels = g.r.tile_select(n, A, Q, thr, floor)
    flags = np.zeros(g.n_local, bool)
    flags[got[:count]] = True
    assert np.array_equal(flags, want), np.flatnonzero(flags != want)[:8]
    assert count == int(want.sum()) and pixels == int(g.inside[want].sum()) and (got[count:] == NONE).all()
    # the inputs are worth deciding: both answers occur, below two samples, and (where t^2 is finite and not 0 at A = 0)
    # on both sides of the boundary within two ulp of it
    assert want.any() and (tn < 2).any() and want[tn < 2].all()
    if thr < 1e8:
        assert not want.all()
        assert edge.sum() >= 300 and want[edge].any() and not want[edge].all()
