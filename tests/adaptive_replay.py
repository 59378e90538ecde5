"""Restatement of the film statistics and of prt_render_adaptive's loop (include/prt.h "Film statistics and adaptive
sampling") in numpy: the moments in float32, operation for operation, the stopping rule in float64, and the adaptive loop
walked over per-sample frames (one (H, W, 3) float32 radiance frame per sample index, from the oracle or from one-sample
renders, both of which are exact: 0 + x = x)."""
import numpy as np

F = np.float32
KR, KG, KB = F(0.2126), F(0.7152), F(0.0722)


def luminance(rgb):
    """y = (0.2126f r + 0.7152f g) + 0.0722f b, every operation rounded to float32."""
    rgb = np.asarray(rgb, F)
    return ((KR * rgb[..., 0] + KG * rgb[..., 1]).astype(F) + (KB * rgb[..., 2]).astype(F)).astype(F)


def add_sample(A, Q, rgb):
    """A += y; Q += y * y, in place, float32."""
    y = luminance(rgb)
    A += y
    Q += (y * y).astype(F)


def moments(frames):
    """(A, Q) after adding `frames` (an iterable of (H, W, 3) float32 frames) in order."""
    A = Q = None
    for f in frames:
        if A is None:
            A = np.zeros(f.shape[:2], F)
            Q = np.zeros(f.shape[:2], F)
        add_sample(A, Q, f)
    return A, Q


def rule_terms(n, A, Q, threshold, noise_floor):
    """(lhs, t^2) of the rule in float64, in the order of the contract; callers handle n < 2."""
    n = np.asarray(n, F).astype(np.float64)
    A = np.asarray(A, F).astype(np.float64)
    Q = np.asarray(Q, F).astype(np.float64)
    with np.errstate(all="ignore"):
        m = A / n
        V = np.maximum(0.0, Q / n - m * m)
        lhs = V / (n - 1.0)
        t = np.float64(F(threshold)) * (m + np.float64(F(noise_floor)))
        return lhs, t * t


def unconverged(n, A, Q, threshold, noise_floor):
    lhs, t2 = rule_terms(n, A, Q, threshold, noise_floor)
    with np.errstate(all="ignore"):
        return (np.asarray(n, F) < F(2)) | (lhs > t2)


def noise_map(n, A, Q, noise_floor):
    """prt_film_noise_read: sqrt(V / (n - 1)) / (m + noise_floor) in float64, rounded once; +inf where n < 2."""
    n64 = np.asarray(n, F).astype(np.float64)
    with np.errstate(all="ignore"):
        m = np.asarray(A, F).astype(np.float64) / n64
        V = np.maximum(0.0, np.asarray(Q, F).astype(np.float64) / n64 - m * m)
        out = (np.sqrt(V / (n64 - 1.0)) / (m + np.float64(F(noise_floor)))).astype(F)
    out[np.asarray(n, F) < F(2)] = np.inf
    return out


def tiles(W, H):
    """[(x0, y0, x1, y1)] of the 8x8 tiles, row-major (the last column / row may be partial)."""
    return [(x, y, min(x + 8, W), min(y + 8, H)) for y in range(0, H, 8) for x in range(0, W, 8)]


class Replay:
    """The adaptive loop over frame(s) -> (H, W, 3) float32 radiance of sample index s.  State persists, so a second run()
    continues a finished frame (min_spp = 0, a later first_sample)."""

    def __init__(self, W, H, frame):
        self.W, self.H, self.frame = W, H, frame
        self.accum = np.zeros((H, W, 3), F)
        self.n = np.zeros((H, W), F)
        self.A = np.zeros((H, W), F)
        self.Q = np.zeros((H, W), F)
        self.tiles = tiles(W, H)

    def _add(self, s, tile_ids):
        f = self.frame(s)
        for i in tile_ids:
            x0, y0, x1, y1 = self.tiles[i]
            sl = (slice(y0, y1), slice(x0, x1))
            self.accum[sl] += f[sl]
            self.n[sl] += F(1)
            y = luminance(f[sl])
            self.A[sl] += y
            self.Q[sl] += (y * y).astype(F)

    def run(self, min_spp, step_spp, max_spp, threshold, noise_floor, first_sample=0, ranks=1):
        """Returns a dict: counts (per tile, samples of this call), ranges (per tile: (first, count)), the info fields for
        the whole film, margins (|lhs - t^2| / t^2 of every pixel decision made at n >= 2 with t^2 > 0), `per_rank`: the info
        fields of every rank of a round-robin partition (each rank loops over its own tiles), and `selects`: per rank, for
        every select of its loop in turn, (the number of tiles it was given, the global ids of those it kept, ascending)."""
        nt = len(self.tiles)
        counts = np.zeros(nt, np.int64)
        margins = []
        info = [dict(passes=0, tiles_local=len(range(r, nt, ranks)), tiles_converged=0, tiles_capped=0, stops=[],
                     pixel_samples=0) for r in range(ranks)]
        selects = [[] for r in range(ranks)]
        if min_spp:
            for s in range(min_spp):
                self._add(first_sample + s, range(nt))
            counts[:] = min_spp
            for r in range(ranks):
                info[r]["pixel_samples"] = min_spp * sum(self._pixels(i) for i in range(r, nt, ranks))
        for r in range(ranks):  # each rank walks its own loop; the film is shared because tiles are disjoint
            active = list(range(r, nt, ranks))
            added = min_spp
            I = info[r]
            while active:
                still = []
                for i in active:
                    x0, y0, x1, y1 = self.tiles[i]
                    sl = (slice(y0, y1), slice(x0, x1))
                    lhs, t2 = rule_terms(self.n[sl], self.A[sl], self.Q[sl], threshold, noise_floor)
                    with np.errstate(all="ignore"):
                        ok = (self.n[sl] >= F(2)) & (t2 > 0)
                        margins.extend((np.abs(lhs - t2) / t2)[ok].ravel().tolist())
                    if unconverged(self.n[sl], self.A[sl], self.Q[sl], threshold, noise_floor).any():
                        still.append(i)
                selects[r].append((len(active), np.array(still, np.int64)))
                if len(still) < len(active):
                    I["tiles_converged"] += len(active) - len(still)
                    I["stops"].append(added)
                active = still
                if not active:
                    break
                if added >= max_spp:
                    I["tiles_capped"] = len(active)
                    I["stops"].append(added)
                    break
                k = min(step_spp, max_spp - added)
                for s in range(k):
                    self._add(first_sample + added + s, active)
                counts[active] += k
                I["pixel_samples"] += k * sum(self._pixels(i) for i in active)
                I["passes"] += 1
                added += k
        for I in info:
            I["min_tile_spp"] = min(I["stops"]) if I["stops"] else 0
            I["max_tile_spp"] = max(I["stops"]) if I["stops"] else 0
        with_tiles = [I for I in info if I["tiles_local"]]
        total = dict(passes=max(I["passes"] for I in info), tiles_local=nt,
                     tiles_converged=sum(I["tiles_converged"] for I in info), tiles_capped=sum(I["tiles_capped"] for I in info),
                     pixel_samples=sum(I["pixel_samples"] for I in info),
                     min_tile_spp=min(I["min_tile_spp"] for I in with_tiles), max_tile_spp=max(I["max_tile_spp"] for I in with_tiles))
        return dict(counts=counts, info=total, per_rank=info, margins=np.array(margins, np.float64), selects=selects,
                    ranges=[(first_sample, int(c)) for c in counts])

    def _pixels(self, i):
        x0, y0, x1, y1 = self.tiles[i]
        return (x1 - x0) * (y1 - y0)

    def count_map(self, counts):
        m = np.zeros((self.H, self.W), F)
        for i, (x0, y0, x1, y1) in enumerate(self.tiles):
            m[y0:y1, x0:x1] = counts[i]
        return m


INFO_FIELDS = ("passes", "tiles_local", "tiles_converged", "tiles_capped", "min_tile_spp", "max_tile_spp", "pixel_samples")


def info_dict(info):
    """A PrtAdaptiveInfo as the dict the replay produces."""
    return {k: int(getattr(info, k)) for k in INFO_FIELDS}


def replay_info(rep):
    return {k: int(rep["info"][k]) for k in INFO_FIELDS}


# The two fixtures of the issue: (5, 5, 8) camera toward the origin, 44 x 28 film (partial tiles on two edges), depth 4,
# seed 3, first_sample 0, 8 / 8 / 96 samples, noise floor 0.01
FIXTURE = dict(W=44, H=28, depth=4, seed=3, min_spp=8, step_spp=8, max_spp=96, noise_floor=0.01, cam_pos=(5.0, 5.0, 8.0))
FIXTURE_THRESHOLDS = {"CORNELL": 0.10, "DEFAULT": 0.15}

# A film whose tile lists span k_tile_compact's trips of 1024 flags: 56 x 44 = 2464 tiles, both edges partial; as 3 ranks
# 822 / 821 / 821 local tiles.  4 / 4 / 32 samples, first_sample 0.
FIXTURE_WIDE = dict(W=444, H=348, depth=4, seed=3, min_spp=4, step_spp=4, max_spp=32, noise_floor=0.01, cam_pos=(5.0, 5.0, 8.0),
                    preset="CORNELL", threshold=0.2)


def runs(ids):
    """The number of runs of consecutive tile ids in an ascending list."""
    ids = np.asarray(ids, np.int64)
    return int(len(ids) > 0) + int((np.diff(ids) != 1).sum())
