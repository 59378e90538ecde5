"""Randomized parity (-m gpu): tests/fuzz_parity.py's generator, a fixed seed, 200 cases.

Each case draws a scene (analytic primitives of every material, a refined mesh, placed copies of a second mesh, in any
combination), a camera, frame size, depth, sample count and batching, one of the three tree builders, the node layout, kernel
tunables (incl. a stack so small that rays take the overflow list) and the sampling flags, renders through the C-ABI and
compares EVERY pixel and the ray count with the oracle's throughput form (CPURenderer::TraceRay's iterative twin,
backend/cuda_megakernel/renderer.cu:81-119; PrimitiveList::Intersect semantics, core/primitive.cpp:21-59).
A longer run (6,300 cases, 0 mismatches) is recorded in DESIGN.md.
48 further cases render with light sampling and are held, sample by sample, to the float64 replay (tests/lighting_replay.py).
40 generated call sequences drive one long-lived context through the whole interface (tests/interface_sequences.py)."""
import importlib.util
import os

import pytest

import util  # noqa: F401  (puts the repo root on sys.path)

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(util.ROOT, "tests", "fuzz_parity.py"))
fuzz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fuzz)


@pytest.mark.parametrize("first", [0, 50, 100, 150])
def test_random_scenes_cameras_builders_and_tunables_bit_exact(first):
    bad = []
    for case in range(first, first + 50):
        msg, ok = fuzz.run_case(case, seed=7)
        if not ok:
            bad.append(msg)
    assert bad == []


@pytest.mark.parametrize("first", [0, 24])
def test_random_light_sampled_scenes_match_the_float64_replay(first):
    """fuzz_parity.run_lighting_case: the generators above with analytic primitives turned emissive at random (and emitters
    outside the light set), a random mode, sampling flags, batching and the tunables lighting honours; two sample indices per
    case, every stable pixel sample within the tolerance of tests/lighting_replay.py, shadow-ray counts and light set as in
    tests/test_gpu_lighting_replay.py.  A draw with too many undecidable light samples is redrawn; at most 10 % may be."""
    bad, redraws = [], 0
    for case in range(first, first + 24):
        msg, ok, n = fuzz.run_lighting_case(case, seed=17)
        print(msg, flush=True)
        redraws += n
        if not ok:
            bad.append(msg)
    assert bad == []
    assert redraws <= 0.1 * 24, redraws


@pytest.mark.parametrize("first", [0, 40])
def test_awkward_rays_against_the_brute_force_scan(first):
    """Closest hit of rays with zero direction components, axis-parallel rays, lattice origins, grazing and far-away rays on
    random scenes / builders / layouts, against the oracle's linear scan (PrimitiveList::Intersect, primitive.cpp:21-59)."""
    bad = []
    for case in range(first, first + 40):
        msg, ok = fuzz.run_ray_case(case, seed=11, n=2048)
        if not ok:
            bad.append(msg)
    assert bad == []


@pytest.mark.parametrize("first", [0])
def test_random_scenes_and_awkward_rays_moved_across_coordinate_scales(first):
    """fuzz_parity --scale: the generators above with scene, camera and rays moved by a (scale, translation) drawn from the
    non-extreme table of tests/scale_cases.py (scales 2^-20 .. 2^20, offsets up to 1e5); the oracle scans linearly (its own
    BVH has absolute pads).  30 frames + 30 ray cases."""
    import time
    t0 = time.time()
    bad = []
    for case in range(first, first + 30):
        for msg, ok in (fuzz.run_case(case, seed=19, scale=True), fuzz.run_ray_case(case, seed=23, n=2048, scale=True)):
            if not ok:
                bad.append(msg)
    print(f"scale fuzz slice: 60 cases in {time.time() - t0:.1f} s", flush=True)
    assert bad == []


def test_grazing_rays_from_far_away_keep_the_reference_spheres_phantom_hits():
    """Circle::Intersect's discriminant b*b - 4*a*c (shape.h:160-163) cancels for a far origin: a ray that passes up to
    ~2e-7 * dist^2 / R OUTSIDE a sphere is still a hit of the reference's arithmetic.  The walk over the primitives' world
    boxes (scenes with more than 16 primitives) must not cull those: its pad has a term in dist^2 (DevScene::abvh_q).
    40 small spheres, 200 k rays aimed to graze them within a few of those margins from 30 ... 1000 units away, against
    the oracle's linear scan; the test requires that phantom hits do occur in the sample."""
    import numpy as np
    from util import prt
    rng = np.random.default_rng(5)
    sc = prt.Scene(preset=None)
    mat = sc.AddLambertian((0.7, 0.7, 0.7))
    centres, radii = [], []
    for _ in range(40):
        c = rng.uniform(-5, 5, 3)
        s = float(rng.uniform(0.3, 1.5))
        r = float(rng.uniform(0.1, 0.6))
        sc.AddCircle(r, mat, scale=(s, s, s), translation=tuple(float(v) for v in c))
        centres.append(c)
        radii.append(r * s)
    centres, radii = np.array(centres), np.array(radii)
    n = 200_000
    i = rng.integers(0, 40, n)
    dist = np.exp(rng.uniform(np.log(30.0), np.log(1000.0), n))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = rng.normal(size=(n, 3))
    v -= (v * u).sum(1, keepdims=True) * u
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    m = rng.uniform(-2e-7, 5e-7, n) * dist * dist / radii[i]      # signed distance of the line from the sphere's surface
    ang = np.arcsin(np.clip((radii[i] + m) / dist, 0.0, 1.0))
    o = (centres[i] + u * dist[:, None]).astype(np.float32)
    d = (-u * np.cos(ang)[:, None] + v * np.sin(ang)[:, None]).astype(np.float32)
    d = np.stack([prt.glm_normalize(x) for x in d]).astype(np.float32)
    r = prt.HipWavefrontRenderer(device=0, max_depth=2, seed=0)
    r.Init(prt.Film(16, 16), sc, prt.Camera(position=(5.0, 5.0, 8.0), width=16, height=16))
    got = r.closest_hit(o, d)
    want = util.oracle_scene(sc).closest_hit(o, d, use_bvh=False, n_threads=16)
    assert util.hits_equal(got, want) == []
    # phantom hits are in the sample: hits on the aimed-at sphere by rays whose line (as fp32 data, in double) misses it
    oo, dd = o.astype(np.float64), d.astype(np.float64)
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    miss_by = np.linalg.norm(np.cross(oo - centres[i], dd), axis=1) - radii[i]
    phantom = (want["prim"] == i) & (miss_by > 1e-6 * dist)
    assert phantom.sum() > 100, int(phantom.sum())


def test_grazing_rays_along_triangle_edges_down_to_a_sixth_of_a_degree():
    """The adversarial case for box culling against Triangle::Intersect's rounding (shape.h:262-303): rays that graze a
    triangle's plane, travel along one of its edges and cross the plane within a few rounding errors of that edge, on
    meshes whose leaf boxes are tight there.  Down to a cosine of incidence of 3e-3 (0.17 degrees) the traversal returns
    what the oracle's brute-force scan returns.  Below that the reference's barycentrics are dominated by rounding (lateral
    error 3u * dist / cos: a quarter of a unit at cos 1e-5 from 14 units away) and it reports hits on triangles the ray does
    not come near; no spatial culling can follow it there: tests/graze_probe.py, DESIGN.md section 0."""
    spec = importlib.util.spec_from_file_location("graze_probe", os.path.join(util.ROOT, "tests", "graze_probe.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    gp.a.n, gp.a.cos_lo, gp.a.cos_hi = 150_000, 3e-3, 0.08
    for build in (0, 1):
        gp.a.gpu_build = build
        assert gp.probe("axis-aligned planar grid", *gp.grid_mesh()) == 0
        assert gp.probe("tilted planar grid", *gp.tilted_grid()) == 0
        m = util.prt.scenes.refined("bunny.ply", 12_000)
        assert gp.probe("bunny 12 k", m.GetVertices(), m.GetNormals(), m.GetIndices()) == 0


def test_random_call_sequences_on_one_long_lived_renderer():
    """ProgressiveRender in chunks, SetCamera, film Clear, sampling flags, samples in flight, run-time tunables, re-Init with
    another scene and film size, on one context or on a group of 2-3 contexts sharing the GPU (prt_group_*): after every
    render the film equals what the oracle accumulates for the same sequence (the reference's call contract:
    src/main.cpp:481-509, one more sample per ProgressiveRender, the caller clears the film)."""
    bad = []
    for case in range(60):
        msg, ok = fuzz.run_sequence_case(case, seed=13)
        if not ok:
            bad.append(msg)
    assert bad == []


@pytest.mark.parametrize("first", range(0, 40, 5))
def test_the_whole_interface_on_one_long_lived_renderer(first):
    """fuzz_parity.run_interface_case, the 40 cases whose coverage tests/test_interface_sequences.py counts without a GPU:
    renders of 1 .. 70 samples, every setter the oracle covers (Refit, UpdateInstances, set_film, max_depth and the tunables,
    primary_walk / primary_reuse / last_segment among them), the queries between the batches, excursions into lens,
    environment, textures, light sampling and an adaptive pass, on one context or a group.  After every render the film and
    the ray count are the oracle's and prt_primary_reuse is what the model of tests/interface_sequences.py allows; after every
    query its answer is the oracle's; an excursion's film is a fresh context's."""
    import interface_sequences as iseq
    assert iseq.CAMPAIGN_CASES == 40
    bad = []
    for case in range(first, first + 5):
        msg, ok = fuzz.run_interface_case(case, seed=iseq.CAMPAIGN_SEED)
        if not ok:
            bad.append(msg)
    assert bad == []
