"""The lit radiance query with a scatter pdf on the caller's segment (include/prt.h prt_radiance_lit_pb; radiance(pb=)) on
the GPU.

1. pb=None and pb = -1 everywhere equal radiance(lighting=True) bit for bit at depths 1, 2 and 5: sum, segments, final
   states and info.
2. The chain through a white vertex.  4099 rays with given states all hit a white Lambertian floor.  The full query with
   D + 1 segments is held against the continuation a caller builds from the public functions: closest_hit, scatter (the
   direction normalised in fp32), pb = max(0, n.d) / pi, the floor's light sample e0 from sample_light + occluded, and
   cont = radiance(so, d, rng', lighting=True, pb=pb, max_depth=D).
     D = 1: full == fl(cont + e0) bit for bit (the light sum of the full path is e0 alone, its path radiance is cont's).
     D = 2, 5: the same terms in two orders of fp32 additions: the path radiance L is identical, and the light sum is
       ((e0 + e1) + ...) against (e1 + ...) added to L before e0.  Two orders of at most D + 2 non-negative terms differ by
       at most 2 (D + 2) 2^-24 of the larger result per component: derived, not measured.
   Segments are cont's + 1 and the final states are equal.  The same chain without pb does NOT equal the full query on the
   rays whose continued segment meets a light, and there are such rays: the test can tell the weighting apart."""
import numpy as np
import pytest

import bake_replay as br
import lighting_replay as lr
from util import prt
from parallelraytracing_amd import capi
from test_gpu_bake import SEED, bits, cornell_with_cube, renderer

pytestmark = pytest.mark.gpu

F = np.float32
N = 4099
INV_PI = F(0.318309886183790672)


def cornell_rays():
    rng = np.random.default_rng(21)
    o = np.stack([rng.uniform(-4.0, 4.0, N), rng.uniform(0.5, 8.0, N), rng.uniform(-4.0, 4.0, N)], axis=1).astype(F)
    d = lr.normalize_rows_f32(rng.normal(size=(N, 3)).astype(F))
    return o, d, rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)


# ---- 1. pb = None and pb = -1 are the lit query -----------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["numpy", "torch"])
def test_no_pb_and_minus_one_are_the_lit_query_bit_for_bit(form):
    sc, _ = cornell_with_cube()
    r, _ = renderer(sc)
    r.set_lighting("mis")
    r.set_light_sources("all")
    o, d, states = cornell_rays()
    if form == "torch":
        import torch
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        o_, d_, minus = to(o), to(d), to(np.full(N, -1.0, F))
        st = lambda: to(states.view(np.int32))
        back = lambda a: a.cpu().numpy()
    else:
        o_, d_, minus = o, d, np.full(N, -1.0, F)
        st = lambda: states
        back = lambda a: a
    for depth in (1, 2, 5):
        _, want = r.radiance(o_, d_, rng_state=st(), max_depth=depth, lighting=True, return_info=True)
        assert back(want["sum"]).any() and (depth == 1 or want["shadow_rays"] > 0)
        for pb in (None, minus):
            _, got = r.radiance(o_, d_, rng_state=st(), max_depth=depth, lighting=True, return_info=True, pb=pb)
            assert np.array_equal(bits(back(got["sum"])), bits(back(want["sum"]))), (depth, pb is None)
            assert np.array_equal(back(got["segments"]), back(want["segments"]))
            assert np.array_equal(back(got["rng_state"]).view(np.uint32), back(want["rng_state"]).view(np.uint32))
            assert (got["shadow_rays"], got["shadow_occluded"]) == (want["shadow_rays"], want["shadow_occluded"])
    # samples by ray index (no states), several samples: the value applies to every sample of its ray
    _, want = r.radiance(o_, d_, samples=3, first_sample=2, max_depth=3, lighting=True, return_info=True)
    _, got = r.radiance(o_, d_, samples=3, first_sample=2, max_depth=3, lighting=True, return_info=True, pb=minus)
    assert np.array_equal(bits(back(got["sum"])), bits(back(want["sum"]))) and np.array_equal(back(got["segments"]), back(want["segments"]))
    # NaN means no weighting too; under lighting off pb is ignored and the result is the unlit query's
    nan = np.full(N, np.nan, F)
    _, got = r.radiance(o, d, rng_state=states, max_depth=2, lighting=True, return_info=True, pb=nan)
    _, want = r.radiance(o, d, rng_state=states, max_depth=2, lighting=True, return_info=True)
    assert np.array_equal(bits(got["sum"]), bits(want["sum"]))
    r.set_lighting("off")
    _, got = r.radiance(o, d, rng_state=states, max_depth=3, lighting=True, return_info=True, pb=np.full(N, 0.2, F))
    _, want = r.radiance(o, d, rng_state=states, max_depth=3, return_info=True)
    assert np.array_equal(bits(got["sum"]), bits(want["sum"])) and np.array_equal(got["rng_state"], want["rng_state"])
    assert got["shadow_rays"] == 0


# ---- 2. the chain through a white vertex -----------------------------------------------------------------------------------
def floor_scene():
    """A white Lambertian floor (primitive 0) under a black sky, a quad light (primitive 1) and an emissive mesh above it."""
    sc = prt.Scene(preset=None, sky=(0.0, 0.0, 0.0))
    white = sc.AddLambertian((1.0, 1.0, 1.0))
    sc.AddQuad(40.0, 40.0, white)
    sc.AddQuad(2.0, 2.0, sc.AddEmissive((8.0, 7.0, 6.0)), euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 3.0, 0.0))
    m = br.square_mesh(1.5)
    mat, inv = prt.make_transform((1.0, 1.0, 1.0), (180.0, 0.0, 0.0), (1.8, 2.5, 0.4))
    sc.AddMesh(m.transform(mat, inv), sc.AddEmissive((3.0, 4.0, 5.0)))
    cube = br.cube_mesh()                                  # a Lambertian cube between floor and lights: a blocker, and more vertices
    mat, inv = prt.make_transform((0.4, 0.4, 0.4), (0.0, 25.0, 0.0), (-0.8, 1.5, 0.3))
    sc.AddMesh(cube.transform(mat, inv), sc.AddLambertian((0.6, 0.5, 0.4)))
    return sc, white


def floor_rays():
    rng = np.random.default_rng(33)
    o = np.stack([rng.uniform(-2.5, 2.5, N), rng.uniform(0.2, 0.9, N), rng.uniform(-2.5, 2.5, N)], axis=1).astype(F)
    d = np.stack([rng.uniform(-0.6, 0.6, N), np.full(N, -1.0), rng.uniform(-0.6, 0.6, N)], axis=1).astype(F)
    return o, lr.normalize_rows_f32(d), rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("mode", ["mis", "nee"])
@pytest.mark.parametrize("env", [False, True])
def test_chain_through_a_white_vertex(env, mode):
    sc, white = floor_scene()
    r, _ = renderer(sc)
    r.set_lighting(mode)
    r.set_light_sources("all")
    if env:
        r.set_environment(np.random.default_rng(8).uniform(0.1, 2.0, (8, 16, 3)).astype(F), 0.5)
    o, d, R = floor_rays()      # (rr_depth = 0, clamp = 0: the renderer's defaults)
    hits = r.closest_hit(o, d)
    assert (hits["prim"] == 0).all() and (hits["material_id"] == white).all() and (hits["front_face"] == 1).all()
    scattered, att, em, so, sd, R1 = r.scatter(d, hits, R)
    assert scattered.all() and (att == 1).all() and not em.any()
    d1 = lr.normalize_rows_f32(sd)
    n = hits["normal"].astype(F)
    c = ((n[:, 0] * d1[:, 0] + n[:, 1] * d1[:, 1]).astype(F) + (n[:, 2] * d1[:, 2]).astype(F)).astype(F)
    pb = (np.where(c > 0, c, F(0)).astype(F) * INV_PI).astype(F)
    ls = r.sample_light(d, hits, R)
    cast = ls["pdf_bsdf"] > 0
    occ = r.occluded(hits["position"], ls["dir"], np.where(cast, ls["tmax"], F(0)).astype(F))
    e0 = np.where((cast & ~occ)[:, None], ls["contrib"], F(0)).astype(F)
    assert cast.sum() > N // 2 and occ.any() and e0.any()
    lit_hit = r.closest_hit(so, d1)
    on_light = (lit_hit["prim"] >= 0) & np.isin(lit_hit["material_id"], [1, 2])      # the two emissive materials
    assert on_light.sum() > 50 and {int(v) for v in lit_hit["prim"][on_light]} >= {1}
    assert (lit_hit["prim"][on_light] >= 2).any()            # the emissive mesh's triangles too
    for D in (1, 2, 5):
        _, full = r.radiance(o, d, rng_state=R, max_depth=D + 1, lighting=True, return_info=True)
        _, cont = r.radiance(so, d1, rng_state=R1, max_depth=D, lighting=True, return_info=True, pb=pb)
        assert np.array_equal(full["segments"], cont["segments"] + 1), D
        assert np.array_equal(full["rng_state"], cont["rng_state"]), D
        if D == 1:
            want = (cont["sum"] + e0).astype(F)
            bad = np.nonzero((bits(full["sum"]) != bits(want)).any(axis=1))[0]
            assert bad.size == 0, (env, mode, bad[:8], full["sum"][bad[:3]], want[bad[:3]])
            _, none = r.radiance(so, d1, rng_state=R1, max_depth=1, lighting=True, return_info=True)
            differs = (bits(none["sum"]) != bits(cont["sum"])).any(axis=1)
            assert differs[on_light].all(), (env, mode, np.nonzero(on_light & ~differs)[0][:8])
            assert ((none["sum"] + e0).astype(F) != full["sum"]).any(axis=1)[on_light].all()
            if not env:
                assert not differs[~on_light].any()          # a black sky and a Lambertian hit carry no weight
        else:
            a = full["sum"].astype(np.float64)
            b = cont["sum"].astype(np.float64) + e0.astype(np.float64)
            bound = 2.0 * (D + 2) * 2.0 ** -24 * np.maximum(a, b)
            err = np.abs(a - b)
            print(f"env={env} {mode} D={D}: max |full - (cont + e0)| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
            assert (err <= bound).all(), (env, mode, D, (err - bound).max())
        assert full["shadow_rays"] == cont["shadow_rays"] + int(cast.sum()), D
        assert (cont["shadow_rays"] > 0) == (D > 1), D
