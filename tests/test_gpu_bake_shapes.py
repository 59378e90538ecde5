"""Surface baking on the GPU beyond toy maps: the shapes of tests/bake_replay.py's BIG_SHAPES (a grid whose vertices are texel
centres, a 2,003-face soup, faces far larger than the map, near-collinear slivers, a 20 k-face scan under a planar projection,
a placed copy) on maps of several compaction trips, strips and the sizes at which the coverage rule is exact.  tests/
test_bake_replay.py shows from the replay alone what makes each shape a test.

1. Surface: bake_surface equals the replay bit for bit on every shape and size, counts included; the grid on dyadic maps also
   equals the lowest coverer in exact rational arithmetic.
2. Rays: bake_rays equals the replay bit for bit on maps of thousands of covered texels.
3. The texel list, through the sums: bake_irradiance equals the ordered fp32 sum of the public radiance query over bake_rays'
   outputs at every covered texel, in every chunking, unlit, light-sampled and with the texel's light sample: a list with a
   texel missing, repeated or out of place cannot pass.
4. The gutter fill over several passes, 5. one context across a large map, a small one and the large one again."""
import functools

import numpy as np
import pytest

import bake_replay as br
from util import prt
from test_gpu_bake import SEED, _paths_by_the_public_query, bits, renderer, same_surface

pytestmark = pytest.mark.gpu

F = np.float32
CASES = [(name, H, W) for name in br.BIG_SHAPES for H, W in br.SHAPE_SIZES[name]]


def scene_of(name):
    """The shape on the ground quad under the emissive quad -> (scene, target keywords with the UVs of the call)"""
    s = br.shape(name)
    sc = prt.Scene(preset=None, sky=(0.4, 0.3, 0.6))
    ground, light, body = sc.AddLambertian((0.5, 0.5, 0.5)), sc.AddEmissive((15.0, 15.0, 15.0)), sc.AddLambertian((0.8, 0.8, 0.8))
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -2.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 7.0, 0.0))
    uvs = s["uvs"] if s["uvs"] is not None else s["mesh"].GetUVs()
    if s["placed"]:
        sc.AddMesh(br.square_mesh(3.0, -1.5), ground)           # a world-space mesh beside the copy
        sc.AddInstance(s["mesh"], body, scale=br.COPY_SRT[0], euler_deg=br.COPY_SRT[1], translation=br.COPY_SRT[2])
        return sc, dict(instance=0, uvs=uvs)
    sc.AddMesh(s["mesh"], body)
    return sc, dict(mesh=0, uvs=uvs)


def fresh(name):
    sc, kw = scene_of(name)
    return renderer(sc)[0], kw


@functools.lru_cache(maxsize=None)
def context(name):
    """One renderer per shape, shared by the tests that only read it"""
    return fresh(name)


def same_info(info, want, H, W):
    return (info["n_texels"], info["n_covered"], info["n_degenerate"], info["n_faces_skipped"]) == \
        (H * W, want["n_covered"], want["n_degenerate"], want["n_faces_skipped"])


# ---- 1. surface -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,H,W", CASES)
def test_surface_equals_the_replay_bit_for_bit(name, H, W):
    r, kw = context(name)
    want = br.reference(name, H, W)
    got = r.bake_surface(size=(H, W), **kw)
    bad = same_surface(got, want)
    differ = np.argwhere(got["owner"] != want["owner"])
    assert bad == [], (name, H, W, bad, len(differ), differ[:8].tolist(), got["owner"][tuple(differ[:8].T)], want["owner"][tuple(differ[:8].T)])
    assert same_info(got["info"], want, H, W), (got["info"], want["n_covered"], want["n_degenerate"], want["n_faces_skipped"])
    if name == "grid" and (H, W) in br.DYADIC:
        s = br.shape(name)
        owner, count = br.exact_owner(br.mesh_faces(s["mesh"])[0], W, H)
        assert (count > 1).any() and np.array_equal(got["owner"], owner)


# ---- 2. rays --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "ico_copy"])
def test_rays_equal_the_replay_bit_for_bit(name):
    r, kw = context(name)
    H, W = 80, 96
    surf = br.reference(name, H, W)
    assert surf["n_covered"] > 3 * 1024
    for sample in (0, 3):
        want = br.rays(surf, sample, SEED)
        got = r.bake_rays(size=(H, W), sample=sample, **kw)
        assert np.array_equal(bits(got["o"]), bits(want["o"])) and np.array_equal(bits(got["d"]), bits(want["d"])), (name, sample)
        assert np.array_equal(got["rng_state"], want["rng_state"]), (name, sample)


# ---- 3. the texel list, through the sums ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lighting", [False, True])
@pytest.mark.parametrize("name,H,W", [("soup", 80, 96), ("soup", 1, 2049), ("bunny", 33, 129)])
def test_sums_are_the_radiance_querys_at_every_listed_texel(name, H, W, lighting):
    r, kw = fresh(name)
    if lighting:
        r.set_lighting("mis")
        r.set_light_sources("all")
    ref = br.reference(name, H, W)
    cov, want, seg, shadow = _paths_by_the_public_query(r, kw, H, W, 3, 2, lighting)
    assert np.array_equal(cov, ref["coverage"].ravel() != 0) and cov.sum() > 1024 and not cov[:1024].all() and not cov[-1024:].all()
    assert want.any() and seg > 3 * cov.sum() and len(np.unique(want, axis=0)) > 4
    for chunk in (0, 1, 2):
        r.set_param("bake_chunk", chunk)
        irr, got = r.bake_irradiance(size=(H, W), samples=3, first_sample=2, lighting=lighting, return_info=True, **kw)
        total = got["sum"].reshape(-1, 3)
        bad = np.nonzero((bits(total[cov]) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (name, H, W, lighting, chunk, bad.size, bad[:8], total[cov][bad[:3]], want[bad[:3]])
        assert not total[~cov].any() and np.array_equal(got["coverage"].ravel() != 0, cov)
        assert got["info"]["segments"] == seg and got["info"]["rays"] == 3 * cov.sum() and got["info"]["n_covered"] == cov.sum()
        assert got["info"]["shadow_rays"] == shadow and (shadow > 0) == lighting
        assert np.array_equal(bits(irr), bits(got["sum"] * F(np.pi) / F(3)))


def test_texel_light_sums_are_the_composition_on_a_long_list():
    from test_gpu_bake_light import _composition
    r, kw = fresh("soup")
    r.set_lighting("mis")
    H, W = 80, 96
    cov, want, seg, shadow, texel_rays = _composition(r, kw, H, W, 3, 2)
    assert cov.sum() > 3 * 1024 and want.any() and texel_rays > cov.sum() // 2 and len(np.unique(want, axis=0)) > 4
    plain = r.bake_irradiance(size=(H, W), samples=3, first_sample=2, lighting=True, return_info=True, **kw)[1]
    assert not np.array_equal(bits(plain["sum"].reshape(-1, 3)[cov]), bits(want))      # the option does something
    for chunk in (0, 1, 2):
        r.set_param("bake_chunk", chunk)
        _, got = r.bake_irradiance(size=(H, W), samples=3, first_sample=2, lighting=True, texel_light=True, return_info=True, **kw)
        total = got["sum"].reshape(-1, 3)
        bad = np.nonzero((bits(total[cov]) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (chunk, bad.size, bad[:8], total[cov][bad[:3]], want[bad[:3]])
        assert not total[~cov].any() and np.array_equal(got["coverage"].ravel() != 0, cov)
        assert got["info"]["segments"] == seg and got["info"]["rays"] == 3 * cov.sum() and got["info"]["shadow_rays"] == shadow


# ---- 4. gutter fill -------------------------------------------------------------------------------------------------------
def test_dilate_equals_the_replays_fill_over_several_passes():
    r, kw = context("soup")
    H, W = 80, 96
    _, base = r.bake_irradiance(size=(H, W), samples=2, return_info=True, **kw)
    assert np.array_equal(base["coverage"], br.reference("soup", H, W)["coverage"]) and base["info"]["n_filled"] == 0
    c1 = br.dilate(base["coverage"], base["sum"], 1)[0]
    c2 = br.dilate(base["coverage"], base["sum"], 2)[0]
    # pass 2 fills texels none of whose neighbours was owned: all they see was filled by pass 1
    second = (c2 == 2) & (c1 == 0)
    padded = np.pad(base["coverage"], 1)
    owned_near = sum(padded[1 + di:1 + di + H, 1 + dj:1 + dj + W] for di, dj in br.NEIGHBOURS)
    assert second.any() and not owned_near[second].any()
    for passes in (1, 4):
        cov, val, filled = br.dilate(base["coverage"], base["sum"], passes)
        _, got = r.bake_irradiance(size=(H, W), samples=2, dilate=passes, return_info=True, **kw)
        assert np.array_equal(got["coverage"], cov) and np.array_equal(bits(got["sum"]), bits(val)), passes
        assert got["info"]["n_filled"] == filled > 0 and np.isfinite(got["sum"]).all() and (got["coverage"] == 2).sum() == filled
    assert filled > int((c1 == 2).sum())


# ---- 5. context reuse -----------------------------------------------------------------------------------------------------
def test_one_context_across_a_large_map_a_small_one_and_the_large_one_again():
    def bake(r, kw, size):
        _, got = r.bake_irradiance(size=size, samples=2, dilate=1, return_info=True, **kw)
        return got

    def same(a, b):
        return np.array_equal(bits(a["sum"]), bits(b["sum"])) and np.array_equal(a["coverage"], b["coverage"]) and \
            {k: v for k, v in a["info"].items() if k != "device_ms"} == {k: v for k, v in b["info"].items() if k != "device_ms"}

    r, kw = fresh("soup")
    seq = [bake(r, kw, size) for size in ((128, 128), (3, 5), (128, 128))]
    big, small = bake(*fresh("soup"), (128, 128)), bake(*fresh("soup"), (3, 5))
    ref = br.reference("soup", 128, 128)
    assert np.array_equal(big["coverage"] == 1, ref["coverage"] != 0) and big["info"]["n_covered"] == ref["n_covered"] > 8 * 1024
    assert big["sum"].any() and same(seq[0], big) and same(seq[1], small) and same(seq[2], big)
