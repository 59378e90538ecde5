"""Ray families and cases for holding the radiance queries (include/prt.h "Radiance query") to the float64 replays on rays
the caller chose.  HIP-free: the CPU test of the reference side (test_query_replay.py) and the GPU test
(test_gpu_query_replay.py) share the rays, the cases and the replay of a case.

A family is N = 4099 rays (a multiple of neither 64 nor 256: 17 blocks of the step kernel, the last one partial) with uint32
RNG states, all from one np.random.default_rng(seed) per family and case:

  shell   util.random_rays around the geometry, centre / radius / spread as tests/test_gpu_radiance.py's RAYS and
          tests/test_gpu_radiance_lit.py's _cloud use them for the same scenes (restated in SHELL);
  inside  origins uniform in a box that encloses the scene's objects (INSIDE_BOX), directions uniform on the sphere and
          normalised with glm_normalize: rays that start inside the glass and metal spheres, inside a closed mesh, behind
          and above the quad lights, inside the Cornell box;
  gap     scene `resting` only: ground points at radius rho from the contact point of the resting sphere light, rho^2
          uniform in [0.05^2, 3^2] (uniform by area: with rho itself uniform the share of vertices on the margin's edge breaks
          the cap on undecidable samples), the origin halfway up the gap above the ground point, the direction (u, -1, v)
          normalised, u, v uniform in +-0.2: first vertices inside and outside the sphere's margin;
  scaled  the shell family, every direction multiplied in fp32 by a per-ray factor from SCALES: directions are used as
          given, not normalised.

The replays model a render, which skips the material's draws on the last segment; the queries make them.  Radiance and
segments are the same; final RNG states are therefore compared with OracleScene.trace, never with a replay."""
from __future__ import annotations

import contextlib
import functools

import numpy as np

import environment_replay as er
import light_cluster_replay as lcr
import lighting_replay as lr
import mesh_light_replay as mr
import texture_replay as tex
import util
from util import orc, prt

F = np.float32
N = 4099
SEED = 11
MODES = ("mis", "nee")
SCALES = (0.125, 1.0, 1.0, 3.7)
CLUSTERS = 8
RR_CLAMP = (0, 2, 1.5)
FAMILIES = ("shell", "inside", "gap", "scaled")

# centre, radius, spread of util.random_rays per geometry
_CLOUD = ((0.0, 0.5, 0.0), 7.0, 2.5)                  # test_gpu_radiance_lit._cloud: the ground-and-objects scenes
SHELL = {"penumbra": _CLOUD, "specular": _CLOUD, "placed": _CLOUD, "bunny_light": _CLOUD,
         "CORNELL": ((0.0, 1.0, 0.0), 12.0, 3.0), "DEFAULT": ((0.0, 1.0, 0.0), 14.0, 6.0),         # test_gpu_radiance.RAYS
         "RANDOM_BALLS_SMALL": ((0.0, 1.0, 0.0), 14.0, 6.0), "MATERIAL_TEST": ((0.0, 1.0, 0.0), 12.0, 4.0),
         "COPIES": ((0.0, 0.5, 0.0), 9.0, 3.0),
         "textured": ((0.0, 0.0, 0.0), 6.0, 2.0)}      # texture_replay.primary_and_random_rays
INSIDE_BOX = {"penumbra": ((-4.0, -0.99, -4.0), (4.0, 3.5, 4.0)), "specular": ((-4.0, -0.99, -3.0), (4.0, 3.9, 3.0)),
              "CORNELL": ((-2.0, 0.1, -2.0), (2.0, 3.0, 2.0)), "bunny": ((-2.5, -0.99, -2.5), (2.5, 3.2, 2.5))}


def _row(name, geometry, build, families, sources="analytic", selection="power", blockers=True, textured=False, oracle=True,
         longest=None):
    """longest: the longest path the scene's geometry admits, where that is below the case's depth (None: the depth)."""
    return dict(name=name, geometry=geometry, build=build, families=families, sources=sources, selection=selection,
                blockers=blockers, textured=textured, oracle=oracle, longest=longest)


def _lr_case(name, sampling=None):
    def build():
        c = lr.case(name, 9, 7)
        if sampling is not None:
            c["sampling"] = sampling
        return dict(c, sources="analytic", env=None)
    return build


def _mr_case(name):
    return lambda: dict(mr.case(name, 9, 7), sources="all", env=None)


def _er_case(name):
    def build():
        c = er.case(name)
        assert c["light_share"] == 0.5
        return dict(c, env=er.case_env(c))
    return build


def _tex_case(name):
    def build():
        c = tex.lighting_case(name)[0]
        return dict(c, env=er.case_env(c) if name.endswith("_env") else None)
    return build


# The rows of the lit query's table (every row runs in both modes).  oracle: OracleScene.trace covers the scene and the
# sampling (no texture, no environment image, no roulette or clamp), so the unlit query is held to it as well.
ROWS = (
    _row("penumbra", "penumbra", _lr_case("penumbra"), ("shell", "inside", "scaled")),
    _row("specular", "specular", _lr_case("specular"), ("shell", "inside")),
    _row("DEFAULT_rr_clamp", "DEFAULT", _lr_case("DEFAULT", RR_CLAMP), ("shell", "scaled"), oracle=False),
    _row("RANDOM_BALLS_SMALL", "RANDOM_BALLS_SMALL", _lr_case("RANDOM_BALLS_SMALL"), ("shell",)),
    _row("CORNELL", "CORNELL", _lr_case("CORNELL"), ("inside",)),
    _row("resting", "resting", _lr_case("resting"), ("gap",), blockers=False, longest=2),
    _row("placed_power", "placed", _mr_case("placed"), ("shell",), "all"),
    _row("placed_clustered", "placed", _mr_case("placed"), ("shell",), "all", "clustered"),
    _row("bunny_light_power", "bunny_light", _mr_case("bunny_light"), ("shell",), "all", longest=2),
    _row("bunny_light_clustered", "bunny_light", _mr_case("bunny_light"), ("shell",), "all", "clustered", longest=2),
    _row("env_DEFAULT_sun", "DEFAULT", _er_case("DEFAULT_sun"), ("shell", "scaled"), oracle=False),
    _row("env_placed_mesh", "placed", _er_case("placed_mesh"), ("shell",), "all", oracle=False),
    _row("env_blackrows", "DEFAULT", _er_case("blackrows"), ("shell",), oracle=False),
    _row("tex_A_mis_analytic", "textured", _tex_case("A_mis_analytic"), ("shell",), textured=True, oracle=False),
    _row("tex_B_mis_mesh", "textured", _tex_case("B_mis_mesh"), ("shell",), "all", textured=True, oracle=False),
    _row("tex_B_nee_mesh_env", "textured", _tex_case("B_nee_mesh_env"), ("shell",), "all", textured=True, oracle=False),
)
ROW = {r["name"]: r for r in ROWS}
LIT = tuple((r["name"], f) for r in ROWS for f in r["families"])
# the reference side alone: the bunny scene (rays that start inside a closed mesh) runs on the CPU only
CPU_ONLY = (_row("bunny", "bunny", _lr_case("bunny"), ("inside",)),)
MULTI_SAMPLE = ("penumbra", "placed_clustered", "tex_B_nee_mesh_env")      # seeds by ray index, samples (2, 3, 4)
UNLIT_BLIND = ("tex_B_nee_mesh_env", "env_DEFAULT_sun")                    # lighting off where the oracle is blind
SCALED_ORACLE = ("CORNELL", "DEFAULT+", "MATERIAL_TEST", "COPIES")         # tests/test_gpu_radiance.py's make_scene


def row(name):
    return ROW.get(name) or {r["name"]: r for r in CPU_ONLY}[name]


def family_seed(case_name, family):
    names = [r["name"] for r in ROWS + CPU_ONLY] + list(SCALED_ORACLE) + ["empty"]
    return 1 + 7 * names.index(case_name) + FAMILIES.index(family)


def _states(rng, n):
    return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def _unit_rows(v):
    return np.stack([prt.glm_normalize(x) for x in np.asarray(v, F)]).astype(F)


@functools.lru_cache(maxsize=None)
def rays(case_name, family, geometry=None):
    """(o, d, state) of one family for one case: computed once, shared, never written to."""
    geometry = geometry or row(case_name)["geometry"]
    # `scaled` is the shell family scaled: the same generator, the factors drawn after the states
    rng = np.random.default_rng(family_seed(case_name, "shell" if family == "scaled" else family))
    if family in ("shell", "scaled"):
        centre, radius, spread = SHELL[geometry]
        o, d = util.random_rays(rng, N, center=centre, radius=radius, spread=spread)
        st = _states(rng, N)
        if family == "scaled":
            d = (d * rng.choice(np.asarray(SCALES, F), N)[:, None]).astype(F)
    elif family == "inside":
        lo, hi = INSIDE_BOX[geometry]
        o = rng.uniform(lo, hi, (N, 3)).astype(F)
        d = _unit_rows(rng.normal(size=(N, 3)))
        st = _states(rng, N)
    elif family == "gap":
        assert geometry == "resting"
        rho = np.sqrt(rng.uniform(0.05 ** 2, 3.0 ** 2, N))
        phi = rng.uniform(0.0, 2.0 * np.pi, N)
        gap = 10.005 - np.sqrt(100.0 - rho ** 2)
        o = np.column_stack([rho * np.cos(phi), -1.0 + 0.5 * gap, rho * np.sin(phi)]).astype(F)
        d = _unit_rows(np.column_stack([rng.uniform(-0.2, 0.2, N), -np.ones(N), rng.uniform(-0.2, 0.2, N)]))
        st = _states(rng, N)
    else:
        raise ValueError(family)
    for a in (o, d, st):
        a.setflags(write=False)
    return o, d, st


def sphere_directions(seed=family_seed("empty", "shell")):
    """N unit directions uniform on the sphere (normalised in fp32, glm order)."""
    d = _unit_rows(np.random.default_rng(seed).normal(size=(N, 3)))
    d.setflags(write=False)
    return d


def make_scene(name):
    """tests/test_gpu_radiance.py's make_scene, restated (a test module is not imported from a helper)."""
    if name == "DEFAULT+":
        scene = prt.Scene("DEFAULT")
        scene.AddMetal((0.9, 0.8, 0.7), 0.6)
        scene.AddDielectric(1.5)
        return scene
    if name == "COPIES":
        ico = prt.Mesh(prt.scenes.asset("icosahedron.ply"))
        sc = prt.Scene(preset=None)
        ground = sc.AddLambertian((0.5, 0.5, 0.5))
        light = sc.AddEmissive((15.0, 15.0, 15.0))
        mats = (sc.AddLambertian((0.8, 0.3, 0.3)), sc.AddMetal((0.9, 0.8, 0.7), 0.6), sc.AddDielectric(1.5), sc.AddMetal((0.7, 0.7, 0.9), 0.0))
        sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
        sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
        for k in range(7):
            sc.AddInstance(ico, mats[k % 4], scale=0.6 + 0.15 * k, euler_deg=(10.0 * k, 25.0 * k, 0.0),
                           translation=(2.2 * ((k % 3) - 1), 0.2 * k, 2.0 * ((k // 3) - 1)))
        return sc
    return prt.Scene(name)


def scaled_oracle_rays(name):
    return rays(name, "scaled", geometry=name.rstrip("+"))


# ---- a case, built once ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(row, scene, cam, depth, sampling, use_bvh, sources, env (EnvMap or None), osc).  Shared; not written to."""
    rw = row(name)
    c = rw["build"]()
    assert c["sources"] == rw["sources"], (name, c["sources"])
    return dict(c, row=rw, osc=orc.OracleScene(c["scene"].desc()))


def host_tables(c):
    """The cluster tables of a case from a host-only context (no GPU)."""
    h = prt.HipWavefrontRenderer(device=-1)
    h.set_light_sources("all")
    h.set_light_selection("clustered", CLUSTERS)
    h.set_scene_host_only(c["scene"])
    return lcr.read_tables(h)


@contextlib.contextmanager
def _textured_walk():
    import pytest
    with pytest.MonkeyPatch.context() as mp:
        tex.patch_walk(mp)
        yield


def replay(c, start, mode, samples=(0,), tables=None, wrong=None, stability=True):
    """The float64 replay of case c's light-sampled query over the rays `start` = (o, d) or (o, d, state); pix = ray index.
    mode "mis" | "nee" | "off".  tables: the cluster tables where the row selects by cluster."""
    rw = c["row"]
    n = len(start[0])
    args = (c["cam"], 1, 1, c["depth"], SEED, samples, mode, c["sampling"])
    kw = dict(pix=np.arange(n), use_bvh=c["use_bvh"], osc=c["osc"], stability=stability, start=start)
    with contextlib.ExitStack() as stack:
        if rw["textured"]:
            stack.enter_context(_textured_walk())
        if rw["selection"] == "clustered":
            assert tables is not None
            stack.enter_context(lcr.clustered(tables))
        if c["env"] is not None:
            assert wrong is None
            return er.replay(c["scene"], c["env"], *args, sources=c["sources"], **kw)
        if c["sources"] == "all":
            assert wrong is None
            return mr.replay(c["scene"], *args, sources="all", **kw)
        return lr.replay(c["scene"], *args, wrong=wrong, **kw)


def unstable_share(c, r):
    return er.unstable_share(r) if c["env"] is not None else lr.unstable_share(r)


def segments(r, n_samples=1):
    """Per-ray segment counts of a replay (summed over its samples)."""
    return (r.last + 1).reshape(n_samples, -1).sum(0).astype(np.uint32)


def oracle_trace(c, o, d, state, depth=None):
    """OracleScene.trace per ray: (L [n, 3] float32, segments [n] uint32, final state [n] uint32)."""
    n = len(o)
    L, seg, st = np.empty((n, 3), F), np.empty(n, np.uint32), np.empty(n, np.uint32)
    osc, bvh = c["osc"], c["use_bvh"]
    depth = c["depth"] if depth is None else depth
    for i in range(n):
        L[i], seg[i], st[i] = osc.trace(o[i], d[i], depth, int(state[i]), iterative=True, use_bvh=bvh)
    return L, seg, st


# ---- what a lit query is held to (the GPU test's comparison; raises on failure) -------------------------------------------
def check_lit(c, r, got_sum, info, n_samples=1):
    """Every stable ray within the replay's tolerance, the shadow-ray counts within the number of undecidable samples, the
    segments equal.  n_samples > 1: got_sum is the fp32 sum over the samples ascending; a ray is stable only if all of its
    samples are, and the tolerance is the samples' summed plus 4 U sum |value| for the fp32 additions.  -> a record."""
    n = len(got_sum)
    value = r.value.reshape(n_samples, n, 3)
    want = value.sum(0)
    tol = r.tol.reshape(n_samples, n, 3).sum(0)
    if n_samples > 1:
        tol = tol + 4.0 * lr.U * np.abs(value).sum(0)
    stable = r.stable.reshape(n_samples, n).all(0)
    err = np.abs(got_sum.astype(np.float64) - want)
    over = (err > tol).any(1) & stable
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / np.where(tol > 0, tol, 1e-300), 0.0)[stable]
    slack = r.n_unstable + r.n_indifferent
    rec = dict(compared=int(stable.sum()), left_out=int(n - stable.sum()), outside=int(over.sum()),
               worst_ratio=round(float(ratio.max()) if ratio.size else 0.0, 4), unstable=r.n_unstable, indifferent=r.n_indifferent,
               shadow_rays=(int(info["shadow_rays"]), r.shadow_rays), occluded=(int(info["shadow_occluded"]), r.shadow_occluded))
    print(rec, flush=True)
    assert unstable_share(c, r) <= lr.MAX_UNSTABLE, rec
    bad = np.nonzero(over)[0]
    assert bad.size == 0, (rec, bad[:8], got_sum[bad[:3]], want[bad[:3]], tol[bad[:3]])
    assert rec["compared"] >= 0.995 * n, rec
    assert abs(int(info["shadow_rays"]) - r.shadow_rays) <= slack, rec
    assert abs(int(info["shadow_occluded"]) - r.shadow_occluded) <= slack, rec
    assert np.array_equal(info["segments"], segments(r, n_samples)), rec
    return rec
