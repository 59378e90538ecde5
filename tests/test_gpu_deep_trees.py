"""Deep trees on the GPU (-m gpu): every traversal instance against the oracle's LINEAR SCAN, bit for bit, on trees of
9 .. 19 levels whose rays use the stack rows no other test reaches (tests/deep_trees.py; test_deep_trees_host.py holds
the depths and the stack needs quoted below).

    case   depth8  deepest need   what walks it
    d9        9        7          lean8_5waves (no overflow possible)
    d10      10        9          lean8_5waves + overflow list -> 4-wide tree; refitted: deep15_4waves
    d12      12       11          the same; stack_lds 5: wide11_5waves up to its row 11
    d15      15       13          the same; wide11_5waves overflows
    d16      16       15          the same, up to the LAST row of deep15_4waves; the PATH instance (15 entries) applies
    d17      17       16          host-built only: deep15_4waves overflows, the PATH instance does not apply, refits are refused
    d19      19       18          the same
    p11    1 + 10     10          inst12_4waves (six placed copies of d10)
    p12    1 + 11     11          inst12_4waves (six placed copies of an 11-level comb)

"Deepest need" is the probe ray's stack need by the host emulation's LOWER estimate; the probe is the centre pixel of the
33 x 33 camera that measure_traversal() renders, so max_stack_used on the device must reach it (capped by the
instance's own stack + 1, the entry at which it gives the ray up).

The same probe ray on the 4-wide tree (wide = 1) needs 3, 4, 42, 43, 48, 47, 54 entries (d9 .. d19, the lower estimate of
deep_trees.stack_need4, asserted by the host gate): from 12 levels on more than the 32 LDS entries of MODE 3 and the 27 of
MODE 1, so max_stack_used there can only come from MODE 1's spill rows, after the overflow list where MODE 2 / 3 run first.
At 9 and 10 levels that ray stays shallow and the figure is only printed.  The binary tree of these combs has 13 .. 23
levels: wide = 0 runs the 31-entry LDS-only binary instance, the binary spill instance (depth > 32) is NOT exercised."""
import numpy as np
import pytest

import deep_trees as dt
import scale_cases as sc
import util
from test_gpu_scale import _check_queries
from util import prt

pytestmark = pytest.mark.gpu

NEED4 = {"d9": 3, "d10": 4, "d12": 42, "d15": 43, "d16": 48, "d17": 47, "d19": 54}   # (test_deep_trees_host.py asserts these)
DEEPEST = {"d9": 7, "d10": 9, "d12": 11, "d15": 13, "d16": 15, "d17": 16, "d19": 18, "p11": 10, "p12": 11}
STACK = {"lean8_5waves": 8, "wide11_5waves": 11, "inst12_4waves": 12, "deep15_4waves": 15}


def _renderer(scene, cam, params=(), W=33, H=33, depth=5, seed=5):
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=seed)
    for k, v in params:
        r.set_param(k, v)
    film = prt.Film(W, H)
    r.Init(film, scene, cam)
    return r, film


def _queries(r, c, label):
    return _check_queries(r, c["o"], c["d"], c["want"], c["diam"], label)


def _stack_used(r, need, label):
    """measure_traversal's deepest stack of the instance in use: at least the probe ray's need, or the entry at which the
    instance hands the ray to the overflow list (its stack + 1)."""
    inst = r.kernel_instance()
    used = int(r.measure_traversal().max_stack_used)
    r.synchronize()
    print(f"   {label}: {inst}, max_stack_used {used} (probe ray needs {need})", flush=True)
    assert used >= min(need, STACK[inst] + 1), (label, inst, used, need)
    return used


@pytest.mark.parametrize("name", dt.NAMES)
def test_host_built_tree_equals_the_linear_scan_under_every_instance(name):
    """Default parameters: lean8_5waves at every depth; from 10 levels on max_stack_used >= 9 = the overflow list was used
    without the stack_cap hook, and synchronize() is clean.  Then the same rays under stack_lds 4 / 5 / 6 (deep15, wide11,
    lean8: each up to its top rows or into its overflow), steal 0 / 64, the 4-wide tree's instances (wide = 1 with
    stack_lds 0 / 1 / 2 / 3: MODE 3 with 32 entries, MODE 1, MODE 2 with 27, MODE 3 with 24, each but MODE 1 followed by the
    MODE 1 re-walk of its overflow list; from 12 levels on max_stack_used >= the probe ray's 42 .. 54 entries, which only
    MODE 1's spill rows hold), the binary tree (wide = 0: its LDS-only instance, see above) and variants 1 / 2."""
    c = dt.case_data(name)
    depth = dt.CASES[name][4]
    r, _ = _renderer(c["scene"], c["cam"])
    info = r.bvh_info()
    assert info.depth8 == depth and not info.built_on_device and r.kernel_instance() == "lean8_5waves"
    n_occ, _ = _queries(r, c, f"{name} default")
    # (at 9 levels idle lanes of a draining wave take the bottom entries of their neighbours' stacks: no floor there)
    used = _stack_used(r, DEEPEST[name] if depth >= 10 else 0, f"{name} default")
    if depth >= 10:
        assert used >= 9
    for lds, inst in ((4, "deep15_4waves"), (5, "wide11_5waves"), (6, "lean8_5waves")):
        r.set_param("stack_lds", lds)
        assert r.kernel_instance() == inst
        _queries(r, c, f"{name} stack_lds {lds}")
        _stack_used(r, DEEPEST[name] if depth >= 10 else 0, f"{name} stack_lds {lds}")
    r.set_param("stack_lds", 0)
    for steal in (0, 64):
        r.set_param("steal", steal)
        _queries(r, c, f"{name} steal {steal}")
    r.set_param("steal", 8)   # (the default)
    for wide, lds in ((1, 0), (1, 1), (1, 2), (1, 3), (0, 0)):
        r.set_param("wide", wide)
        r.set_param("stack_lds", lds)
        _queries(r, c, f"{name} wide {wide} stack_lds {lds}")
        if wide == 1:
            used4 = int(r.measure_traversal().max_stack_used)
            r.synchronize()
            print(f"   {name} wide 1 stack_lds {lds}: {r.kernel_instance()}, max_stack_used {used4} of max_stack4 {info.max_stack4} "
                  f"(probe ray needs {NEED4[name]})", flush=True)
            assert c["probe_need4"] == NEED4[name] and used4 <= info.max_stack4
            if NEED4[name] > 32:   # beyond every LDS stack of the 4-wide instances: MODE 1's spill rows, through the overflow list
                assert used4 >= NEED4[name], (name, lds, used4)
    r.set_param("wide", 2)
    r.set_param("stack_lds", 0)
    for v in (1, 2):
        r.set_variant(v)
        assert util.hits_equal(r.closest_hit(c["o"], c["d"]), c["want"]) == [], (name, "variant", v)
    r.set_variant(0)
    r.synchronize()
    print(f"{name}: depth8 {depth}, max_stack4 {info.max_stack4}, {len(c['o'])} rays x 13 configurations, occluded per tmax variant {n_occ}", flush=True)


def _moved_rays(c, mesh2):
    """The case's rays for the deformed mesh: families of its own, and its own probe."""
    return dt.scene_data(dt.mesh_scene(mesh2), c["per"], 77)


@pytest.mark.parametrize("name", ["d10", "d12", "d15", "d16"])
def test_refitted_tree_walks_its_upper_rows_and_equals_the_linear_scan(name):
    """prt_refit_meshes drops the 4-wide tree: deep15_4waves takes over, and nothing re-walks an overflow.  Refit with the
    tree's own vertices, then with a copy scaled by 1.5 and sheared: max_stack_used reaches the probe ray's need (9, 11,
    13, 15: at 15 / 16 levels rows 12 and above, at 16 the last row), hits and occlusion equal the linear scan of the new
    geometry and a fresh Init of it."""
    c = dt.case_data(name)
    mesh = c["scene"].meshes[0][0]
    r, _ = _renderer(c["scene"], c["cam"])
    r.Refit(c["scene"])
    assert r.bvh_info().refits == 1 and r.kernel_instance() == "deep15_4waves"
    _queries(r, c, f"{name} refit with its own vertices")
    used = _stack_used(r, DEEPEST[name], f"{name} refit with its own vertices")
    assert used >= (12 if dt.CASES[name][4] >= 15 else 9)
    for lds in (5, 6):   # (forced instances that the depth allows stay forced, the others fall back: see the last test)
        r.set_param("stack_lds", lds)
        _queries(r, c, f"{name} refit, stack_lds {lds}")
    r.set_param("stack_lds", 0)
    m2 = dt.deformed(mesh)
    c2 = _moved_rays(c, m2)
    r.Refit(c2["scene"])
    r.SetCamera(c2["cam"])
    assert r.bvh_info().refits == 2 and r.kernel_instance() == "deep15_4waves"
    n8 = r.bvh_read8()
    _, levels = util.check_bvh8(n8, r.bvh_read()[1])
    assert levels == dt.CASES[name][4]
    shares = dt.hit_shares(c2["fam"], c2["want"])
    assert min(shares.values()) >= sc.MIN_HIT_SHARE, shares
    _, got = _queries(r, c2, f"{name} refit deformed")
    # the probe of the deformed mesh was chosen on a fresh host tree of it; on the refitted tree (same topology as before,
    # new boxes) its need is emulated again, from the tree read back
    co, cd = util.orc.camera_rays(c2["cam"].desc(), np.array([16.5], np.float32), np.array([16.5], np.float32))
    cw = util.oracle_scene(c2["scene"]).closest_hit(co, cd, use_bvh=False, n_threads=1)
    need2 = int(dt.stack_need8(r, c2["scene"], co, cd, cw["d2"])[0])
    _stack_used(r, need2, f"{name} refit deformed")
    r2, _ = _renderer(c2["scene"], c2["cam"])
    assert util.hits_equal(r2.closest_hit(c2["o"], c2["d"]), got) == []
    print(f"{name}: refitted twice, {len(c['o'])} + {len(c2['o'])} rays", flush=True)


@pytest.mark.parametrize("name", ["d17", "d19"])
def test_refit_of_a_tree_deeper_than_16_levels_is_refused(name):
    """Without the 4-wide tree no instance holds a ray that needs more than 15 entries (the probe rays need 16 / 18), and
    such a ray used to be dropped without an error.  prt_refit_meshes returns PRT_ERR_INVALID with the depth in its
    message before it touches anything: refits stays 0, the instance stays lean8_5waves, the scene answers as before."""
    c = dt.case_data(name)
    r, _ = _renderer(c["scene"], c["cam"])
    _queries(r, c, f"{name} before the refused refit")
    for mesh in (c["scene"].meshes[0][0], dt.deformed(c["scene"].meshes[0][0])):
        with pytest.raises(prt.PrtError, match=rf"{dt.CASES[name][4]} levels.*depth8 > 16"):
            r.Refit(dt.mesh_scene(mesh))
        info = r.bvh_info()
        assert info.refits == 0 and info.depth8 == dt.CASES[name][4] and info.n_nodes4 > 0 and r.kernel_instance() == "lean8_5waves"
    _queries(r, c, f"{name} after the refused refit")
    _stack_used(r, DEEPEST[name], f"{name} after the refused refit")
    r.synchronize()


@pytest.mark.parametrize("builder", [1, 2])
@pytest.mark.parametrize("name", dt.NAMES)
def test_device_built_trees_equal_the_linear_scan(name, builder, record_property):
    """gpu_build 1 / 2 on every case: the tree read back is valid, hits and occlusion equal the linear scan, and the case is
    consistent: built on the device with at most 15 levels, or the host's tree with the host's depth."""
    c = dt.case_data(name)
    r, _ = _renderer(c["scene"], c["cam"], params=(("gpu_build", builder),))
    info = r.bvh_info()
    _, levels = util.check_bvh8(r.bvh_read8(), r.bvh_read()[1])
    assert levels == info.depth8
    if info.built_on_device:
        assert info.depth8 <= 15 and info.n_nodes4 == 0
        assert r.kernel_instance() == ("lean8_5waves" if info.depth8 <= 9 else "deep15_4waves")
    else:
        assert info.depth8 == dt.CASES[name][4] and info.n_nodes4 > 0 and r.kernel_instance() == "lean8_5waves"
    _queries(r, c, f"{name} builder {builder}")
    used = int(r.measure_traversal().max_stack_used)
    r.synchronize()
    rec = dict(case=name, builder=builder, built_on_device=int(info.built_on_device), depth8=int(info.depth8), instance=r.kernel_instance(),
               max_stack_used=used)
    record_property("deep_tree_device_build", rec)
    print(f"{rec}", flush=True)
    assert not info.built_on_device or used < info.depth8   # (the host's tree: the 4-wide re-walk's stack counts too)


@pytest.mark.parametrize("name", list(dt.PLACED))
def test_placed_copies_of_deep_meshes_equal_the_linear_scan(name):
    """inst12_4waves with top_depth + mesh depth = 11 / 12: max_stack_used >= 10 (11 in the depth-12 case: the probe ray),
    hits and occlusion equal the linear scan, synchronize() is clean; again after the copies moved, with a refit and with
    a rebuild of the top level."""
    c = dt.case_data(name)
    r, _ = _renderer(c["scene"], c["cam"])
    assert r.kernel_instance() == "inst12_4waves" and r.bvh_info().depth8 == dt.PLACED[name][2]
    _queries(r, c, name)
    used = _stack_used(r, DEEPEST[name], name)
    assert used >= 10
    m = dt.case_data(name, True)
    for k, (cc, mode) in enumerate(((m, "refit"), (c, "rebuild"), (m, "rebuild"))):
        r.UpdateInstances(cc["scene"], mode)
        r.SetCamera(cc["cam"])
        assert r.instance_update_info().updates == k + 1 and r.kernel_instance() == "inst12_4waves"
        _queries(r, cc, f"{name} after {mode} {k}")
        if mode == "rebuild":
            assert _stack_used(r, DEEPEST[name] if cc is c else cc["probe_need"], f"{name} after {mode} {k}") >= 10
        r.synchronize()
    print(f"{name}: {len(c['o'])} rays x 4 placements", flush=True)


PIPELINES = (((), None, False), ((), dict(jitter=1, rr_depth=2, clamp=4.0), False), ((("path_kernel", 2),), None, False),
             ((("path_kernel", 1),), dict(jitter=1), True))


def _lit(scene_mesh):
    """The comb over a ground quad under an emissive quad (frames need light)."""
    s = dt.mesh_scene(scene_mesh)
    s.AddQuad(30.0, 30.0, s.AddLambertian((0.5, 0.5, 0.5)), translation=(0.5, -1.0, 0.0))
    s.AddQuad(3.0, 3.0, s.AddEmissive((15.0, 15.0, 15.0)), euler_deg=(180.0, 0.0, 0.0), translation=(0.5, 3.0, 0.0))
    return s


@pytest.mark.parametrize("name,refit", [("d12", False), ("d12", True), ("d16", False), ("d16", True), ("d17", False)])
def test_frames_of_deep_trees_equal_the_linear_scan_oracle(name, refit):
    """32 x 32 and 33 x 33 (the centre pixel's primary ray is the probe ray), 2 spp, 5 segments from the probe camera: the
    plain pipeline, jitter + roulette + clamp, and path_kernel 2 / 1 (the PATH instance's 15 entries hold 16 levels: taken
    at 12 and 16 levels, host-built and refitted, not taken at 17, where the pipeline renders the frame): every pixel, the
    weights and the ray count against the oracle rendering with its linear scan.  (The 17-level tree cannot be
    refitted: the test above.)"""
    c = dt.case_data(name)
    scene = _lit(c["scene"].meshes[0][0])
    osc = util.oracle_scene(scene)
    spp, depth, seed = 2, 5, 9
    n_rays = []
    for W in (32, 33):
        cam = prt.Camera(position=c["cam"].position, front=c["cam"].front, width=W, height=W)
        want = {}
        for params, sampling, one in PIPELINES:
            r, film = _renderer(scene, cam, params, W, W, depth, seed)
            if refit:
                r.Refit(scene)
                assert r.kernel_instance() == "deep15_4waves"
            sp = r.set_sampling(**sampling) if sampling else None
            for _ in range(spp if one else 1):
                r.ProgressiveRender(1 if one else spp)
            path = r.shade_instance() == ""   # (the path route launches no shade kernel)
            r.download()
            r.synchronize()
            key = tuple(sorted(sampling.items())) if sampling else ()
            if key not in want:
                want[key] = osc.render(cam.desc(), W, W, spp=spp, max_depth=depth, seed=seed, iterative=True, use_bvh=False, n_threads=8,
                                       sampling=sp)
            a, w, n = want[key]
            nbad = int((film.accum != a).any(axis=-1).sum())
            assert nbad == 0 and np.array_equal(film.weights, w) and r.stats().rays_total == n, (name, W, params, sampling, nbad)
            assert path == (bool(params) and dt.CASES[name][4] <= 16), (name, params, path)
            n_rays.append(n)
    print(f"{name} refit {refit}: 8 frames 32x32x{spp} and 33x33x{spp}, rays {n_rays}", flush=True)


@pytest.mark.parametrize("how", ["refitted", "device-built"])
def test_no_silent_loss_without_a_four_wide_tree(how):
    """A scene without the 4-wide tree (refitted, device-built) has nothing to re-walk an overflow list with.  The stack_cap
    hook, stack_lds 6 on a tree deeper than 9 levels and stack_lds 5 on one deeper than 12 used to append the deep rays to
    that list and drop them: a miss reported with a clean synchronize().  Now the launchers ignore the hook and the forced
    instance where the tree is deeper than its stack: every combination gives the linear scan's hits (an error from
    set_param / synchronize would do as well; wrong hits with a clean synchronize never)."""
    if how == "refitted":
        c = dt.case_data("d15")
        r, _ = _renderer(c["scene"], c["cam"])
        r.Refit(c["scene"])
    else:   # the deepest case the device builder keeps (a deeper tree than 15 levels falls back to the host's, with its 4-wide tree)
        for name in ("d16", "d15"):
            c = dt.case_data(name)
            r, _ = _renderer(c["scene"], c["cam"], params=(("gpu_build", 1),))
            if r.bvh_info().built_on_device:
                break
    info = r.bvh_info()
    assert info.n_nodes4 == 0 and info.depth8 > 12   # (deeper than wide11_5waves holds: the stack_lds 5 leg bites too)
    print(f"   {how}: depth8 {info.depth8}, built_on_device {info.built_on_device}", flush=True)
    for param, value in (("stack_cap", 3), ("stack_lds", 6), ("stack_lds", 5)):
        try:
            r.set_param(param, value)
            inst = r.kernel_instance()
            got = r.closest_hit(c["o"], c["d"])
            occ = r.occluded(c["o"], c["d"], np.full(len(c["o"]), np.inf, np.float32))
            r.synchronize()
        except prt.PrtError as e:
            print(f"   {how} {param} = {value}: refused: {e}", flush=True)
        else:
            print(f"   {how} {param} = {value}: {inst}", flush=True)
            assert util.hits_equal(got, c["want"]) == [], (how, param, value, int((got["prim"] != c["want"]["prim"]).sum()))
            assert np.array_equal(occ, c["want"]["prim"] >= 0), (how, param, value)
            if info.depth8 > STACK.get(inst, 15) + 1:
                pytest.fail(f"{inst} chosen for {info.depth8} levels without a 4-wide tree")
        r.set_param(param, 0)
