#!/usr/bin/env python3
"""Randomized parity: random scenes (analytic primitives of every material, refined meshes, placed copies), random cameras,
builders, kernel tunables and sampling flags; every frame bit for bit against the oracle (throughput form) + ray counts.
--lighting: the same generators with emissive analytic primitives and light sampling, every sample against the float64 replay.
--scale: scene, camera and rays moved by a (scale, translation) drawn from tests/scale_cases.py's non-extreme table; the oracle
         then always scans linearly (its own BVH carries absolute pads).
--interface: ONE long-lived context (or a group) through generated call sequences of the whole interface, against the model of
         tests/interface_sequences.py: films, ray counts, every query's answer, and what prt_primary_reuse may say (~0.08 s per case).
  python tests/fuzz_parity.py --cases 200 --seed 1      (GPU box; ~0.3 s per case)
Test infrastructure (it calls the oracle): a checker, not a product path; tests/test_gpu_fuzz.py runs a seeded subset."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parallelraytracing_amd as prt  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import scale_cases  # noqa: E402

MESHES = {}


def mesh(name, tris):
    key = (name, tris)
    if key not in MESHES:
        m = prt.Mesh(prt.scenes.asset(name))
        MESHES[key] = m.refine(tris) if tris else m
    return MESHES[key]


def random_scene(rng):
    sc = prt.Scene(preset=None)
    mats = [sc.AddLambertian(tuple(rng.uniform(0.2, 0.9, 3))), sc.AddLambertian(tuple(rng.uniform(0.2, 0.9, 3))),
            sc.AddMetal(tuple(rng.uniform(0.5, 1.0, 3)), float(rng.choice([0.0, 0.05, 0.3]))),
            sc.AddDielectric(float(rng.choice([1.3, 1.5, 2.4]))), sc.AddEmissive(tuple(rng.uniform(2, 12, 3)))]
    pick = lambda: mats[int(rng.integers(0, len(mats)))]  # noqa: E731
    desc = []
    if rng.random() < 0.8:
        sc.AddQuad(float(rng.uniform(8, 40)), float(rng.uniform(8, 40)), mats[0], translation=(0.0, float(rng.uniform(-2.0, -0.5)), 0.0))
    if rng.random() < 0.7:
        sc.AddQuad(3.0, 3.0, mats[4], euler_deg=(180.0, 0.0, 0.0), translation=(float(rng.uniform(-2, 2)), float(rng.uniform(4, 8)), float(rng.uniform(-2, 2))))
    n_prims = int(rng.choice([0, 1, 3, 8, 20, 40]))
    for _ in range(n_prims):
        tr = tuple(float(v) for v in rng.uniform(-5, 5, 3))
        if rng.random() < 0.6:
            s = float(rng.uniform(0.3, 1.5))
            sc.AddCircle(float(rng.uniform(0.2, 1.2)), pick(), scale=(s, s, s), translation=tr)
        else:
            sc.AddQuad(float(rng.uniform(0.5, 3)), float(rng.uniform(0.5, 3)), pick(),
                       euler_deg=(float(rng.choice([0, 50, 90, 180])), 0.0, 0.0), translation=tr)
    desc.append(f"{n_prims} prims")
    kind = rng.choice(["none", "world", "inst", "both"], p=[0.1, 0.4, 0.25, 0.25])
    name, tris = [("icosahedron.ply", 0), ("icosahedron.ply", 300), ("bunny.ply", 0), ("bunny.ply", 4000), ("hand.ply", 0),
                  ("dragon.ply", 0)][int(rng.integers(0, 6))]
    world = None
    if kind in ("world", "both"):
        world = mesh(name, tris)
        sc.AddMesh(world, pick())
        desc.append(f"world {name}:{tris}")
    if kind in ("inst", "both"):
        n_inst = int(rng.integers(1, 7))
        name2, tris2 = [("icosahedron.ply", 0), ("bunny.ply", 0), ("icosahedron.ply", 1200)][int(rng.integers(0, 3))]
        for _ in range(n_inst):
            sc.AddInstance(mesh(name2, tris2), pick(), scale=float(rng.uniform(0.3, 2.5)),
                           euler_deg=tuple(float(v) for v in rng.uniform(-180, 180, 3)),
                           translation=tuple(float(v) for v in rng.uniform(-5, 5, 3)))
        desc.append(f"{n_inst} copies of {name2}:{tris2}")
    return sc, ", ".join(desc), kind, world


def draw_move(case, seed):
    """--scale: the (name, s, T) of a case, from a stream of its own (the other draws of the case stay what they are)."""
    return scale_cases.draw(np.random.default_rng([seed, case, 31337]))


def run_case(case, seed, scale=False):
    rng = np.random.default_rng([seed, case])
    scene, desc, kind, _ = random_scene(rng)
    W, H = int(rng.choice([17, 64, 96, 131])), int(rng.choice([9, 48, 72]))
    if scale and scene.n_triangles > 6000:  # (the oracle scans linearly here: keep its share of the wall time down)
        W, H = min(W, 64), min(H, 48)
    pos = rng.normal(size=3)
    pos = pos / np.linalg.norm(pos) * rng.uniform(3, 14)
    pos[1] = abs(pos[1]) + 0.3
    front = -pos + rng.uniform(-1, 1, 3)
    cam = prt.Camera(position=tuple(float(v) for v in pos), front=tuple(float(v) for v in front), width=W, height=H)
    if scale:
        mname, ms, mT = draw_move(case, seed)
        scene, cam = scale_cases.move_scene(scene, ms, mT), scale_cases.move_camera(cam, ms, mT)
        desc += f", moved {mname}"
    depth = int(rng.integers(1, 9))
    spp = int(rng.integers(1, 4))
    rseed = int(rng.integers(0, 1 << 30))
    r = prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=rseed)
    params = {}
    has_mesh = kind != "none"
    if has_mesh and rng.random() < 0.5:
        params["gpu_build"] = int(rng.choice([1, 2]))
    if rng.random() < 0.3:
        params["node_stride"] = 8
    if rng.random() < 0.3:
        params["prim_bvh"] = 0
    if rng.random() < 0.3:
        params["compact_primary"] = 0
    if rng.random() < 0.2:
        params["primary_hit"] = 0
    if rng.random() < 0.4:
        params["path_kernel"] = int(rng.choice([0, 2]))  # (1 = the default: batches of one sample)
    if rng.random() < 0.3:
        params["fuse"] = int(rng.integers(0, 2))
    if rng.random() < 0.2:
        params["exact_grids"] = int(rng.integers(0, 3))
    if rng.random() < 0.2 and kind in ("world",):
        params["stack_cap"] = int(rng.integers(2, 6))  # forces the overflow list (host-built trees only: needs the 4-wide tree)
        params.pop("gpu_build", None)
    if rng.random() < 0.25:  # the big-grab tier of the ray hand-out, forced onto small launches
        params["big"] = int(rng.choice([2, 3, 5]))
        params["big_min"] = 1
        params["big_keep"] = int(rng.choice([0, 1, 4]))
        params["chunk"] = int(rng.choice([64, 128, 256]))
    if rng.random() < 0.3:
        params["static_small"] = int(rng.choice([0, 2, 64]))  # granules dealt round-robin / through the cursor
    if rng.random() < 0.2:
        params["refill_min"] = int(rng.choice([1, 8, 32, 64]))
    if rng.random() < 0.2:
        params["tri_min"] = int(rng.choice([1, 8, 64]))
    for k, v in params.items():
        r.set_param(k, v)
    film = prt.Film(W, H)
    try:
        r.Init(film, scene, cam)
    except prt.PrtError as e:  # e.g. a tree too deep for the two-level kernel: must be a clean error
        # (a MOVED scene that is refused is a failure: the unmoved one is accepted, and the table is the supported range)
        return f"case {case}: Init refused ({str(e)[:80]}) [{desc}]", not scale
    sp = None
    if rng.random() < 0.4:
        sp = r.set_sampling(jitter=int(rng.integers(0, 2)), rr_depth=int(rng.choice([0, 1, 3])), clamp=float(rng.choice([0.0, 1.5])))
    sif = int(rng.integers(1, spp + 1))
    r.set_samples_in_flight(sif)
    r.ProgressiveRender(spp)
    r.download()
    osc = orc.OracleScene(scene.desc())
    # small meshes: the oracle scans linearly as the reference does (its own BVH only for the big ones, to stay fast)
    acc, wts, rays = osc.render(cam.desc(), W, H, spp=spp, max_depth=depth, seed=rseed, iterative=True,
                                use_bvh=scene.n_triangles > 6000 and not scale, n_threads=8, sampling=sp)
    st = r.stats()
    nbad = int((film.accum != acc).any(axis=-1).sum())
    ok = nbad == 0 and np.array_equal(film.weights, wts) and st.rays_total == rays
    msg = (f"case {case}: {'ok ' if ok else 'MISMATCH'} {W}x{H} spp {spp} depth {depth} [{desc}] params {params} sampling "
           f"{(sp.jitter, sp.rr_depth, sp.clamp) if sp else None}: {nbad} bad pixels, rays {st.rays_total} vs {rays}")
    return msg, ok


def run_ray_case(case, seed, n=4096, scale=False):
    """Closest hit of awkward rays against the oracle's BRUTE-FORCE scan: directions with zero components (infinite slab
    reciprocals), axis-parallel rays inside box planes, origins on vertices / inside the mesh / far away, near-degenerate
    directions; a random scene and builder as above."""
    rng = np.random.default_rng([seed, case, 77])
    scene, desc, kind, world = random_scene(rng)
    base = scene
    if scale:
        mname, ms, mT = draw_move(case, seed)
        scene = scale_cases.move_scene(base, ms, mT)
        desc += f", moved {mname}"
    r = prt.HipWavefrontRenderer(device=0, max_depth=2, seed=0)
    params = {}
    if kind != "none" and rng.random() < 0.5:
        params["gpu_build"] = int(rng.choice([1, 2]))
    if rng.random() < 0.3:
        params["node_stride"] = 8
    if rng.random() < 0.3:
        params["prim_bvh"] = 0
    for k, v in params.items():
        r.set_param(k, v)
    film = prt.Film(16, 16)
    r.Init(film, scene, prt.Camera(position=(5.0, 5.0, 8.0), width=16, height=16))
    o = rng.uniform(-6, 6, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    q = n // 8
    d[0:q, int(rng.integers(0, 3))] = 0.0                      # one zero component
    ax = int(rng.integers(0, 3))
    d[q:2 * q] = 0.0
    d[q:2 * q, ax] = rng.choice([-1.0, 1.0], size=q)           # axis-parallel
    o[2 * q:3 * q] = np.round(o[2 * q:3 * q] * 2) / 2           # origins on a coarse lattice (often on box planes / quads)
    d[3 * q:4 * q] *= np.float32(1e-3)                          # short direction vectors (normalised below like any other)
    d[4 * q:5 * q, 1] = rng.choice([1e-9, -1e-9, 1e-7], size=q).astype(np.float32)  # grazing the y = const quads
    o[5 * q:6 * q] *= np.float32(50.0)                          # far away, aimed at the origin
    d[5 * q:6 * q] = -o[5 * q:6 * q] + rng.normal(size=(q, 3)).astype(np.float32)
    verts = world.GetVertices() if world is not None else None
    if verts is not None and len(verts):
        sel = verts[rng.integers(0, len(verts), size=q)]
        d[6 * q:7 * q] = sel - o[6 * q:7 * q]                   # aimed exactly at mesh vertices (if the mesh is in the scene)
    d = np.stack([prt.glm_normalize(v) if np.any(v != 0) else np.array([0, 0, 1], np.float32) for v in d]).astype(np.float32)
    if scale:  # (a uniform scale and a translation leave directions alone)
        o, d = scale_cases.move_rays(o, d, ms, mT)
    got = r.closest_hit(o, d)
    want = orc.OracleScene(scene.desc()).closest_hit(o, d, use_bvh=False, n_threads=8)
    bad = []
    for f in ("prim", "front_face", "material_id", "d2", "position", "normal"):
        same = got[f] == want[f]
        if got[f].dtype.kind == "f":
            same = same | (np.isnan(got[f]) & np.isnan(want[f]))
        if not np.all(same):
            bad.append(f)
    ok = bad == []
    if not ok:
        idx = np.nonzero((got["prim"] != want["prim"]) | (got["d2"] != want["d2"]))[0]
        for i in idx[:6]:
            print(f"   ray {i}: o {o[i].tolist()} d {d[i].tolist()} got prim {got['prim'][i]} d2 {got['d2'][i]!r} front {got['front_face'][i]} "
                  f"want prim {want['prim'][i]} d2 {want['d2'][i]!r} front {want['front_face'][i]}", flush=True)
        print(f"   {len(idx)} rays differ; n_prims {len(scene.primitives)}", flush=True)
    nhit = int((got["prim"] != 0xFFFFFFFF).sum()) if got["prim"].dtype.kind == "u" else int((got["prim"] >= 0).sum())
    return f"ray case {case}: {'ok ' if ok else 'MISMATCH ' + str(bad)} [{desc}] params {params}: {nhit} of {n} hit", ok


def run_sequence_case(case, seed):
    """ONE long-lived renderer driven through a random sequence of the interface's calls (ProgressiveRender in chunks of
    any size, SetCamera, film Clear, sampling flags, samples in flight, run-time tunables, re-Init with another scene, a
    second film size, a group of 2-3 contexts on the same GPU): after every render the film must equal what the oracle
    accumulates for the same sequence (samples first_sample .. of the current camera / scene / flags added in order)."""
    rng = np.random.default_rng([seed, case, 4242])
    depth = int(rng.integers(1, 7))
    rseed = int(rng.integers(0, 1 << 30))
    use_group = rng.random() < 0.25
    k_ctx = int(rng.integers(2, 4))
    r = prt.HipWavefrontGroupRenderer([0] * k_ctx, max_depth=depth, seed=rseed) if use_group else \
        prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=rseed)
    log = [f"group x{k_ctx}" if use_group else "single"]
    state = {}

    def new_camera(W, H):
        pos = rng.normal(size=3)
        pos = pos / np.linalg.norm(pos) * rng.uniform(3, 12)
        pos[1] = abs(pos[1]) + 0.3
        return prt.Camera(position=tuple(float(v) for v in pos), front=tuple(float(v) for v in (-pos + rng.uniform(-1, 1, 3))), width=W, height=H)

    def init():
        scene, desc, kind, _ = random_scene(rng)
        W, H = int(rng.choice([17, 40, 96])), int(rng.choice([9, 33, 48]))
        film = prt.Film(W, H)
        cam = new_camera(W, H)
        if not use_group and kind != "none" and rng.random() < 0.4:
            r.set_param("gpu_build", int(rng.choice([0, 1, 2])))
        r.Init(film, scene, cam)
        state.update(scene=scene, osc=orc.OracleScene(scene.desc()), W=W, H=H, film=film, cam=cam, fi=0, sp=None,
                     acc=np.zeros((H, W, 3), np.float32), wts=np.zeros((H, W), np.float32), rays=0)
        r.set_sampling(0, 0, 0.0)
        log.append(f"Init {W}x{H} [{desc}]")

    init()
    n_ops = int(rng.integers(4, 14))
    for _ in range(n_ops):
        op = rng.choice(["render", "render", "render", "camera", "clear", "sampling", "sif", "param", "reinit"])
        if op == "render":
            k = int(rng.integers(1, 5))
            if use_group:
                r.frame_index = state["fi"]
            r.ProgressiveRender(k)
            st = state
            st["osc"].render(st["cam"].desc(), st["W"], st["H"], spp=k, first_sample=st["fi"], max_depth=depth, seed=rseed,
                             iterative=True, use_bvh=st["scene"].n_triangles > 6000, n_threads=8, accum=st["acc"],
                             weights=st["wts"], sampling=st["sp"])
            st["fi"] += k
            f = r.download()
            log.append(f"render {k}")
            if not (np.array_equal(f.accum, st["acc"]) and np.array_equal(f.weights, st["wts"])):
                nbad = int((f.accum != st["acc"]).any(axis=-1).sum())
                return f"sequence case {case}: MISMATCH after {log}: {nbad} bad pixels", False
        elif op == "camera":
            state["cam"] = new_camera(state["W"], state["H"])
            r.SetCamera(state["cam"])
            log.append("SetCamera")
        elif op == "clear":
            if use_group:
                r.Clear()
            else:
                state["film"].Clear()
                r.frame_index = 0
            state["fi"] = 0
            state["acc"][:] = 0
            state["wts"][:] = 0
            log.append("Clear")
        elif op == "sampling":
            state["sp"] = r.set_sampling(jitter=int(rng.integers(0, 2)), rr_depth=int(rng.choice([0, 1, 3])), clamp=float(rng.choice([0.0, 1.5])))
            if state["sp"].jitter == 0 and state["sp"].rr_depth == 0 and state["sp"].clamp == 0.0:
                state["sp"] = None
            log.append("sampling")
        elif op == "sif":
            r.set_samples_in_flight(int(rng.integers(1, 6)))
            log.append("sif")
        elif op == "param":
            name, val = [("fuse", int(rng.integers(0, 2))), ("exact_grids", int(rng.integers(0, 3))), ("refill_min", int(rng.choice([1, 16, 64]))),
                         ("tri_min", int(rng.choice([1, 24, 64]))), ("compact_primary", int(rng.integers(0, 2))), ("steal", int(rng.choice([0, 8]))),
                         ("primary_hit", int(rng.integers(0, 2))),
                         ("path_kernel", int(rng.integers(0, 3)))][int(rng.integers(0, 8))]
            r.set_param(name, val)
            log.append(f"{name}={val}")
        else:
            init()
    return f"sequence case {case}: ok  {log}", True


# ---- the whole interface on one long-lived context (tests/interface_sequences.py: the model, the generator) ---------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hits_bad(got, want):
    bad = []
    for f in ("prim", "front_face", "material_id", "d2", "position", "normal"):
        same = got[f] == want[f]
        if got[f].dtype.kind == "f":
            same = same | (np.isnan(got[f]) & np.isnan(want[f]))
        if not np.all(same):
            bad.append(f)
    return bad


def interface_query(r, m, kind, n, rseed):
    """One query (interface_sequences.QUERIES) on renderer r, its answer against the oracle's for the model m's scene and
    camera.  The model learns of the call (a measurement is an instrumented batch, the chunked radiance query a set_param).
    -> a list of what differs, empty if nothing does."""
    import interface_sequences as iseq
    bad = []
    rng = np.random.default_rng([int(rseed), 31])
    o, d = iseq.query_rays(rseed, n)
    if kind.startswith("measure_"):
        m.measure(kind)
    else:
        m.query(kind)
    if kind == "camera_rays":
        px, py = rng.uniform(0, m.W, n).astype(np.float32), rng.uniform(0, m.H, n).astype(np.float32)
        go, gd = r.camera_rays(px, py)
        wo, wd = orc.camera_rays(m.cam.desc(), px, py)
        if not (np.array_equal(_bits(go), _bits(wo)) and np.array_equal(_bits(gd), _bits(wd))):
            bad.append("camera_rays")
    elif kind == "closest_hit":
        bad += ["closest_hit." + f for f in _hits_bad(r.closest_hit(o, d), m.closest_hit(o, d))]
    elif kind == "closest_hit_device":
        import torch
        dev = torch.device("cuda", 0)
        got = prt.hits_to_numpy(r.closest_hit_device(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
        bad += ["closest_hit_device." + f for f in _hits_bad(got, m.closest_hit(o, d))]
    elif kind == "occluded":
        want = m.closest_hit(o, d)
        t = iseq.occlusion_tmax(rseed, want)
        got = r.occluded(o, d, t)
        if got.dtype != bool or not np.array_equal(got, iseq.occlusion_contract(want, t, d)):
            bad.append("occluded")
    elif kind == "radiance":
        state = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        L, seg, st = m.trace(o, d, state)
        _, info = r.radiance(o, d, rng_state=state, return_info=True)
        if not (np.array_equal(_bits(info["sum"]), _bits(L)) and np.array_equal(info["segments"], seg) and np.array_equal(info["rng_state"], st)):
            bad.append("radiance")
    elif kind == "radiance_chunked":   # 3 samples, one per launch: prt_set_param bumps a generation
        r.set_param("radiance_chunk", 1)
        m.set_param("radiance_chunk", 1)
        first = int(rng.integers(0, 1000))
        want, segs = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        for s in range(3):   # sample s of ray i is the path of path_seed(i, first_sample + s, seed); the sum in sample order
            L, seg, _ = m.trace(o, d, m.path_seeds(n, first + s))
            want = (want + L).astype(np.float32)
            segs += seg
        _, info = r.radiance(o, d, samples=3, first_sample=first, return_info=True)
        if not (np.array_equal(_bits(info["sum"]), _bits(want)) and np.array_equal(info["segments"], segs)):
            bad.append("radiance_chunked")
    elif kind == "scatter":
        hits = m.closest_hit(o, d)
        sel = hits["prim"] >= 0
        if sel.any():
            state = rng.integers(0, 2 ** 32, int(sel.sum()), dtype=np.uint64).astype(np.uint32)
            got = r.scatter(d[sel], hits[sel], state)
            want = orc.scatter_batch(list(m.scene.materials), d[sel], hits[sel], state)
            names = ("scattered", "attenuation", "emitted", "origin", "dir", "rng_state")
            bad += ["scatter." + nm for nm, g, w in zip(names, got, want) if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f")]
    elif kind == "render_features":
        import denoise_replay as dr
        got = r.render_features()
        px, py = iseq.pixel_centres(m.W, m.H)
        co, cd = orc.camera_rays(m.cam.desc(), px, py)
        want = dr.features_from_hits(m.closest_hit(co, cd), m.scene, m.W, m.H)
        if not np.array_equal(got["prim"], want["prim"]):
            bad.append("render_features.prim")
        bad += ["render_features." + k for k in ("normal", "position", "depth", "albedo") if not np.array_equal(got[k], want[k], equal_nan=True)]
    elif kind == "display":
        if m.known and not m.group:
            disp = r.UpdateDisplay().astype(np.int32)
            diff = np.abs(disp - orc.tonemap(m.acc, m.wts).astype(np.int32))
            if diff.max() > 1:   # (powf on the GPU against glibc's: one lsb, tests/test_gpu_parity.py)
                bad.append(f"display: off by {int(diff.max())}")
        else:
            r.UpdateDisplay()
    elif kind == "download":
        f = r.download()
        if m.known and not (np.array_equal(f.accum, m.acc) and np.array_equal(f.weights, m.wts)):
            bad.append("download")
    elif kind == "stats":
        got = int(r.stats().rays_total)
        if m.known and got != m.rays:
            bad.append(f"stats: {got} rays, the oracle {m.rays}")
        r.reset_stats()
        m.reset_stats()
        if r.stats().rays_total != 0:
            bad.append("reset_stats")
    elif kind == "occupancy":
        a, b = bytes(r.kernel_occupancy()), bytes(r.kernel_occupancy())
        if a != b or not any(a):
            bad.append("kernel_occupancy")
    elif kind == "bvh_read8":
        if r.bvh_info().n_nodes8:
            if not np.array_equal(r.bvh_read8(), r.bvh_read8()):
                bad.append("bvh_read8")
    elif kind == "measure_traversal":
        st = r.measure_traversal(sample=3)
        _, _, rays = m.osc.render(m.cam.desc(), m.W, m.H, spp=1, first_sample=3, max_depth=m.depth, seed=m.seed, iterative=True,
                                  use_bvh=m.use_bvh, n_threads=8, sampling=m.sp)
        if m.covered and int(st.rays_total) != rays:
            bad.append(f"measure_traversal: {int(st.rays_total)} rays, the oracle {rays}")
    elif kind == "measure_shade_divergence":
        if r.measure_shade_divergence(sample=3).shape != (r.max_depth, 16):
            bad.append("measure_shade_divergence")
    else:
        raise ValueError(kind)
    return bad


def check_batches(r, recs, what=""):
    """After a call that ran the batches `recs` (the model's records): what prt_primary_reuse says of the LAST of them against
    its verdict.  -> a list of complaints."""
    import interface_sequences as iseq
    if not recs or not hasattr(r, "primary_reuse"):
        return []
    active, v = r.primary_reuse()[0], recs[-1]["verdict"]
    if (v == iseq.MUST_NOT and active != 0) or (v == iseq.MUST and active != 1):
        return [f"{what}: primary_reuse {active} where the model says '{v}' (setters {recs[-1]['setters']}, queries {recs[-1]['queries']})"]
    return []


def excursion_switch(r, kind, on, scene_kind=None):
    """Turns one of the features the oracle does not cover on or off (interface_sequences.EXCURSIONS)."""
    import interface_sequences as iseq
    if kind == "lens":
        r.set_lens(aperture=0.05, focus_distance=3.0) if on else r.set_lens()
    elif kind == "environment":
        r.set_environment(iseq.environment_image() if on else None)
    elif kind == "textures":
        r.set_textures(iseq.cube_uv_scene(textured=True) if on else None)
    elif kind == "mis":
        r.set_lighting("mis" if on else "off")
    elif kind == "adaptive":
        r.set_film_statistics(on)


def _excursion_render(r, kind, k):
    if kind == "adaptive":
        info = r.render_adaptive(0.05, min_spp=k, step_spp=k, max_spp=2 * k, noise_floor=0.01)
        passes = int(info.passes)
    else:
        r.ProgressiveRender(k)
        passes = 0
    f = r.download()
    return f.accum.copy(), f.weights.copy(), passes


def run_excursion(r, m, kind, k):
    """Clear / feature on / render / feature off / Clear on the long-lived context, and the same from scratch on a fresh one
    (same scene, camera, film, depth, seed, sampling flags; its own tunables): the two films must be equal byte for byte."""
    import interface_sequences as iseq
    bad = []
    r.film.Clear()
    r.frame_index = 0
    excursion_switch(r, kind, True)
    acc, wts, passes = _excursion_render(r, kind, k)
    recs = iseq.excursion_model(m, kind, k, listed_passes=min(passes, 1))
    if kind != "adaptive" or passes <= 1:   # (the model logged one listed pass at the most; the last batch is what is asked)
        bad += check_batches(r, recs, f"excursion {kind}")
    sp, sif = m.sp, m.sif

    def from_scratch():
        fresh = prt.HipWavefrontRenderer(device=0, max_depth=m.depth, seed=m.seed)
        fresh.Init(prt.Film(m.W, m.H), m.scene, m.cam)
        fresh.set_param("primary_reuse", 0)
        fresh.set_samples_in_flight(sif)
        if sp is not None:
            fresh.set_sampling(sp.jitter, sp.rr_depth, sp.clamp)
        excursion_switch(fresh, kind, True)
        return _excursion_render(fresh, kind, k)

    acc2, wts2, passes2 = from_scratch()
    if not (np.array_equal(_bits(acc), _bits(acc2)) and np.array_equal(wts, wts2) and passes == passes2):
        acc3, wts3, _ = from_scratch()   # (do two fresh contexts agree with each other?  If not, the call is not deterministic)
        bad.append(f"excursion {kind} ({k} samples): {int((acc != acc2).any(axis=-1).sum())} pixels differ from a fresh context's, passes "
                   f"{passes} / {passes2}; two fresh contexts {'agree' if np.array_equal(_bits(acc2), _bits(acc3)) else 'DIFFER'}")
    excursion_switch(r, kind, False)
    r.film.Clear()
    r.frame_index = 0
    r.reset_stats()
    m.reset_stats()
    return bad


def run_interface_case(case, seed):
    """interface_sequences.generate(seed, case) on ONE long-lived context (or a group of 2-3, which takes the setters only) and
    on the model: after every render the film and the ray count equal the oracle's and prt_primary_reuse agrees with the model's
    verdict; after every query its answer equals the oracle's; an excursion's film equals a fresh context's."""
    import interface_sequences as iseq
    head, ops = iseq.generate(seed, case)
    depth, rseed, use_group = head["depth"], head["seed"], head["group"]
    r = prt.HipWavefrontGroupRenderer([0] * head["k_ctx"], max_depth=depth, seed=rseed) if use_group else \
        prt.HipWavefrontRenderer(device=0, max_depth=depth, seed=rseed)
    m = iseq.Model(depth, rseed, use_group)
    state, log = {}, [f"group x{head['k_ctx']}" if use_group else "single"]
    try:
        return _run_interface_ops(case, ops, r, m, use_group, state, log)
    except prt.PrtError as e:  # (it may be a device fault: main() runs nothing after it)
        return f"interface case {case}: LIBRARY ERROR {str(e)[:300]} after {log}", False


def _run_interface_ops(case, ops, r, m, use_group, state, log):
    import interface_sequences as iseq
    for op in ops:
        k = op[0]
        log.append(" ".join(str(x) for x in op[:3]))
        bad = []
        if k == "init":
            scene, cam = iseq.apply_setter(m, op, state)
            film = prt.Film(op[2], op[3])
            try:
                r.Init(film, scene, cam)
            except prt.PrtError as e:  # e.g. a tree too deep for the two-level kernel: must be a clean error
                return f"interface case {case}: Init refused ({str(e)[:80]}) after {log}", True
            r.set_sampling(0, 0, 0.0)
            if not use_group:
                r.reset_stats()
                m.reset_stats()
        elif k == "render":
            before = int(r.stats().rays_total) if use_group else 0
            if use_group:
                r.frame_index = m.fi
            r.ProgressiveRender(op[1])
            rays0 = m.rays
            recs = m.render(op[1])
            f = r.download()
            if m.known:
                if not (np.array_equal(f.accum, m.acc) and np.array_equal(f.weights, m.wts)):
                    bad.append(f"{int((f.accum != m.acc).any(axis=-1).sum())} bad pixels")
                got = int(r.stats().rays_total)
                if (got - before != m.rays - rays0) if use_group else (got != m.rays):
                    bad.append(f"rays {got - before} vs the oracle's {m.rays - rays0 if use_group else m.rays}")
            bad += check_batches(r, recs, "render")
        elif k == "query":
            bad = interface_query(r, m, op[1], op[2], op[3])
        elif k == "excursion":
            bad = run_excursion(r, m, op[1], op[2])
        else:
            res = iseq.apply_setter(m, op, state)
            if k == "camera":
                r.SetCamera(res)
            elif k == "clear":
                if use_group:
                    r.Clear()
                else:
                    r.film.Clear()
                    r.frame_index = 0
            elif k == "sampling":
                r.set_sampling(*op[1:])
            elif k == "sif":
                r.set_samples_in_flight(op[1])
            elif k == "param":
                r.set_param(op[1], op[2])
            elif k == "max_depth":
                r.max_depth = op[1]
            elif k == "refit":
                r.Refit(res)
            elif k == "instances":
                r.UpdateInstances(res)
            elif k == "set_film":
                r.set_film(prt.Film(op[1], op[2]))
                r.SetCamera(res)
        if bad:
            return f"interface case {case}: MISMATCH {bad} after {log}", False
    return f"interface case {case}: ok  {log}", True


def run_graze_case(case, seed, n=100_000):
    """Spheres only, more than 16 of them (so the walk over their world boxes runs), rays aimed to graze them within a few
    rounding margins of the reference's discriminant (2e-7 * dist^2 / R), from 0.5 ... 2000 units away, random radii down
    to 0.01 and scales; against the oracle's linear scan."""
    rng = np.random.default_rng([seed, case, 991])
    sc = prt.Scene(preset=None)
    mat = sc.AddLambertian((0.7, 0.7, 0.7))
    k = int(rng.integers(17, 120))
    centres, radii = [], []
    spread = float(rng.choice([2.0, 8.0, 40.0]))
    for _ in range(k):
        c = rng.uniform(-spread, spread, 3)
        s = float(np.exp(rng.uniform(np.log(0.1), np.log(3.0))))
        r = float(np.exp(rng.uniform(np.log(0.01), np.log(1.0))))
        sc.AddCircle(r, mat, scale=(s, s, s), translation=tuple(float(v) for v in c))
        centres.append(c)
        radii.append(r * s)
    if rng.random() < 0.3:  # the classic ground: one huge sphere
        sc.AddCircle(1000.0, mat, translation=(0.0, -1000.0 - spread, 0.0))
    centres, radii = np.array(centres), np.array(radii)
    i = rng.integers(0, k, n)
    lo, hi = [(0.5, 30.0), (5.0, 300.0), (30.0, 2000.0)][int(rng.integers(0, 3))]
    dist = np.exp(rng.uniform(np.log(lo), np.log(hi), n)) + radii[i] * 1.01
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = rng.normal(size=(n, 3))
    v -= (v * u).sum(1, keepdims=True) * u
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    m = rng.uniform(-3e-7, 6e-7, n) * dist * dist / radii[i]
    ang = np.arcsin(np.clip((radii[i] + m) / dist, 0.0, 1.0))
    o = (centres[i] + u * dist[:, None]).astype(np.float32)
    d = (-u * np.cos(ang)[:, None] + v * np.sin(ang)[:, None]).astype(np.float32)
    inv = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    d = (d * inv[:, None]).astype(np.float32)  # (x * (1 / sqrt(dot)): glm's normalize, vectorised)
    r = prt.HipWavefrontRenderer(device=0, max_depth=2, seed=0)
    r.Init(prt.Film(16, 16), sc, prt.Camera(position=(5.0, 5.0, 8.0), width=16, height=16))
    got = r.closest_hit(o, d)
    want = orc.OracleScene(sc.desc()).closest_hit(o, d, use_bvh=False, n_threads=16)
    bad = []
    for f in ("prim", "front_face", "material_id", "d2", "position", "normal"):
        same = got[f] == want[f]
        if got[f].dtype.kind == "f":
            same = same | (np.isnan(got[f]) & np.isnan(want[f]))
        if not np.all(same):
            bad.append(f)
    oo, dd = o.astype(np.float64), d.astype(np.float64)
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    miss_by = np.linalg.norm(np.cross(oo - centres[i], dd), axis=1) - radii[i]
    phantom = int(((want["prim"] == i) & (miss_by > 1e-6 * dist)).sum())
    ok = bad == []
    return f"graze case {case}: {'ok ' if ok else 'MISMATCH ' + str(bad)} {k} spheres, spread {spread}, dist {lo}..{hi}: {phantom} phantom hits in {n} rays", ok


def run_graze_quads_case(case, seed, n=100_000, cos_lo=1e-5, cos_hi=0.08):
    """More than 16 quads (so the walk over the primitives' world boxes runs), rays that graze a quad's plane, travel along
    one of its edges and cross the plane within a few rounding errors (3u * dist / cos) of it; against the linear scan.
    Returns the message, ok, and the cosines of incidence of the rays that differ."""
    rng = np.random.default_rng([seed, case, 555])
    sc = prt.Scene(preset=None)
    mat = sc.AddLambertian((0.7, 0.7, 0.7))
    k = int(rng.integers(17, 60))
    quads = []
    for _ in range(k):
        c = rng.uniform(-6, 6, 3)
        w, h = float(rng.uniform(0.5, 4.0)), float(rng.uniform(0.5, 4.0))
        ex = float(rng.choice([0.0, 50.0, 90.0, 180.0, float(rng.uniform(0, 360))]))
        sc.AddQuad(w, h, mat, euler_deg=(ex, 0.0, 0.0), translation=tuple(float(v) for v in c))
        a = np.radians(ex)
        R = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        quads.append((c, w, h, R))
    i = rng.integers(0, k, n)
    C = np.array([quads[j][0] for j in i])
    Wd = np.array([quads[j][1] for j in i])
    Hd = np.array([quads[j][2] for j in i])
    Rm = np.array([quads[j][3] for j in i])
    ax = Rm[:, :, 0]          # local x in world
    nz = Rm[:, :, 2]          # local z in world
    nrm = Rm[:, :, 1]         # local y (the normal)
    along_x = rng.random(n) < 0.5
    eu = np.where(along_x[:, None], ax, nz)                     # edge direction
    outw = np.where(along_x[:, None], nz, ax) * rng.choice([-1.0, 1.0], (n, 1))
    half_out = np.where(along_x, Hd, Wd) * 0.5
    half_along = np.where(along_x, Wd, Hd) * 0.5
    dist = np.exp(rng.uniform(np.log(0.5), np.log(40.0), (n, 1)))
    cosi = np.exp(rng.uniform(np.log(cos_lo), np.log(cos_hi), (n, 1)))
    psi = rng.uniform(-0.08, 0.08, (n, 1))
    err = 3 * 6e-8 * dist / cosi
    off = rng.uniform(-1.0, 3.0, (n, 1)) * err
    cross_pt = C + eu * (rng.uniform(-0.8, 0.8, (n, 1)) * half_along[:, None]) + outw * (half_out[:, None] + off)
    g = eu * np.cos(psi) + outw * np.sin(psi)
    d = g * np.sqrt(1 - cosi ** 2) - nrm * cosi * rng.choice([-1.0, 1.0], (n, 1))
    o = (cross_pt - d * dist).astype(np.float32)
    d = d.astype(np.float32)
    inv = (1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])).astype(np.float32)
    d = (d * inv[:, None]).astype(np.float32)
    r = prt.HipWavefrontRenderer(device=0, max_depth=2, seed=0)
    r.Init(prt.Film(16, 16), sc, prt.Camera(position=(5.0, 5.0, 8.0), width=16, height=16))
    got = r.closest_hit(o, d)
    want = orc.OracleScene(sc.desc()).closest_hit(o, d, use_bvh=False, n_threads=16)
    diff = (got["prim"] != want["prim"]) | ~((got["d2"] == want["d2"]) | (np.isnan(got["d2"]) & np.isnan(want["d2"])))
    bad = np.nonzero(diff)[0]
    ok = len(bad) == 0
    extra = "" if ok else f"; cosines of the differing rays: min {cosi[bad, 0].min():.2e} max {cosi[bad, 0].max():.2e}"
    return f"quad graze case {case}: {'ok ' if ok else 'MISMATCH'} {k} quads, {len(bad)} of {n} rays differ{extra}", ok, cosi[bad, 0]


def lighting_draw(rng):
    """A random scene, camera, frame and settings for a light-sampled render (run_lighting_case)."""
    scene, desc, kind, _ = random_scene(rng)
    # with random probability analytic primitives become emitters; sometimes one with a transform outside the light set
    e2 = scene.AddEmissive(tuple(rng.uniform(1, 8, 3)))
    turned = 0
    for p in scene.primitives[1:]:
        if rng.random() < 0.15:
            p.material_id = e2
            turned += 1
    if rng.random() < 0.3:
        scene.AddCircle(float(rng.uniform(0.3, 0.8)), e2, scale=(1.5, 1.0, 0.7), translation=tuple(float(v) for v in rng.uniform(-4, 4, 3)))
        desc += ", a stretched emitter"
    desc += f", {turned} turned emissive"
    W, H = int(rng.choice([64, 96, 131])), int(rng.choice([48, 72]))
    pos = rng.normal(size=3)
    pos = pos / np.linalg.norm(pos) * rng.uniform(3, 14)
    pos[1] = abs(pos[1]) + 0.3
    front = -pos + rng.uniform(-1, 1, 3)
    cam = prt.Camera(position=tuple(float(v) for v in pos), front=tuple(float(v) for v in front), width=W, height=H)
    depth = int(rng.integers(2, 9))
    rseed = int(rng.integers(0, 1 << 30))
    mode = str(rng.choice(["mis", "nee"]))
    smp = (0, 0, 0.0)
    if rng.random() < 0.5:
        smp = (int(rng.integers(0, 2)), int(rng.choice([0, 1, 3])), float(rng.choice([0.0, 1.5])))
    params = {}
    if kind != "none" and rng.random() < 0.5:
        params["gpu_build"] = int(rng.choice([1, 2]))
    if rng.random() < 0.3:
        params["node_stride"] = 8
    if rng.random() < 0.3:
        params["prim_bvh"] = 0
    if rng.random() < 0.2:
        params["exact_grids"] = int(rng.integers(0, 3))
    if rng.random() < 0.3:
        params["steal"] = 0
        params["tail"] = 0
    if rng.random() < 0.25:
        params["big"] = int(rng.choice([2, 3, 5]))
        params["big_min"] = 1
        params["big_keep"] = int(rng.choice([0, 1, 4]))
        params["chunk"] = int(rng.choice([64, 128, 256]))
    if rng.random() < 0.3:
        params["static_small"] = int(rng.choice([0, 2, 64]))
    samples = (0, int(rng.integers(1, 40)))
    sif = int(rng.choice([1, 2, 16]))
    return dict(scene=scene, desc=desc, cam=cam, W=W, H=H, depth=depth, seed=rseed, mode=mode, sampling=smp, params=params,
                samples=samples, sif=sif)


def run_lighting_case(case, seed, render=True):
    """A random scene with emissive analytic primitives, rendered with light sampling (random mode, sampling flags, tunables
    and batching), every sample of every pixel against the float64 per-path replay of tests/lighting_replay.py.  A draw whose
    share of undecidable light samples exceeds the replay's cap is redrawn.  -> (message, ok, redraws).
    render=False: the reference side alone (no GPU), to measure the redraw rate."""
    import lighting_replay as lr
    for attempt in range(5):
        rng = np.random.default_rng([seed, case, 8086, attempt])
        c = lighting_draw(rng)
        osc = orc.OracleScene(c["scene"].desc())
        rep = lr.replay(c["scene"], c["cam"], c["W"], c["H"], c["depth"], c["seed"], c["samples"], c["mode"], c["sampling"],
                        use_bvh=c["scene"].n_triangles > 6000, osc=osc)
        if lr.unstable_share(rep) <= lr.MAX_UNSTABLE:
            break
    else:
        return f"lighting case {case}: no draw within the cap in 5 attempts", False, 5
    head = (f"lighting case {case}: {c['W']}x{c['H']} depth {c['depth']} {c['mode']} [{c['desc']}] params {c['params']} sampling "
            f"{c['sampling']} lights {rep.lights.n} light samples {rep.n_light_samples} occluded {rep.shadow_occluded} "
            f"unstable {rep.n_unstable} redraws {attempt}")
    if not render:
        return head, True, attempt
    r = prt.HipWavefrontRenderer(device=0, max_depth=c["depth"], seed=c["seed"])
    for k, v in c["params"].items():
        r.set_param(k, v)
    film = prt.Film(c["W"], c["H"])
    try:
        r.Init(film, c["scene"], c["cam"])
    except prt.PrtError as e:  # e.g. a tree too deep for the two-level kernel: must be a clean error
        return f"lighting case {case}: Init refused ({str(e)[:80]}) [{c['desc']}]", True, attempt
    r.set_samples_in_flight(c["sif"])
    r.set_lighting(c["mode"])
    if c["sampling"] != (0, 0, 0.0):
        r.set_sampling(*c["sampling"])
    r.reset_stats()
    frames = lr.render_samples(r, film, c["samples"])
    r.synchronize()
    try:
        rec = lr.check_against_gpu(rep, frames, r.light_stats(), r.light_info(), quiet=True)
    except AssertionError as e:
        return f"{head}: MISMATCH {str(e)[:400]}", False, attempt
    return f"{head}: ok, worst error / tolerance {rec['worst_ratio']}", True, attempt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--sequences", action="store_true", help="random call sequences on one long-lived renderer (or a group of contexts)")
    ap.add_argument("--interface", action="store_true", help="the whole interface on one long-lived renderer against the model of tests/interface_sequences.py")
    ap.add_argument("--graze", action="store_true", help="rays grazing spheres within the reference's rounding margins (walk over the primitives' boxes)")
    ap.add_argument("--graze-quads", action="store_true", help="rays grazing quads along their edges (walk over the primitives' boxes)")
    ap.add_argument("--cos-lo", type=float, default=1e-5, help="--graze-quads: smallest cosine of incidence")
    ap.add_argument("--rays", action="store_true", help="closest-hit cases with awkward rays against the brute-force scan")
    ap.add_argument("--lighting", action="store_true", help="light-sampled frames against the float64 per-path replay")
    ap.add_argument("--no-render", action="store_true", help="--lighting: the reference side alone (no GPU): redraw rate")
    ap.add_argument("--scale", action="store_true", help="frames and --rays: move scene, camera and rays by a (scale, translation) of tests/scale_cases.py")
    a = ap.parse_args()
    t0 = time.time()
    bad = 0
    for case in range(a.first, a.first + a.cases):
        msg, ok = (run_lighting_case(case, a.seed, render=not a.no_render)[:2] if a.lighting else
                   run_ray_case(case, a.seed, scale=a.scale) if a.rays else run_sequence_case(case, a.seed) if a.sequences else
                   run_interface_case(case, a.seed) if a.interface else
                   run_graze_case(case, a.seed) if a.graze else
                   run_graze_quads_case(case, a.seed, cos_lo=a.cos_lo)[:2] if a.graze_quads else run_case(case, a.seed, scale=a.scale))
        if not ok:
            bad += 1
        if "LIBRARY ERROR" in msg:
            print(msg, flush=True)
            print(f"fuzz_parity: stopped at case {case}: the library reported an error", flush=True)
            sys.exit(2)
        if a.verbose or not ok or "refused" in msg:
            print(msg, flush=True)
        if (case - a.first) % 25 == 24:
            print(f"... {case - a.first + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    print(f"fuzz_parity: {a.cases} cases from {a.first} (seed {a.seed}): {bad} mismatches, {time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
