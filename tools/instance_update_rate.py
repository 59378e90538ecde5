#!/usr/bin/env python3
"""What moving placed copies costs: prt_set_instance_transforms (refit, rebuild) against the only other route, a full
prt_set_scene of the moved description, and what the moved tree costs to traverse.

  python tools/instance_update_rate.py [--scenes C5I,ico10k --builders 0,1 --runs 10 --rounds 3 --out profiles/instance_update_rate.json]

Scenes: C5I (12 placed copies of the 870 k-triangle dragon, 10.44 M placed triangles) and ico10k (10,000 copies of the
icosahedron in a 40 x 40 x 40 cloud around the C3 camera's target, seen from the C3 camera).
Per scene and builder (prt_set_param("gpu_build")):
  1. update time: refit / rebuild / set_scene of random similarity transforms: HIP-event time on the context's stream and
     host wall time, median of --runs, side by side;
  2. frame time (one sample, 1920x1080) after a REBUILD of random transforms against a fresh prt_set_scene of the same
     transforms, alternating in one process, --rounds rounds; the margin is the spread of the fresh runs themselves;
  3. frame time after a REFIT of a jiggle and of a permutation, relative to a rebuild of the same transforms: the cost of
     keeping the topology (reported, not gated).
One JSON document goes to --out, and every row is printed as it is measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ico10k(prt):
    rng = np.random.default_rng(10)
    sc = prt.Scene(preset=None)
    ground, light = sc.AddLambertian((0.5, 0.5, 0.5)), sc.AddEmissive((15.0, 15.0, 15.0))
    body = [sc.AddLambertian((0.8, 0.8, 0.8)), sc.AddMetal((0.9, 0.9, 0.9), 0.05)]
    sc.AddQuad(200.0, 200.0, ground, translation=(0.0, -21.0, 0.0))
    sc.AddQuad(40.0, 40.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 30.0, 0.0))
    ico = prt.Mesh(prt.scenes.asset("icosahedron.ply"))
    srts = [(float(rng.uniform(0.2, 0.6)), tuple(float(v) for v in rng.uniform(-180, 180, 3)), tuple(float(v) for v in rng.uniform(-20, 20, 3)))
            for _ in range(10_000)]
    for k, (s, e, t) in enumerate(srts):
        sc.AddInstance(ico, body[k & 1], scale=s, euler_deg=e, translation=t)
    return sc, prt.Camera(prt.scenes.MESH_CAMERA, width=1920, height=1080), srts


def c5i(prt):
    sc, cam, *_ = prt.scenes.config("C5I")
    return sc, cam, [i.srt for i in sc.instances]


def motions(srts, rng):
    n = len(srts)
    size = max(1e-6, float(np.ptp(np.array([t for _, _, t in srts]), axis=0).max()))
    jiggle = [(s, tuple(np.asarray(e) + rng.uniform(-3, 3, 3)), tuple(np.asarray(t) + rng.uniform(-0.02, 0.02, 3) * s[0])) for s, e, t in srts]
    shift = n // 2 + 1
    permute = [(srts[k][0], srts[k][1], srts[(k + shift) % n][2]) for k in range(n)]
    rand = [(tuple(float(v * f) for v in s), tuple(rng.uniform(-180, 180, 3)), tuple(np.asarray(t) + rng.uniform(-0.1, 0.1, 3) * size))
            for (s, e, t), f in zip(srts, rng.uniform(0.7, 1.4, n))]
    return {"jiggle": jiggle, "permute": permute, "random": rand}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="C5I,ico10k")
    ap.add_argument("--builders", default="0,1")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_update_rate.json"))
    a = ap.parse_args()
    import torch

    import parallelraytracing_amd as prt
    stream = torch.cuda.Stream(device=0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    def move(scene, srts):
        for k, (s, e, t) in enumerate(srts):
            scene.SetInstanceTransform(k, scale=tuple(float(v) for v in s) if not np.isscalar(s) else s, euler_deg=tuple(float(v) for v in e),
                                       translation=tuple(float(v) for v in t))

    def renderer(scene, cam, builder):
        r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=1)
        r.set_param("gpu_build", builder)
        film = prt.Film(1920, 1080)
        r.Init(film, scene, cam)
        r.set_stream(stream.cuda_stream)
        return r, film

    def frame_ms(r, n=3):
        out = []
        for _ in range(n + 1):
            out.append(timed(lambda: (r.ProgressiveRender(1), r.synchronize()))[0])
        return float(np.median(out[1:]))

    for name in a.scenes.split(","):
        scene, cam, srts = (c5i if name.upper() == "C5I" else ico10k)(prt)
        srts = [((s, s, s) if np.isscalar(s) else s, e, t) for s, e, t in srts]
        for builder in [int(b) for b in a.builders.split(",")]:
            rng = np.random.default_rng(5)
            r, film = renderer(scene, cam, builder)
            # 1. update time
            t = {"refit": [], "rebuild": [], "set_scene": []}
            for _ in range(a.runs):
                move(scene, motions(srts, rng)["random"])
                for how in ("refit", "rebuild"):
                    t[how].append(timed(lambda: r.UpdateInstances(scene, how)))
                t["set_scene"].append(timed(lambda: r.Init(film, scene, cam)))
            info = r.instance_update_info()
            emit({"scene": name, "builder": builder, "what": "update_ms", "copies": len(srts), "triangles": scene.n_triangles,
                  "top_nodes": info.top_nodes, "top_depth": info.top_depth,
                  **{f"{k}_{w}": round(float(np.median([x[i] for x in v])), 3) for k, v in t.items() for i, w in enumerate(("event", "wall"))}})
            # 2. frames after a rebuild against a fresh scene, alternating
            move(scene, motions(srts, rng)["random"])
            reb, fresh = [], []
            for _ in range(a.rounds):
                move(scene, srts)
                r.UpdateInstances(scene, "rebuild")
                move(scene, motions(srts, np.random.default_rng(6))["random"])
                r.UpdateInstances(scene, "rebuild")
                reb.append(frame_ms(r))
                r2, _ = renderer(scene, cam, builder)
                fresh.append(frame_ms(r2))
                del r2
            emit({"scene": name, "builder": builder, "what": "frame_ms_after_rebuild", "rebuild": [round(x, 3) for x in reb],
                  "fresh_set_scene": [round(x, 3) for x in fresh], "fresh_spread": round(max(fresh) - min(fresh), 3),
                  "rebuild_minus_fresh_median": round(float(np.median(reb) - np.median(fresh)), 3)})
            # 3. the cost of a kept topology
            for what in ("jiggle", "permute"):
                m = motions(srts, np.random.default_rng(7))[what]
                move(scene, srts)
                r.UpdateInstances(scene, "rebuild")
                move(scene, m)
                r.UpdateInstances(scene, "refit")
                ran = r.instance_update_info().last_mode
                f_refit = frame_ms(r)
                r.UpdateInstances(scene, "rebuild")
                f_rebuild = frame_ms(r)
                emit({"scene": name, "builder": builder, "what": f"frame_ms_refit_{what}", "refit": round(f_refit, 3), "rebuild": round(f_rebuild, 3),
                      "refit_over_rebuild": round(f_refit / f_rebuild, 3), "refit_ran_as": "refit" if ran == 0 else "rebuild"})
            r.set_stream(0)
            del r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/instance_update_rate.py", "args": vars(a), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
