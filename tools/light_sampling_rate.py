#!/usr/bin/env python3
"""Cost of light sampling (PrtLighting) on C3: ms per 256-spp step at 1080p with lighting off, nee and mis, and shadow
rays per second.  usage: python3 tools/light_sampling_rate.py [--steps N]

--mesh-lights [--out profiles/NAME.json]: the same on a MESH-LIT scene (C3 with the dragon emissive: ~870 k triangle lights
beside the quad) for lighting off, mis with light sources "analytic" and "all", the latter with the bucketed and the plain
binary search over the thresholds (prt_set_param light_buckets 1 / 0); the two searches again on kind D's emitter as 8
triangles; and the variance of the ground pixels under "all" against "analytic" at equal samples (two seeds per
configuration, per-pixel variance estimate (X1 - X2)^2 / 2) and at equal time (x the ratio of the step times).

--light-selection power|clustered [--light-clusters N]: the selection of the "all" rows above (prt_set_light_selection).

--clusters [--rounds R] [--out profiles/NAME.json]: clustered light selection on the same mesh-lit scene, MIS: "analytic",
"all" with power selection and "all" with clustered selection at 8, 32 and 64 clusters, on ONE context whose settings are
switched, the configurations alternating R times: ms per step and shadow rays per second (median and spread over the
rounds), and the ground-pixel variance against "analytic" at equal samples and at equal time (per round two films of
independent sample indices, per-pixel variance estimate (X1 - X2)^2 / 2; median and spread of the ratio over the rounds)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallelraytracing_amd import renderer as prt, scenes  # noqa: E402


def emissive_dragon_scene():
    sc = prt.Scene(preset=None)
    ground = sc.AddLambertian((0.5, 0.5, 0.5))
    light = sc.AddEmissive((15.0, 15.0, 15.0))
    glow = sc.AddEmissive((1.0, 0.8, 0.6))
    sc.AddQuad(20.0, 20.0, ground, translation=(0.0, -1.0, 0.0))
    sc.AddQuad(4.0, 4.0, light, euler_deg=(180.0, 0.0, 0.0), translation=(0.0, 5.0, 0.0))
    sc.AddMesh(scenes.refined("dragon.ply", 870_000), glow)
    return sc


SELECTION = ("power", 32)  # --light-selection / --light-clusters


def timed(sc, cam, W, H, spp, D, steps, mode, sources, buckets=1, seed=0):
    film = prt.Film(W, H)
    r = prt.HipWavefrontRenderer(device=0, max_depth=D, seed=seed)
    r.set_param("light_buckets", buckets)
    r.set_light_sources(sources)
    r.set_light_selection(*SELECTION)
    r.Init(film, sc, cam)
    r.set_samples_in_flight(spp)
    r.set_lighting(mode)
    r.ProgressiveRender(spp)  # warm-up
    r.reset_stats()
    film.Clear()
    t0 = time.perf_counter()
    for _ in range(steps):
        r.ProgressiveRender(spp)
    r.synchronize()
    dt = (time.perf_counter() - t0) / steps
    ls = r.light_stats()
    r.download()
    rec = dict(mode=mode, sources=sources, buckets=buckets, ms_per_step=round(1e3 * dt, 2), n_lights=int(ls.n_lights),
               closest_hit_grays_s=round(r.stats().rays_total / steps / dt / 1e9, 3),
               shadow_grays_s=round(ls.shadow_rays / steps / dt / 1e9, 3),
               occluded_share=round(ls.shadow_occluded / max(ls.shadow_rays, 1), 4))
    print(rec, flush=True)
    return rec, film.accum.reshape(-1, 3).sum(1) / (steps * spp), r


def mesh_lights(a):
    import gc
    import json

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_sha import kernel_sha
    out = dict(kernel_sha16=kernel_sha(), steps=a.steps, scene="C3 with the dragon emissive (1, 0.8, 0.6), 1080p, 256 spp per step", rows=[])
    _, cam, W, H, spp, D = scenes.config("C3")
    sc = emissive_dragon_scene()
    X = {}
    for mode, sources, buckets in (("off", "analytic", 1), ("mis", "analytic", 1), ("mis", "all", 1), ("mis", "all", 0)):
        for k, seed in enumerate((0, 1000)):
            if k == 1 and (mode == "off" or buckets == 0):
                continue
            rec, x, r = timed(sc, cam, W, H, spp, D, a.steps, mode, sources, buckets, seed)
            rec["seed"] = seed
            out["rows"].append(rec)
            X[mode, sources, buckets, k] = x
            if "ground" not in X:
                px, py = np.meshgrid(np.arange(W, dtype=np.float32) + 0.5, np.arange(H, dtype=np.float32) + 0.5)
                o, d = r.camera_rays(px.ravel(), py.ravel())
                X["ground"] = r.closest_hit(o, d)["prim"] == 0
            del r
            gc.collect()  # (renderer and film refer to each other: the context's path buffers go with the cycle)
    g = X["ground"]
    t = {(r_["sources"], r_["buckets"]): r_["ms_per_step"] for r_ in out["rows"] if r_["mode"] == "mis" and r_["seed"] == 0}
    v_an = float((((X["mis", "analytic", 1, 0] - X["mis", "analytic", 1, 1])[g]) ** 2).mean() / 2.0)
    v_all = float((((X["mis", "all", 1, 0] - X["mis", "all", 1, 1])[g]) ** 2).mean() / 2.0)
    out["ground_pixels"] = int(g.sum())
    out["variance_ratio_equal_samples"] = round(v_an / v_all, 3)
    out["variance_ratio_equal_time"] = round(v_an / v_all * t["analytic", 1] / t["all", 1], 3)
    print({k: out[k] for k in ("ground_pixels", "variance_ratio_equal_samples", "variance_ratio_equal_time")}, flush=True)
    # 8 lights: kind D's emitter as triangles
    d_tri = scenes.triangulate_quads(scenes.mesh_scene(prt.Mesh(scenes.asset("icosahedron.ply"))))
    out["rows_8_lights"] = []
    for buckets in (1, 0, 1, 0):
        rec, _, r = timed(d_tri, cam, W, H, spp, D, a.steps, "mis", "all", buckets)
        out["rows_8_lights"].append(rec)
        del r
        gc.collect()
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)
        print("wrote", a.out)


def clusters(a):
    import json

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_sha import kernel_sha
    _, cam, W, H, spp, D = scenes.config("C3")
    sc = emissive_dragon_scene()
    film = prt.Film(W, H)
    r = prt.HipWavefrontRenderer(device=0, max_depth=D, seed=0)
    r.Init(film, sc, cam)
    r.set_samples_in_flight(spp)
    r.set_lighting("mis")
    px, py = np.meshgrid(np.arange(W, dtype=np.float32) + 0.5, np.arange(H, dtype=np.float32) + 0.5)
    o, d = r.camera_rays(px.ravel(), py.ravel())
    ground = r.closest_hit(o, d)["prim"] == 0
    configs = [("analytic", "power", 32), ("all", "power", 32), ("all", "clustered", 8), ("all", "clustered", 32), ("all", "clustered", 64)]
    name = lambda c: c[0] if c[1] == "power" else f"{c[0]} clustered {c[2]}"   # noqa: E731
    rows = {name(c): dict(ms=[], shadow_grays_s=[], var=[]) for c in configs}
    build_ms = {}
    for rnd in range(a.rounds):
        for c in configs:
            r.set_light_sources(c[0])
            t0 = time.perf_counter()
            r.set_light_selection(c[1], c[2])
            if rnd == 0:
                build_ms[name(c)] = round(1e3 * (time.perf_counter() - t0), 1)   # (about 0 where max_clusters did not change)
            r.ProgressiveRender(spp)  # warm-up
            X, ms, sh = [], [], []
            for half in range(2):
                film.Clear()
                r.frame_index = (2 * rnd + half) * a.steps * spp
                r.synchronize()
                r.reset_stats()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    r.ProgressiveRender(spp)
                r.synchronize()
                dt = (time.perf_counter() - t0) / a.steps
                ms.append(1e3 * dt)
                sh.append(r.light_stats().shadow_rays / a.steps / dt / 1e9)
                r.download()
                X.append(film.accum.reshape(-1, 3).sum(1).astype(np.float64) / (a.steps * spp))
            row = rows[name(c)]
            row["ms"] += ms
            row["shadow_grays_s"] += sh
            row["var"].append(float(((X[0] - X[1])[ground] ** 2).mean() / 2.0))
            row["n_lights"] = int(r.light_stats().n_lights)
            row["n_clusters"] = int(r.light_cluster_info().n_clusters) if c[1] == "clustered" else 0
            print(rnd, name(c), [round(m, 2) for m in ms], row["var"][-1], flush=True)
    med = lambda v: float(np.median(v))   # noqa: E731
    out = dict(kernel_sha16=kernel_sha(), steps=a.steps, rounds=a.rounds, ground_pixels=int(ground.sum()), cluster_build_ms=build_ms,
               scene="C3 with the dragon emissive (1, 0.8, 0.6), 1080p, 256 spp per step, MIS", rows=[])
    an = rows["analytic"]
    for c in configs:
        row = rows[name(c)]
        eq_s = [v / va for v, va in zip(row["var"], an["var"])]
        eq_t = [e * med(row["ms"]) / med(an["ms"]) for e in eq_s]
        out["rows"].append(dict(config=name(c), n_lights=row["n_lights"], n_clusters=row["n_clusters"], ms_per_step_median=round(med(row["ms"]), 2),
                                ms_per_step_min_max=[round(min(row["ms"]), 2), round(max(row["ms"]), 2)],
                                shadow_grays_s_median=round(med(row["shadow_grays_s"]), 3),
                                ground_variance_over_analytic_equal_samples=dict(median=round(med(eq_s), 3), min_max=[round(min(eq_s), 3), round(max(eq_s), 3)]),
                                ground_variance_over_analytic_equal_time=dict(median=round(med(eq_t), 3), min_max=[round(min(eq_t), 3), round(max(eq_t), 3)])))
        print(out["rows"][-1], flush=True)
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)
        print("wrote", a.out)


def main():
    global SELECTION
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--mesh-lights", action="store_true")
    ap.add_argument("--clusters", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--light-selection", choices=("power", "clustered"), default="power")
    ap.add_argument("--light-clusters", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    SELECTION = (a.light_selection, a.light_clusters)
    if a.clusters:
        return clusters(a)
    if a.mesh_lights:
        return mesh_lights(a)
    sc, cam, W, H, spp, D = scenes.config("C3")
    for mode in ("off", "nee", "mis"):
        film = prt.Film(W, H)
        r = prt.HipWavefrontRenderer(device=0, max_depth=D, seed=0)
        r.Init(film, sc, cam)
        r.set_samples_in_flight(spp)
        r.set_lighting(mode)
        r.ProgressiveRender(spp)  # warm-up
        r.reset_stats()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r.ProgressiveRender(spp)
        dt = (time.perf_counter() - t0) / a.steps
        ls = r.light_stats()
        print(f"{mode:4s} {1e3 * dt:8.1f} ms/step  closest-hit {r.stats().rays_total / a.steps / dt / 1e9:5.2f} G rays/s  "
              f"shadow {ls.shadow_rays / a.steps / dt / 1e9:5.2f} G rays/s  occluded {ls.shadow_occluded / max(ls.shadow_rays, 1):.3f}")
        del r


if __name__ == "__main__":
    main()
