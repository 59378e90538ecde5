#!/usr/bin/env python3
"""What film statistics and tile-adaptive sampling cost and save: C3 (the 870 k-triangle dragon, depth 5) at a reduced size.

  python tools/adaptive_rate.py [--width 960 --height 540 --min-spp 16 --step-spp 16 --max-spp 128 --sif 16
                                 --thresholds 0.05,0.02 --noise-floor 0.01 --triangles 870000 --out profiles/adaptive_rate.json]

1. A uniform render of --max-spp samples with statistics off, then with statistics on: ms per step (wall) and accumulate ms
   (HIP events, prt_enable_timing), median of --steps steps after one warm-up step.  The yardstick is the statistics-off run
   of the same build; it is measured again at the end, and the difference between its two rows is the spread.
2. An adaptive render at each threshold: wall time of the call, pixel-samples, passes, tiles at the cap, and the largest
   finite noise_map value next to the uniform frame's.
One JSON document goes to --out, and every row is printed as it is measured.  No threshold is set in advance."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--step-spp", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=128)
    ap.add_argument("--sif", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--thresholds", default="0.05,0.02")
    ap.add_argument("--noise-floor", type=float, default=0.01)
    ap.add_argument("--triangles", type=int, default=870_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_rate.json"))
    a = ap.parse_args()

    import parallelraytracing_amd as prt
    scene = prt.scenes.mesh_scene(prt.scenes.refined("dragon.ply", a.triangles))
    cam = prt.Camera(prt.scenes.MESH_CAMERA, width=a.width, height=a.height)
    film = prt.Film(a.width, a.height)
    r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=1)
    r.Init(film, scene, cam)
    r.set_samples_in_flight(a.sif)
    r.enable_timing(True)
    rows = []

    def finite_max(m):
        f = m[np.isfinite(m)]
        return float(f.max()) if f.size else None

    def uniform(name, stats):
        r.set_film_statistics(stats)
        wall, acc = [], []
        for k in range(a.steps + 1):
            film.Clear()
            r.frame_index = 0
            r.reset_stats()
            t0 = time.perf_counter()
            r.ProgressiveRender(a.max_spp)
            dt = (time.perf_counter() - t0) * 1e3
            st = r.stats()
            if k:
                wall.append(dt)
                acc.append(st.accumulate_ms)
        row = dict(setting=name, spp=a.max_spp, ms_per_step=float(np.median(wall)), accumulate_ms=float(np.median(acc)),
                   pixel_samples=a.max_spp * a.width * a.height)
        if stats:
            row["noise_max"] = finite_max(r.noise_map(a.noise_floor))
        rows.append(row)
        print(json.dumps(row), flush=True)

    uniform("uniform, statistics off", False)
    uniform("uniform, statistics on", True)
    for thr in (float(t) for t in a.thresholds.split(",")):
        wall = []
        for k in range(a.steps + 1):
            film.Clear()
            r.frame_index = 0
            r.reset_stats()
            t0 = time.perf_counter()
            info = r.render_adaptive(thr, a.min_spp, a.step_spp, a.max_spp, a.noise_floor)
            dt = (time.perf_counter() - t0) * 1e3
            if k:
                wall.append(dt)
        row = dict(setting=f"adaptive, threshold {thr:g}", ms_per_call=float(np.median(wall)), passes=int(info.passes),
                   pixel_samples=int(info.pixel_samples), tiles=int(info.tiles_local), tiles_capped=int(info.tiles_capped),
                   min_tile_spp=int(info.min_tile_spp), max_tile_spp=int(info.max_tile_spp),
                   noise_max=finite_max(r.noise_map(a.noise_floor)), rays_total=int(r.stats().rays_total))
        rows.append(row)
        print(json.dumps(row), flush=True)
    uniform("uniform, statistics off (again)", False)
    doc = dict(config=dict(scene="C3", width=a.width, height=a.height, depth=5, triangles=a.triangles, min_spp=a.min_spp,
                           step_spp=a.step_spp, max_spp=a.max_spp, samples_in_flight=a.sif, noise_floor=a.noise_floor, steps=a.steps),
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
