#!/usr/bin/env python3
"""What the thin-lens route costs next to the jittered route: C3 (the 870 k-triangle dragon, depth 5) at a reduced size with
jitter, with a lens, and with both.

  python tools/lens_rate.py [--width 960 --height 540 --spp 64 --steps 5 --triangles 870000 --out profiles/lens_rate.json]

Per setting, HIP-event times of the render's own stages (prt_enable_timing), median of --steps steps after one warm-up step:
raygen ms, first-traversal ms (the traversal time of a step cut off after one segment: the same primary rays), ms per step.
The jittered setting is measured twice, first and last: the difference between its two rows is the spread.
All three settings generate one full ray record per sample; what differs is the two extra draws, the sincos / sqrt, the stored
origin, two rays instead of four per slot reservation in ray generation, and primary rays that no longer share an origin in the
first traversal.  One JSON document goes to --out, and every row is printed as it is measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (the first setting runs again at the end: the difference between its two rows is the spread of the measurement)
SETTINGS = (("jitter", 1, (0.0, 0.0, 0.0)), ("lens", 0, (0.0, 0.02, 2.3)), ("jitter+lens", 1, (0.0, 0.02, 2.3)),
            ("jitter (again)", 1, (0.0, 0.0, 0.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=870_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_rate.json"))
    a = ap.parse_args()

    import parallelraytracing_amd as prt
    scene = prt.scenes.mesh_scene(prt.scenes.refined("dragon.ply", a.triangles))
    cam = prt.Camera(prt.scenes.MESH_CAMERA, width=a.width, height=a.height)
    rows = []

    def stage_ms(r, depth):
        r.max_depth = depth
        out = []
        for k in range(a.steps + 1):
            r.reset_stats()
            t0 = time.perf_counter()
            r.ProgressiveRender(a.spp)
            wall = (time.perf_counter() - t0) * 1e3
            st = r.stats()
            out.append((st.raygen_ms, st.intersect_ms, st.raygen_ms + st.intersect_ms + st.shade_ms + st.accumulate_ms + st.scan_ms, wall,
                        st.rays_total))
        return [float(np.median([o[i] for o in out[1:]])) for i in range(5)]

    for name, jitter, lens in SETTINGS:
        r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=1)
        r.Init(prt.Film(a.width, a.height), scene, cam)
        r.set_samples_in_flight(a.spp)
        r.set_sampling(jitter=jitter)
        r.set_lens(*lens)
        r.enable_timing(True)
        first = stage_ms(r, 1)
        full = stage_ms(r, 5)
        row = {"setting": name, "width": a.width, "height": a.height, "spp": a.spp, "triangles": scene.n_triangles,
               "raygen_ms": round(full[0], 3), "first_traversal_ms": round(first[1], 3), "traversal_ms": round(full[1], 3),
               "step_ms": round(full[2], 3), "step_wall_ms": round(full[3], 3), "rays_per_step": int(full[4])}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/lens_rate.py", "args": vars(a), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
