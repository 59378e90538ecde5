#!/usr/bin/env python3
"""What textured shading costs next to the untextured unfused pipeline: C3 (the 870 k-triangle dragon, depth 5) at a reduced
size, with planar UVs put on the dragon by SetUVs.

  python tools/texture_rate.py [--width 960 --height 540 --spp 64 --steps 5 --triangles 870000 --out profiles/texture_rate.json]

Three settings, HIP-event times of the render's own stages (prt_enable_timing), median of --steps steps after one warm-up step:
  unfused     no textures; a 1 x 1 environment image of the sky's colour forces the unfused full-record pipeline (k_raygen_env,
              k_shade_env), the route a texture binding takes: the yardstick
  nearest     a 64 x 64 checker on the ground and a 256 x 256 random image on the dragon, nearest, repeat (k_shade_tex)
  bilinear    the same images, bilinear
The first setting is measured again at the end: the difference between its two rows is the spread.  Recorded per setting:
shade ms and ms per step (raygen + traversal + shade + accumulate).  One JSON document goes to --out, and every row is printed
as it is measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = (("unfused", None), ("nearest", "nearest"), ("bilinear", "bilinear"), ("unfused (again)", None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=870_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_rate.json"))
    a = ap.parse_args()

    import parallelraytracing_amd as prt
    dragon = prt.scenes.refined("dragon.ply", a.triangles)
    dragon.SetUVs(prt.scenes.planar_uvs(dragon, (0, 1)) * np.float32(4.0))
    cam = prt.Camera(prt.scenes.MESH_CAMERA, width=a.width, height=a.height)
    image = np.random.default_rng(1).uniform(0.2, 0.9, size=(256, 256, 3)).astype(np.float32)
    rows = []
    for name, filt in SETTINGS:
        scene = prt.scenes.mesh_scene(dragon)
        r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=1)
        if filt is None:   # the yardstick: the same unfused route, the sky as a one-texel image, nothing textured
            r.set_environment(np.asarray(scene.sky, np.float32).reshape(1, 1, 3), 0.0)
        else:
            scene.SetMaterialTexture(0, scene.AddTexture(prt.scenes.checker(64), filt, "repeat"))
            scene.SetMaterialTexture(2, scene.AddTexture(image, filt, "repeat"))
        r.Init(prt.Film(a.width, a.height), scene, cam)
        r.set_samples_in_flight(a.spp)
        r.enable_timing(True)
        out = []
        for k in range(a.steps + 1):
            r.reset_stats()
            t0 = time.perf_counter()
            r.ProgressiveRender(a.spp)
            wall = (time.perf_counter() - t0) * 1e3
            st = r.stats()
            out.append((st.shade_ms, st.intersect_ms, st.raygen_ms + st.intersect_ms + st.shade_ms + st.accumulate_ms + st.scan_ms, wall,
                        st.rays_total))
        med = [float(np.median([o[i] for o in out[1:]])) for i in range(5)]
        info = r.texture_info()
        row = {"setting": name, "width": a.width, "height": a.height, "spp": a.spp, "triangles": scene.n_triangles,
               "shade_ms": round(med[0], 3), "traversal_ms": round(med[1], 3), "step_ms": round(med[2], 3),
               "step_wall_ms": round(med[3], 3), "rays_per_step": int(med[4]), "texture_device_bytes": int(info.device_bytes)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/texture_rate.py", "args": vars(a), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
