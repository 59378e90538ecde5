#!/usr/bin/env python3
"""Rate of the ray queries on device-resident rays: closest_hit_device against occluded (device form), C3 scene
(dragon refined to 870 k triangles), one ray per pixel at 1920x1080.

  python tools/ray_query_rate.py [--width 1920 --height 1080 --repeats 7 --warmup 2]

Ray sets: shadow rays from the primary hit points toward a point light (tmax = distance to the light * (1 - 1e-4)), the
same rays with tmax = +inf, and diffuse bounce rays (tmax = +inf).  Every set is timed with torch events around the calls
on the context's stream, closest hit and occlusion alternating, after warm-up; the median is reported.  Kernel names for
`rocprofv3 --kernel-trace --stats`: k_traverse8_persistent (closest hit), k_occluded8_persistent (any hit), with
k_pack_rays / k_pack_occlusion_rays, k_scan_prims / k_scan_prims_bounded and k_hit_records / k_occlusion_bytes around them.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIGHT = (2.0, 6.0, 3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    import parallelraytracing_amd as prt
    W, H = a.width, a.height
    scene, cam, _, _, _, _ = prt.scenes.config("C3")
    cam = prt.Camera(cam.position, width=W, height=H)
    r = prt.HipWavefrontRenderer(device=0)
    r.Init(prt.Film(W, H), scene, cam)
    s = torch.cuda.Stream(device=0)
    r.set_stream(s.cuda_stream)
    dev = torch.device("cuda", 0)
    with torch.cuda.stream(s):
        ys, xs = np.mgrid[0:H, 0:W]
        o, d = r.camera_rays((xs.ravel() + 0.5).astype(np.float32), (ys.ravel() + 0.5).astype(np.float32))
        po, pd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        h = r.closest_hit_device(po, pd)
        hit = h[:, 0] >= 0
        pos = h.view(torch.float32)[:, 4:7][hit].contiguous()
        nrm = h.view(torch.float32)[:, 7:10][hit].contiguous()
        v = torch.tensor(LIGHT, dtype=torch.float32, device=dev) - pos
        dist = torch.linalg.norm(v, dim=1)
        sdir = (v / dist[:, None]).contiguous()
        tmax = (dist * (1.0 - 1e-4)).contiguous()
        g = torch.Generator(device=dev).manual_seed(1)
        u = torch.randn(pos.shape, generator=g, device=dev)
        bdir = nrm + u / torch.linalg.norm(u, dim=1, keepdim=True)
        bdir = (bdir / torch.linalg.norm(bdir, dim=1, keepdim=True)).contiguous()
        inf = torch.full_like(tmax, float("inf"))
        sets = {"shadow": (pos, sdir, tmax), "shadow_inf": (pos, sdir, inf), "bounce_inf": (pos, bdir, inf)}
        print(f"# C3 {W}x{H}: {po.shape[0]} primary rays, {pos.shape[0]} hit the scene", flush=True)
        for name, (so, sd, st) in sets.items():
            n = so.shape[0]

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                out = fn()
                e1.record(s)
                e1.synchronize()
                return e0.elapsed_time(e1), out

            ch = lambda: r.closest_hit_device(so, sd)  # noqa: E731
            oc = lambda: r.occluded(so, sd, st)  # noqa: E731
            for _ in range(a.warmup):
                timed(ch)
                timed(oc)
            t_ch, t_oc = [], []
            for _ in range(a.repeats):
                t, hits = timed(ch)
                t_ch.append(t)
                t, occ = timed(oc)
                t_oc.append(t)
            r.synchronize()
            ms_ch, ms_oc = float(np.median(t_ch)), float(np.median(t_oc))
            t2 = (st * st)
            hf = hits.view(torch.float32)
            via_ch = (hits[:, 0] >= 0) & (hf[:, 3] < t2) & (st > 0)
            print(json.dumps({"set": name, "rays": n, "closest_hit_ms": round(ms_ch, 4), "occluded_ms": round(ms_oc, 4),
                              "closest_hit_grays_per_s": round(n / ms_ch / 1e6, 3), "occluded_grays_per_s": round(n / ms_oc / 1e6, 3),
                              "speedup": round(ms_ch / ms_oc, 3), "occluded_fraction": round(float(occ.float().mean().item()), 4),
                              "agrees_with_closest_hit": bool(torch.equal(occ, via_ch))}), flush=True)
    r.set_stream(0)


if __name__ == "__main__":
    main()
