#!/usr/bin/env python3
"""What the sampled guide features cost the feature pass on the device: prt_render_features with samples = 0 (the one-ray
pass, tools/guide_features_rate.py's figure) and K = 1, 4, 16, with max_specular 0 and 8.

  python tools/feature_samples_rate.py [--size 1920x1080 --reps 10 --triangles 100000 --out profiles/feature_samples_rate.json]

Two scenes at --size, both under a thin lens (aperture 0.1) with jitter on: MIRROR_ROOM (tests/guide_features_replay.py) and
the bunny refined to --triangles triangles beside a mirror placed copy of itself.  The renderer runs on a torch stream; device
events on that stream around the synchronous call, on a warm context; the settings alternate call by call, and the median of
--reps calls of each is reported beside the host clock of the same calls.  Every row carries ms per pass, the extra over the
one-ray pass of the same max_specular, and that extra divided by K times the one-ray pass: about 1 is what K more queries cost;
above 1.5 is a finding.  One JSON document goes to --out, and every row is printed as it is measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = (0, 1, 4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_samples_rate.json"))
    a = ap.parse_args()

    import torch

    import guide_features_replay as gr
    import parallelraytracing_amd as prt
    if not torch.cuda.is_available():
        raise SystemExit("feature_samples_rate: no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in a.size.split("x"))
    L = prt.capi.lib()
    rows = []

    def bunny_scene():
        mesh = prt.scenes.refined("bunny.ply", a.triangles)
        sc = prt.scenes.mesh_scene(mesh)
        sc.AddInstance(mesh, sc.AddMetal((0.9, 0.9, 0.9), 0.0), scale=0.8, euler_deg=(0.0, 40.0, 0.0), translation=(-1.3, -0.3, 0.2))
        return sc

    for name, make, cam, focus in (("MIRROR_ROOM", gr.mirror_room, (5.0, 5.0, 8.0), 9.0), ("bunny and a mirror copy", bunny_scene, (2.0, 1.5, 3.0), 3.5)):
        scene = make()
        r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=1)
        r.Init(prt.Film(W, H), scene, prt.Camera(cam, width=W, height=H))
        r.set_lens(aperture=0.1, focus_distance=focus)
        r.set_sampling(jitter=1)
        stream = torch.cuda.Stream(dev)
        r.set_stream(stream.cuda_stream)
        for ms_max in (0, 8):
            r.set_feature_trace(ms_max)
            ms = {k: [] for k in KS}
            host = {k: [] for k in KS}
            with torch.cuda.stream(stream):
                for k in KS:                                       # warm: allocations, the first launch of every kernel
                    r.set_feature_sampling(k)
                    r._check(L.prt_render_features(r._ctx))
                for i in range(a.reps):
                    for k in (KS if i % 2 == 0 else KS[::-1]):     # each setting follows each of its neighbours equally often
                        r.set_feature_sampling(k)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0 = time.perf_counter()
                        e0.record(stream)
                        r._check(L.prt_render_features(r._ctx))
                        e1.record(stream)
                        stream.synchronize()
                        host[k].append((time.perf_counter() - t0) * 1e3)
                        ms[k].append(e0.elapsed_time(e1))
            one = float(np.median(ms[0]))
            for k in KS[1:]:
                m = float(np.median(ms[k]))
                row = dict(scene=name, size=a.size, triangles=int(scene.n_triangles), reps=a.reps, max_specular=ms_max, samples=k,
                           one_ray_ms=one, ms=m, host_ms=float(np.median(host[k])), ms_min_max=[float(min(ms[k])), float(max(ms[k]))],
                           extra_ms=m - one, extra_over_k_one_ray=(m - one) / (k * one))
                rows.append(row)
                print(json.dumps(row), flush=True)
        r.set_stream(0)
        del r

    doc = dict(config=dict(size=a.size, reps=a.reps, device=torch.cuda.get_device_name(0)), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
