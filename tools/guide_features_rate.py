#!/usr/bin/env python3
"""What following specular chains costs the feature pass on the device: prt_render_features with max_specular 0 and 8.

  python tools/guide_features_rate.py [--size 1920x1080 --reps 20 --triangles 100000 --out profiles/guide_features_rate.json]

Two scenes at --size: MIRROR_ROOM (tests/guide_features_replay.py: analytic primitives only, a third of the pixels continue
past a mirror or glass) and the bunny refined to --triangles triangles beside a mirror placed copy of itself (a two-level
tree).  The renderer runs on a torch stream; device events on that stream around the synchronous call, on a warm context;
the two settings alternate call by call, and the median of --reps calls of each is reported beside the host clock of the same
calls, the number of chains, the rounds the host loop ran and the live count of each round.  There is no threshold: what is to
be seen is that the mode costs about one closest-hit query over the live fraction per round plus one small wait.
One JSON document goes to --out, and every row is printed as it is measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_features_rate.json"))
    a = ap.parse_args()

    import torch

    import guide_features_replay as gr
    import parallelraytracing_amd as prt
    if not torch.cuda.is_available():
        raise SystemExit("guide_features_rate: no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in a.size.split("x"))
    L = prt.capi.lib()
    rows = []

    def bunny_scene():
        mesh = prt.scenes.refined("bunny.ply", a.triangles)
        sc = prt.scenes.mesh_scene(mesh)
        sc.AddInstance(mesh, sc.AddMetal((0.9, 0.9, 0.9), 0.0), scale=0.8, euler_deg=(0.0, 40.0, 0.0), translation=(-1.3, -0.3, 0.2))
        return sc

    for name, make, cam in (("MIRROR_ROOM", gr.mirror_room, (5.0, 5.0, 8.0)), ("bunny and a mirror copy", bunny_scene, (2.0, 1.5, 3.0))):
        scene = make()
        r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=1)
        r.Init(prt.Film(W, H), scene, prt.Camera(cam, width=W, height=H))
        stream = torch.cuda.Stream(dev)
        r.set_stream(stream.cuda_stream)
        ms = {0: [], 8: []}
        host = {0: [], 8: []}
        with torch.cuda.stream(stream):
            for k in (0, 8):                                   # warm: allocations, the first launch of every kernel
                r.set_feature_trace(k)
                r._check(L.prt_render_features(r._ctx))
            for i in range(2 * a.reps):
                k = (0, 8)[(i + i // 2) % 2]                   # 0 8 8 0 0 8 8 0 ...: each follows the other as often as itself
                r.set_feature_trace(k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                r._check(L.prt_render_features(r._ctx))
                e1.record(stream)
                stream.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e3)
                ms[k].append(e0.elapsed_time(e1))
        r.set_feature_trace(8)
        b = r.render_features()["guide"]["bounces"]
        live = [int((b > k).sum()) for k in range(int(b.max()))]       # the chains that have followed k + 1 vertices: round k's query
        row = dict(scene=name, size=a.size, triangles=int(scene.n_triangles), reps=a.reps,
                   first_hit_ms=float(np.median(ms[0])), followed_ms=float(np.median(ms[8])),
                   first_hit_host_ms=float(np.median(host[0])), followed_host_ms=float(np.median(host[8])),
                   first_hit_ms_min_max=[float(min(ms[0])), float(max(ms[0]))], followed_ms_min_max=[float(min(ms[8])), float(max(ms[8]))],
                   chain_pixels=live[0], rounds=len(live), live_per_round=live, live_fraction=live[0] / float(W * H))
        row["extra_ms"] = row["followed_ms"] - row["first_hit_ms"]
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
