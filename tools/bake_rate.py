#!/usr/bin/env python3
"""What a bake costs beside the radiance query over the same rays: the dragon of C3 (870 k triangles) at 1024 x 1024, 16 samples
per texel, depth 5.

  python tools/bake_rate.py [--size 1024 --samples 16 --depth 5 --reps 5 --out profiles/bake_rate.json]

The layout is a planar projection of the mesh (prt.scenes.planar_uvs over x and y): a lightmap-sized atlas needs an unwrapper
the project does not have, and the cost of a bake does not depend on which face owns a texel.  The yardstick is radiance()
over the bake's own rays as device tensors (bake_rays per sample, the covered texels, uploaded beforehand), called once per
chunk of whole samples with the chunk the bake uses (about 2^22 rays), states given: the paths the bake follows, through the
public query.  Both are synchronous calls on a warm context; the host clock around each, alternating, median of --reps.  The
expectation is that the bake stays within the query plus its three small passes; nothing here is a threshold.  One JSON
document goes to --out."""
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
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_rate.json"))
    a = ap.parse_args()

    import torch

    import parallelraytracing_amd as prt
    if not torch.cuda.is_available():
        raise SystemExit("bake_rate: no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    mesh = prt.scenes.refined("dragon.ply", 870_000)
    uvs = prt.scenes.planar_uvs(mesh, axes=(0, 1))
    scene = prt.scenes.mesh_scene(mesh)
    r = prt.HipWavefrontRenderer(device=0, max_depth=a.depth, seed=1)
    r.Init(prt.Film(8, 8), scene, prt.Camera(prt.scenes.MESH_CAMERA, width=8, height=8))
    S, N = a.samples, a.size
    kw = dict(mesh=0, size=(N, N), uvs=uvs)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    surf = r.bake_surface(**kw)
    cov = surf["coverage"].ravel() != 0
    n_cov = int(cov.sum())
    cs = min(S, max(1, (1 << 22) // max(1, n_cov)))      # the bake's own chunk: about 2^22 rays, whole samples
    chunks = []
    for s0 in range(0, S, cs):
        o, d, st = [], [], []
        for s in range(s0, min(S, s0 + cs)):
            ray = r.bake_rays(sample=s, **kw)
            o.append(ray["o"].reshape(-1, 3)[cov])
            d.append(ray["d"].reshape(-1, 3)[cov])
            st.append(ray["rng_state"].ravel()[cov].view(np.int32))
        chunks.append(tuple(torch.from_numpy(np.concatenate(x)).to(dev) for x in (o, d, st)))

    def bake():
        ms, out = timed(lambda: r.bake_irradiance(samples=S, return_info=True, **kw))
        return ms, out[1]["info"]

    def query():
        def run():
            return sum(int(r.radiance(o, d, rng_state=st, return_info=True)[1]["segments"].sum(dtype=torch.int64).item()) for o, d, st in chunks)
        return timed(run)

    bake()
    query()
    t_bake, t_query, t_dev = [], [], []
    info = segs = None
    for i in range(a.reps):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            if which == 0:
                ms, info = bake()
                t_bake.append(ms)
                t_dev.append(info["device_ms"])
            else:
                ms, segs = query()
                t_query.append(ms)
    t_surface = [timed(lambda: r.bake_surface(**kw))[0] for _ in range(a.reps)]
    mb, mq = float(np.median(t_bake)), float(np.median(t_query))
    doc = dict(mesh="dragon.ply", triangles=int(mesh.n_triangles), size=f"{N}x{N}", samples=S, depth=a.depth, reps=a.reps,
               device=torch.cuda.get_device_name(0), texels=N * N, covered=n_cov, faces_skipped=int(info["n_faces_skipped"]),
               degenerate=int(info["n_degenerate"]), rays=int(info["rays"]), samples_per_chunk=cs,
               bake_ms=mb, bake_device_ms=float(np.median(t_dev)), bake_segments=int(info["segments"]), bake_ms_min_max=[float(min(t_bake)), float(max(t_bake))],
               query_ms=mq, query_segments=segs, query_ms_min_max=[float(min(t_query)), float(max(t_query))],
               bake_over_query=mb / mq, bake_surface_ms=float(np.median(t_surface)), bake_mrays_s=int(info["segments"]) / mb / 1e3,
               note="bake_ms holds the surface passes, the face arrays' upload and the map's download; query_ms holds neither "
                    "(its rays are on the device already); bake_surface_ms is the surface stage alone with its four downloads")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
