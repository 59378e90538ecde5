#!/usr/bin/env python3
"""What a grid of SH probes costs beside the radiance query over the same rays: the dragon scene of tools/bake_rate.py (870 k
triangles), a 16 x 16 x 16 grid of probes over the scene's box, 256 samples per probe, depth 5.

  python tools/probe_sh_rate.py [--grid 16 --samples 256 --depth 5 --reps 5 --out profiles/probe_sh_rate.json]

Two runs on the same build, alternating, both synchronous calls on a warm context, the host clock around each and the
device time of the probe call beside it, median of --reps:
  * probe_sh(out="torch") over the grid's positions as a device tensor;
  * the yardstick: radiance() over the probes' own rays as device tensors (probe_sh_rays per sample, uploaded beforehand),
    called once per chunk of whole samples with the chunk probe_sh uses (about 2^22 rays), states given, followed by the
    projection written in torch (the nine basis functions, the products, a sum over the samples).
The parent of this feature has no probe path, so the yardstick is what a caller would have written.  Nothing here is a
threshold.  One JSON document goes to --out."""
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
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_sh_rate.json"))
    a = ap.parse_args()

    import torch

    import parallelraytracing_amd as prt
    if not torch.cuda.is_available():
        raise SystemExit("probe_sh_rate: no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    mesh = prt.scenes.refined("dragon.ply", 870_000)
    scene = prt.scenes.mesh_scene(mesh)
    r = prt.HipWavefrontRenderer(device=0, max_depth=a.depth, seed=1)
    r.Init(prt.Film(8, 8), scene, prt.Camera(prt.scenes.MESH_CAMERA, width=8, height=8))
    v = mesh.GetVertices()
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    x = prt.probe_grid(lo, hi, (a.grid,) * 3)
    P, S = len(x), a.samples
    xt = torch.from_numpy(x).to(dev)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    cs = min(S, max(1, (1 << 22) // P))      # probe_sh's own chunk: about 2^22 rays, whole samples
    chunks = []
    for s0 in range(0, S, cs):
        rays = [r.probe_sh_rays(x, sample=s) for s in range(s0, min(S, s0 + cs))]
        chunks.append(tuple(torch.from_numpy(np.concatenate([ray[k] if k != "rng_state" else ray[k].view(np.int32) for ray in rays])).to(dev)
                            for k in ("o", "d", "rng_state")))
    c1, c2a, c2b, c2c = 0.488602512, 1.092548431, 0.315391565, 0.546274215

    def basis(d):
        px, py, pz = d[:, 0], d[:, 1], d[:, 2]
        return torch.stack([torch.full_like(px, 0.282094792), c1 * py, c1 * pz, c1 * px, c2a * (px * py), c2a * (py * pz),
                            c2b * (3.0 * (pz * pz) - 1.0), c2a * (px * pz), c2c * ((px * px) - (py * py))], dim=1)

    def probes():
        ms, out = timed(lambda: r.probe_sh(xt, samples=S, out="torch", return_info=True))
        return ms, out

    def query():
        def run():
            total = torch.zeros((P, 9, 3), dtype=torch.float32, device=dev)
            segs = 0
            for o, d, st in chunks:
                _, info = r.radiance(o, d, rng_state=st, return_info=True)
                total += (info["sum"][:, None, :] * basis(d)[:, :, None]).reshape(-1, P, 9, 3).sum(dim=0)
                segs += int(info["segments"].sum(dtype=torch.int64).item())
            return total * (4.0 * np.pi / S), segs
        return timed(run)

    _, (coeffs, _) = probes()
    _, (ref, _) = query()
    scale = float(ref.abs().max().item())
    diff = float((coeffs - ref).abs().max().item())      # (the torch sum has its own order: close, not bit-equal)
    t_probe, t_query, t_dev = [], [], []
    info = segs = None
    for i in range(a.reps):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            if which == 0:
                ms, (_, got) = probes()
                info = got["info"]
                t_probe.append(ms)
                t_dev.append(info["device_ms"])
            else:
                ms, (_, segs) = query()
                t_query.append(ms)
    mp, mq = float(np.median(t_probe)), float(np.median(t_query))
    doc = dict(mesh="dragon.ply", triangles=int(mesh.n_triangles), grid=f"{a.grid}x{a.grid}x{a.grid}", box=[lo.tolist(), hi.tolist()], probes=P,
               samples=S, depth=a.depth, reps=a.reps, device=torch.cuda.get_device_name(0), rays=int(info["rays"]), samples_per_chunk=cs,
               project_decomposition="one thread per (probe, k), three accumulators",
               probe_ms=mp, probe_device_ms=float(np.median(t_dev)), probe_segments=int(info["segments"]), probe_ms_min_max=[float(min(t_probe)), float(max(t_probe))],
               query_ms=mq, query_segments=segs, query_ms_min_max=[float(min(t_query)), float(max(t_query))],
               probe_over_query=mp / mq, probe_mrays_s=int(info["segments"]) / mp / 1e3, max_abs_difference=diff, max_abs_coefficient=scale,
               note="probe_ms holds the ray kernel, the query's rounds and the projection kernel; query_ms holds the query's rounds "
                    "over rays that are on the device already and the projection as torch operations")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
