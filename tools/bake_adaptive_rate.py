#!/usr/bin/env python3
"""What the bake's statistics cost, and what block-adaptive sampling buys.

  python tools/bake_adaptive_rate.py [--size 1024 --samples 16 --depth 5 --reps 5 --out profiles/bake_adaptive_rate.json]
                                     [--uniform-only --package-root DIR] [--parent-json FILE]

Setup: tools/bake_rate.py's (the dragon of C3, 870 k triangles, a planar layout) under set_lighting("mis") with
texel_light=True, depth 5.

(a) Overhead of the statistics path: bake_irradiance_adaptive with min_spp = max_spp = --samples at --size^2 against
    bake_irradiance(samples=--samples) on the same build: synchronous calls on a warm context, the host clock around each,
    alternating, median of --reps; beside it the median of the calls' own device times (PrtBakeInfo.device_ms, events around
    the device work), which leave out most of the host's share that other work on the host disturbs.  The expectation from
    the code: two more fp32 sums per sample value, three more maps to clear, four more to download, one division per texel.  --uniform-only measures the uniform bake alone through the entry points the
    parent commit has too (with --package-root DIR: the package of another checkout), and --parent-json FILE copies such a
    document into this one, so that the record shows whether the existing path moved.

(b) What adapting buys, at 256^2 so that a 4096-sample reference is affordable: adaptive min 16 / step 16 / max 256 at two
    thresholds against the uniform bake of the same total sample count (rounded up to whole samples per texel): the mean
    squared error of pi * mean against a 4096-sample bake over a disjoint index range, the wall time, and the histogram of
    counts.  Nothing here is a threshold to pass.  One JSON document goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", type=int, default=256)
    ap.add_argument("--reference-samples", type=int, default=4096)
    ap.add_argument("--thresholds", type=float, nargs=2, default=(0.1, 0.05))
    ap.add_argument("--uniform-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_adaptive_rate.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))

    import torch

    import parallelraytracing_amd as prt
    if not torch.cuda.is_available():
        raise SystemExit("bake_adaptive_rate: no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    mesh = prt.scenes.refined("dragon.ply", 870_000)
    uvs = prt.scenes.planar_uvs(mesh, axes=(0, 1))
    r = prt.HipWavefrontRenderer(device=0, max_depth=a.depth, seed=1)
    r.Init(prt.Film(8, 8), prt.scenes.mesh_scene(mesh), prt.Camera(prt.scenes.MESH_CAMERA, width=8, height=8))
    r.set_lighting("mis")
    S, N = a.samples, a.size
    kw = dict(mesh=0, uvs=uvs, lighting=True, texel_light=True)

    def uniform(size, samples, first=0):
        return timed(lambda: r.bake_irradiance(size=(size, size), samples=samples, first_sample=first, return_info=True, **kw))

    def adaptive(size, lo, step, hi, thr, first=0):
        return timed(lambda: r.bake_irradiance_adaptive(size=(size, size), threshold=thr, min_spp=lo, step_spp=step, max_spp=hi, first_sample=first, **kw))

    # ---- (a) ----
    uniform(N, S)
    t_uni, t_stat, d_uni, d_stat = [], [], [], []
    info_u = info_s = None
    if not a.uniform_only:
        adaptive(N, S, 0, S, 0.1)
    for i in range(a.reps):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            if which == 0:
                ms, out = uniform(N, S)
                t_uni.append(ms)
                info_u = out[1]["info"]
                d_uni.append(float(info_u["device_ms"]))
            elif not a.uniform_only:
                ms, out = adaptive(N, S, 0, S, 0.1)
                t_stat.append(ms)
                info_s = out["info"]
                d_stat.append(float(info_s["device_ms"]))
    overhead = dict(mesh="dragon.ply", triangles=int(mesh.n_triangles), size=f"{N}x{N}", samples=S, depth=a.depth, reps=a.reps, lighting="mis",
                    texel_light=True, covered=int(info_u["n_covered"]), rays=int(info_u["rays"]), segments=int(info_u["segments"]),
                    uniform_ms=float(np.median(t_uni)), uniform_ms_min_max=[float(min(t_uni)), float(max(t_uni))],
                    uniform_device_ms=float(np.median(d_uni)), uniform_device_ms_min_max=[min(d_uni), max(d_uni)])
    if a.uniform_only:
        doc = dict(device=torch.cuda.get_device_name(0), overhead=overhead, note="the uniform bake alone, through the entry points of the parent commit")
        print(json.dumps(doc), flush=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    overhead.update(statistics_ms=float(np.median(t_stat)), statistics_ms_min_max=[float(min(t_stat)), float(max(t_stat))],
                    statistics_device_ms=float(np.median(d_stat)), statistics_device_ms_min_max=[min(d_stat), max(d_stat)],
                    statistics_over_uniform=float(np.median(t_stat) / np.median(t_uni)),
                    statistics_over_uniform_device=float(np.median(d_stat) / np.median(d_uni)),
                    same_segments=bool(info_s["segments"] == info_u["segments"]))
    if a.parent_json:
        with open(a.parent_json) as f:
            p = json.load(f)["overhead"]
        overhead.update(parent_uniform_ms=p["uniform_ms"], parent_uniform_ms_min_max=p["uniform_ms_min_max"],
                        parent_uniform_device_ms=p["uniform_device_ms"], parent_uniform_device_ms_min_max=p["uniform_device_ms_min_max"],
                        uniform_over_parent=overhead["uniform_ms"] / p["uniform_ms"],
                        uniform_over_parent_device=overhead["uniform_device_ms"] / p["uniform_device_ms"])

    # ---- (b) ----
    M, R = a.small, a.reference_samples
    ref = r.bake_irradiance(size=(M, M), samples=R, first_sample=1 << 20, return_info=True, **kw)
    cov = ref[1]["coverage"] != 0
    ref_irr = ref[0][cov].astype(np.float64)
    n_cov = int(cov.sum())
    runs = []
    for thr in a.thresholds:
        adaptive(M, 16, 16, 256, thr)                    # warm: the workspace of this shape
        ms_a, got = adaptive(M, 16, 16, 256, thr)
        cnt = got["count"][cov]
        total = int(got["adaptive"]["texel_samples"])
        spp_u = -(-total // n_cov)
        uniform(M, spp_u)
        ms_u, uni = uniform(M, spp_u)
        mse_a = float(np.mean((got["irradiance"][cov].astype(np.float64) - ref_irr) ** 2))
        mse_u = float(np.mean((uni[0][cov].astype(np.float64) - ref_irr) ** 2))
        vals, freq = np.unique(cnt, return_counts=True)
        runs.append(dict(threshold=thr, noise_floor=0.01, adaptive=got["adaptive"], adaptive_ms=ms_a, adaptive_device_ms=float(got["info"]["device_ms"]),
                         adaptive_mse=mse_a, mean_spp=total / n_cov, count_histogram={str(int(v)): int(f) for v, f in zip(vals, freq)},
                         uniform_spp=int(spp_u), uniform_ms=ms_u, uniform_device_ms=float(uni[1]["info"]["device_ms"]), uniform_mse=mse_u,
                         mse_uniform_over_adaptive=mse_u / mse_a, ms_adaptive_over_uniform=ms_a / ms_u))
    gain = dict(size=f"{M}x{M}", covered=n_cov, min_spp=16, step_spp=16, max_spp=256, reference_samples=R,
                reference_mean=float(ref_irr.mean()), runs=runs)
    doc = dict(device=torch.cuda.get_device_name(0), overhead=overhead, gain=gain,
               note="synchronous host-form bakes, host clock; every call holds the surface passes, the face arrays' upload and the maps' "
                    "download (the statistics path downloads six maps, the uniform bake two).  mse: irradiance units (pi * mean), over "
                    "covered texels, against a reference over a disjoint sample-index range; single calls, not medians, in (b).  device_ms: "
                    "events around a call's device work, host waits inside it included")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
