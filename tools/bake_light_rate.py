#!/usr/bin/env python3
"""What the texel's light sample costs a lit bake, and what it buys.

  python tools/bake_light_rate.py [--size 1024 --samples 16 --depth 5 --reps 5 --out profiles/bake_light_rate.json]

Cost: tools/bake_rate.py's setup (the dragon of C3, 870 k triangles, a planar layout at 1024 x 1024, 16 samples per texel,
depth 5) under set_lighting("mis"): bake_irradiance(lighting=True) with and without texel_light=True on the same build,
synchronous calls on a warm context, the host clock around each, alternating, median of --reps.  The expectation from the
code is one sample kernel, one more pass of the occlusion pipeline and one add kernel per chunk.

Variance: the Cornell box with a cube in it (the cube's six sides in a 3 x 2 atlas, 64 x 64 texels, 16 samples per texel,
depth 5, "mis"): the mean squared error of the map with and without texel_light against a 4096-sample bake with it (both
estimators have the same expectation; the reference without it is reported too).  Nothing here is a threshold.  One JSON
document goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cube_atlas_uvs(mesh):
    """cube_uv.ply's six quads (4 vertices each, unit-square UVs) into the cells of a 3 x 2 grid, shrunk to half a cell"""
    uv = mesh.GetUVs().astype(np.float64)
    out = np.empty_like(uv)
    for k in range(6):
        sl = slice(4 * k, 4 * k + 4)
        out[sl, 0] = (k % 3 + 0.25 + 0.5 * uv[sl, 0]) / 3.0
        out[sl, 1] = (k // 3 + 0.25 + 0.5 * uv[sl, 1]) / 2.0
    return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_light_rate.json"))
    a = ap.parse_args()

    import torch

    import parallelraytracing_amd as prt
    if not torch.cuda.is_available():
        raise SystemExit("bake_light_rate: no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    # ---- cost ----
    mesh = prt.scenes.refined("dragon.ply", 870_000)
    uvs = prt.scenes.planar_uvs(mesh, axes=(0, 1))
    r = prt.HipWavefrontRenderer(device=0, max_depth=a.depth, seed=1)
    r.Init(prt.Film(8, 8), prt.scenes.mesh_scene(mesh), prt.Camera(prt.scenes.MESH_CAMERA, width=8, height=8))
    r.set_lighting("mis")
    S, N = a.samples, a.size
    kw = dict(mesh=0, size=(N, N), uvs=uvs, samples=S, lighting=True, return_info=True)

    def bake(texel):
        ms, out = timed(lambda: r.bake_irradiance(texel_light=texel, **kw))
        return ms, out[1]["info"]

    bake(False)
    bake(True)
    t = {False: [], True: []}
    info = {}
    for i in range(a.reps):
        for texel in ((False, True) if i % 2 == 0 else (True, False)):
            ms, info[texel] = bake(texel)
            t[texel].append(ms)
    m_off, m_on = float(np.median(t[False])), float(np.median(t[True]))
    cost = dict(mesh="dragon.ply", triangles=int(mesh.n_triangles), size=f"{N}x{N}", samples=S, depth=a.depth, reps=a.reps, lighting="mis",
                covered=int(info[True]["n_covered"]), rays=int(info[True]["rays"]), segments=int(info[True]["segments"]),
                lit_ms=m_off, lit_ms_min_max=[float(min(t[False])), float(max(t[False]))], lit_device_ms=float(info[False]["device_ms"]),
                lit_shadow_rays=int(info[False]["shadow_rays"]),
                texel_light_ms=m_on, texel_light_ms_min_max=[float(min(t[True])), float(max(t[True]))],
                texel_light_device_ms=float(info[True]["device_ms"]), texel_light_shadow_rays=int(info[True]["shadow_rays"]),
                texel_light_over_lit=m_on / m_off)
    del r

    # ---- variance ----
    cube = prt.Mesh(prt.scenes.asset("cube_uv.ply"))
    mat, inv = prt.make_transform((0.4, 0.4, 0.4), (0.0, 30.0, 0.0), (0.2, 0.6, 0.1))
    cube.transform(mat, inv)
    sc = prt.Scene("CORNELL")
    sc.AddMesh(cube, sc.AddLambertian((0.7, 0.6, 0.5)))
    r = prt.HipWavefrontRenderer(device=0, max_depth=a.depth, seed=1)
    r.Init(prt.Film(8, 8), sc, prt.Camera((2.5, 2.0, 4.0), front=(-2.5, -2.0, -4.0), width=8, height=8))
    r.set_lighting("mis")
    vk = dict(mesh=0, size=(64, 64), uvs=cube_atlas_uvs(cube), lighting=True, return_info=True)
    ref_on, got = r.bake_irradiance(samples=4096, first_sample=1 << 20, texel_light=True, **vk)
    ref_off = r.bake_irradiance(samples=4096, first_sample=1 << 20, texel_light=False, **vk)[0]
    cov = got["coverage"] != 0
    mse = {}
    for texel in (False, True):
        errs = []
        for k in range(8):                      # eight independent 16-sample maps
            irr = r.bake_irradiance(samples=16, first_sample=16 * k, texel_light=texel, **vk)[0]
            errs.append(float(np.mean((irr[cov].astype(np.float64) - ref_on[cov].astype(np.float64)) ** 2)))
        mse[texel] = float(np.mean(errs))
    variance = dict(scene="CORNELL with a cube", size="64x64", samples=16, depth=a.depth, lighting="mis", covered=int(cov.sum()), maps=8,
                    reference_samples=4096, mse_lit=mse[False], mse_texel_light=mse[True], mse_ratio=mse[False] / mse[True],
                    reference_mean=float(ref_on[cov].mean()),
                    references_mse=float(np.mean((ref_on[cov].astype(np.float64) - ref_off[cov].astype(np.float64)) ** 2)))
    doc = dict(device=torch.cuda.get_device_name(0), cost=cost, variance=variance,
               note="cost: synchronous host-form bakes, host clock; both hold the surface passes, the face arrays' upload and the map's "
                    "download.  variance: irradiance units (pi * sum / samples); references_mse is the squared distance between the two "
                    "4096-sample references, the floor under both figures")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
