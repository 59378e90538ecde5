#!/usr/bin/env python3
"""What a refit costs end to end: prt_refit_meshes (host arrays) against prt_refit_meshes_device (arrays on the device,
with and without supplied normals), on the refined dragon (870 k triangles) and the bunny (10 k).

  python tools/refit_rate.py [--scenes dragon,bunny --runs 10 --lib path/to/libprt.so --out profiles/refit_rate.json]

Per scene and form: one warm-up call, then --runs calls that alternate between two deformations of the mesh.  A call is
synchronous on return, so its time is the host clock around it (PrtRefitInfo.wall_ms says the same from inside); the C
entry points are called directly with descriptors built beforehand, so that no Python flattening is in the window.
Reported: median / min / max of the wall time, PrtRefitInfo of the last call (device_ms, bytes over the bus).
--lib: another build of libprt.so (the parent commit's, for the baseline): a library without the device form is measured
for the host form alone.  Compare two builds by running them alternately in one job.  Needs a GPU: there is no fallback.
One JSON document goes to --out, and every row is printed as it is measured."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ("prt_refit_meshes_device", "prt_mesh_normals_device", "prt_refit_info")


def deformed(prt, mesh, amp, seed):
    v = mesh.GetVertices().astype(np.float64)
    rng = np.random.default_rng(seed)
    v[:, 0] += amp * 4.0 * np.sin(3.0 * v[:, 1])
    v[:, 2] += amp * 4.0 * np.cos(2.0 * v[:, 0])
    v += rng.normal(size=v.shape) * amp
    return prt.Mesh(vertices=v.astype(np.float32), normals=mesh.GetNormals(), indices=mesh.GetIndices())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dragon,bunny")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_rate.json"))
    a = ap.parse_args()
    import torch

    from parallelraytracing_amd import capi
    has_device_form = True
    if a.lib:
        try:
            capi._lib = capi.load(a.lib)
        except AttributeError:
            for n in NEW:
                capi.SIGNATURES.pop(n, None)
            capi._lib = capi.load(a.lib)
            has_device_form = False
    import parallelraytracing_amd as prt
    L = capi.lib()
    label = a.label or (os.path.basename(os.path.dirname(a.lib)) if a.lib else "this build")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def measure(call, info):
        call(0)  # warm-up: code objects, the scene's tables, the allocator
        t = []
        for k in range(a.runs):
            t0 = time.perf_counter()
            call(k & 1)
            t.append((time.perf_counter() - t0) * 1e3)
        return {"wall_ms_median": round(float(np.median(t)), 3), "wall_ms_min": round(min(t), 3), "wall_ms_max": round(max(t), 3), **info()}

    for name in a.scenes.split(","):
        base = prt.scenes.refined("dragon.ply", 870_000) if name == "dragon" else prt.Mesh(prt.scenes.asset("bunny.ply"))
        moved = [deformed(prt, base, 0.002, 5), deformed(prt, base, 0.002, 6)]
        scenes = [prt.scenes.mesh_scene(m) for m in moved]
        descs = [s.desc() for s in scenes]
        r = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=1)
        r.Init(prt.Film(64, 36), prt.scenes.mesh_scene(base), prt.Camera(prt.scenes.MESH_CAMERA, width=64, height=36))

        def info():
            b = r.bvh_info()
            out = {"refit_ms": round(b.refit_ms, 3)}
            if has_device_form:
                i = r.refit_info()
                out.update(device_ms=round(i["device_ms"], 3), info_wall_ms=round(i["wall_ms"], 3), h2d_bytes=i["h2d_bytes"], d2h_bytes=i["d2h_bytes"])
            return out

        def host(k):
            r._check(L.prt_refit_meshes(r._ctx, descs[k].meshes, descs[k].n_meshes))

        common = {"build": label, "scene": name, "triangles": base.n_triangles, "vertices": base.n_vertices, "runs": a.runs}
        emit({**common, "form": "host arrays", **measure(host, info)})
        if not has_device_form:
            continue
        pos = [torch.from_numpy(m.GetVertices()).to("cuda:0") for m in moved]
        nrm = torch.from_numpy(base.GetNormals()).to("cuda:0")
        torch.cuda.synchronize()
        for what, normals in (("device arrays, normals supplied", nrm), ("device arrays, normals computed", None)):
            arrs = []
            for p in pos:
                arr = (capi.PrtMeshDeviceArrays * 1)()
                arr[0].positions, arr[0].normals = p.data_ptr(), None if normals is None else normals.data_ptr()
                arrs.append(arr)

            def device(k):
                r._check(L.prt_refit_meshes_device(r._ctx, arrs[k], 1))

            emit({**common, "form": what, **measure(device, info)})
        t0 = time.perf_counter()
        r.bvh_read8()   # the host copies on demand: what the device form left out of every call
        emit({**common, "form": "refresh of the host copies (once, on demand)", "wall_ms": round((time.perf_counter() - t0) * 1e3, 3)})
        del r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/refit_rate.py", "args": vars(a), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
