#!/usr/bin/env python3
"""What the film denoiser costs on the device: prt_denoise_device on device-resident arrays at 1080p and 4K.

  python tools/denoise_rate.py [--sizes 1920x1080,3840x2160 --reps 20 --triangles 100000 --out profiles/denoise_rate.json]

Per size:
 1. ms per a-trous iteration: device events around prt_denoise_device with `iterations` = 0 .. 5; the time of iteration i
    (step 2^i) is the difference between two neighbouring settings, medians of --reps calls after a warm-up call each; the
    iterations = 0 call is what packing, preparing and finishing cost.
 2. The bytes the contract moves per pixel and iteration, 25 taps x 48 B + 32 B (the centre's colour read again and the
    result written), over that time, as a fraction of the measured HBM copy rate (6.29 TB/s) and of the L2 rate (16.8 TB/s)
    of the MI355X: what the stencil would need if no tap were shared between neighbouring pixels.  It is an upper bound on
    the traffic, not a measurement of it: neighbouring pixels share most of their taps in the caches.
 3. The LDS A/B: the same calls with prt_set_param("denoise_lds", 0 | 2 | 1): no iteration, steps 1 and 2, or (the default)
    step 1 alone stage their block's footprint in LDS; the settings alternate in the same process, twice each (the
    difference between a setting's two passes is the spread), and the outputs are compared bit for bit.
 4. ms for the feature pass (prt_render_features, host clock around the synchronous call) on the bunny scene refined to
    --triangles triangles.
One JSON document goes to --out, and every row is printed as it is measured.  Nothing is fixed in advance."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBS, L2_TBS = 6.29, 16.8
BYTES_PER_PIXEL_ITERATION = 25 * 48 + 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_rate.json"))
    a = ap.parse_args()

    import torch

    import denoise_replay as dr
    import parallelraytracing_amd as prt
    if not torch.cuda.is_available():
        raise SystemExit("denoise_rate: no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    r = prt.HipWavefrontRenderer(device=0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(t, reps, **cfg):
        """Median ms of prt_denoise_device over `reps` calls (device events on torch's stream, which the call is ordered in)."""
        r.denoise_arrays(**t, **cfg)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = r.denoise_arrays(**t, **cfg)
            e1.record()
            torch.cuda.synchronize(dev)
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), out

    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        host = dr.synthetic(W, H, seed=7, cap=True)
        t = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
        npix = W * H
        totals = {}
        for lds in (0, 2, 1, 0, 2, 1):   # alternated: the second pass of each is the spread
            r.set_param("denoise_lds", lds)
            ms = [timed(t, a.reps, iterations=k)[0] for k in range(6)]
            totals.setdefault(lds, []).append(ms)
        outs = []
        for lds in (0, 1, 2):
            r.set_param("denoise_lds", lds)
            outs.append(timed(t, 1)[1].view(torch.int32))
        same = bool(torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]))
        r.set_param("denoise_lds", 1)
        for lds in (0, 2, 1):
            best = np.min(np.array(totals[lds]), axis=0)
            spread = float(np.max(np.abs(np.array(totals[lds][0]) - np.array(totals[lds][1]))))
            per_iter = np.diff(best)
            emit(dict(size=size, lds=lds, overhead_ms=float(best[0]), total_ms_5_iterations=float(best[5]),
                      ms_per_iteration=[float(v) for v in per_iter], ms_per_iteration_mean=float(per_iter.mean()),
                      spread_ms=spread, lds_output_equal=same))
        per = float(np.diff(np.min(np.array(totals[1]), axis=0)).mean())   # the default
        tbs = npix * BYTES_PER_PIXEL_ITERATION / (per * 1e-3) / 1e12
        emit(dict(size=size, contract_bytes_per_pixel_iteration=BYTES_PER_PIXEL_ITERATION, contract_tb_per_s=tbs,
                  fraction_of_hbm_rate=tbs / HBM_TBS, fraction_of_l2_rate=tbs / L2_TBS,
                  compulsory_bytes_per_pixel_iteration=64, compulsory_fraction_of_hbm_rate=npix * 64 / (per * 1e-3) / 1e12 / HBM_TBS))

        scene = prt.scenes.mesh_scene(prt.scenes.refined("bunny.ply", a.triangles))
        fr = prt.HipWavefrontRenderer(device=0, max_depth=5, seed=1)
        fr.Init(prt.Film(W, H), scene, prt.Camera(prt.scenes.MESH_CAMERA, width=W, height=H))
        L = prt.capi.lib()
        ms = []
        for k in range(6):
            t0 = time.perf_counter()
            fr._check(L.prt_render_features(fr._ctx))
            if k:
                ms.append((time.perf_counter() - t0) * 1e3)
        emit(dict(size=size, feature_pass_ms=float(np.median(ms)), scene=f"bunny, {scene.n_triangles} triangles"))
        del fr, t

    doc = dict(config=dict(sizes=a.sizes, reps=a.reps, hbm_tb_per_s=HBM_TBS, l2_tb_per_s=L2_TBS, device=torch.cuda.get_device_name(0)), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
