#!/usr/bin/env python3
"""What the temporal reprojection costs on the device: prt_temporal_reproject_device on device-resident arrays at 1080p and 4K.

  python tools/temporal_rate.py [--sizes 1920x1080,3840x2160 --reps 20 --out profiles/temporal_rate.json]

Per size, device events around the _device entry (pack of the frame and of the history into records, k_tp_reproject, unpack of
N' / m1' / m2'), medians of --reps calls after a warm-up call each, on the two-plane fixture of tests/temporal_replay.py (a
coherent camera motion, disocclusions, off-screen and behind-the-camera pixels).  Two settings alternate in the same process,
twice each (the difference between a setting's two passes is the spread): with a history, and without one (hc = NULL: the
kernel reads the frame and writes its inputs back, no gather).  The difference of the two is what the four tap gathers and
the packing of the history cost.
Bytes per pixel that must move (every array read or written once; the four tap gathers counted as ONE read of the history's
56-byte records, what they cost when neighbouring pixels share their lines):
  pack of the frame      13 planar floats in = 52 B, records out = 56 B                       108 B
  pack of the history    the same                                                             108 B
  k_tp_reproject         frame records 56 B in, history 56 B in (not without one), {c', N'} 16 B + {m1', m2'} 8 B + mean 12 B
                         + var 4 B + status 1 B = 41 B out (the array form writes no nrm / pos)   153 B (97 B without a history)
  unpack                 {c', N'} 16 B + {m1', m2'} 8 B in, 3 planar floats out = 12 B           36 B
With a history the entry moves 405 B per pixel; that over the measured time is reported as a fraction of the measured HBM copy
rate of the MI355X (6.29 TB/s), for the setting with a history only.  It is a lower bound on the traffic, not a measurement of
it: how often a history line is fetched again by the gathers is not measured here.  One JSON document goes to --out, and every
row is printed as it is measured.  Nothing is fixed in advance, nothing is gated."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBS = 6.29
PACK_BYTES, UNPACK_BYTES = 52 + 56, 24 + 12
KERNEL_BYTES = {"history": 56 + 56 + 41, "none": 56 + 41}
ENTRY_BYTES_WITH_HISTORY = 2 * PACK_BYTES + KERNEL_BYTES["history"] + UNPACK_BYTES


def row(size, npix, setting, ms, spread_ms, status):
    """One row of the document from a measured time: the derived fields are functions of `ms` alone."""
    r = dict(size=size, setting=setting, ms=ms, spread_ms=spread_ms, pixels_with_status_1=status, kernel_bytes_per_pixel=KERNEL_BYTES[setting])
    if setting == "history":
        r.update(entry_bytes_per_pixel=ENTRY_BYTES_WITH_HISTORY,
                 entry_bytes_fraction_of_hbm_rate=npix * ENTRY_BYTES_WITH_HISTORY / (ms * 1e-3) / 1e12 / HBM_TBS)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_rate.json"))
    a = ap.parse_args()

    import torch

    import parallelraytracing_amd as prt
    import temporal_replay as tr
    if not torch.cuda.is_available():
        raise SystemExit("temporal_rate: no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    r = prt.HipWavefrontRenderer(device=0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(K, cur, hist, reps):
        """Median ms of prt_temporal_reproject_device over `reps` calls (device events on torch's stream, which the call is ordered in)."""
        r.temporal_arrays(K, **cur, history=hist)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = r.temporal_arrays(K, **cur, history=hist)
            e1.record()
            torch.cuda.synchronize(dev)
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), out

    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        K, cur, hist = tr.two_planes(W, H)
        tc = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cur.items()}
        th = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in hist.items()}
        npix = W * H
        ms = {"history": [], "none": []}
        status = None
        for setting in ("history", "none", "history", "none"):   # alternated: the second pass of each is the spread
            t, out = timed(K, tc, th if setting == "history" else None, a.reps)
            ms[setting].append(t)
            if setting == "history":
                status = float(out["status"].float().mean().item())
        for setting in ("history", "none"):
            best = min(ms[setting])
            emit(row(size, npix, setting, best, abs(ms[setting][0] - ms[setting][1]), status))   # best of the two passes' medians
        del tc, th

    doc = dict(config=dict(sizes=a.sizes, reps=a.reps, hbm_tb_per_s=HBM_TBS, device=torch.cuda.get_device_name(0)), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
