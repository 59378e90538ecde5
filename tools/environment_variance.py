#!/usr/bin/env python3
"""What sampling the environment image buys and costs: the ground quad under the 16 x 8 "sun" map (a smooth gradient with
one texel at 1e4) at equal sample counts with lighting OFF (the sun is found by scattered rays only) and with MIS (every
Lambertian vertex sends a shadow ray to the image).

Prints the per-pixel sample-variance ratio OFF / MIS (the variance of a pixel's one-sample values over --samples
independent samples, median and mean over the pixels that see the ground) and the time per sample of both modes at
--width x --height: the MIS step has three launches more per bounce (bounded scan, any-hit walk, k_light_accum).

usage: python3 tools/environment_variance.py [--width 320 --height 240 --samples 64 --depth 5]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallelraytracing_amd import renderer as prt  # noqa: E402


def sun_map():
    i, j = np.mgrid[0:8, 0:16]
    a = np.stack([0.3 + 0.04 * j, 0.4 + 0.03 * i, 0.8 - 0.05 * i + 0.01 * j], -1).astype(np.float32)
    a[2, 11] = 1.0e4
    return a


def ground_scene():
    sc = prt.Scene(preset=None)
    sc.AddQuad(20.0, 20.0, sc.AddLambertian((0.5, 0.6, 0.7)), translation=(0.0, -1.0, 0.0))
    return sc


def one_sample_frames(a, mode):
    film = prt.Film(a.width, a.height)
    r = prt.HipWavefrontRenderer(device=0, max_depth=a.depth, seed=3)
    r.set_environment(sun_map(), 1.0)
    r.Init(film, ground_scene(), prt.Camera((0.0, 3.0, 7.0), width=a.width, height=a.height))
    r.set_lighting(mode)
    lum = np.zeros((a.samples, a.height * a.width))
    for s in range(a.samples):
        film.Clear()
        r.frame_index = s
        r.ProgressiveRender(1)
        r.download()
        lum[s] = film.accum.reshape(-1, 3).mean(1)
    # time per sample: all samples in one call, after a warm-up call
    r.set_samples_in_flight(a.samples)
    r.ProgressiveRender(a.samples)
    r.synchronize()
    t0 = time.perf_counter()
    r.ProgressiveRender(a.samples)
    r.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / a.samples
    return lum, ms


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--width", type=int, default=320)
    p.add_argument("--height", type=int, default=240)
    p.add_argument("--samples", type=int, default=64)
    p.add_argument("--depth", type=int, default=5)
    a = p.parse_args()
    off, ms_off = one_sample_frames(a, "off")
    mis, ms_mis = one_sample_frames(a, "mis")
    ground = mis.var(0, ddof=1) > 0     # pixels that see the ground (a pixel that sees the image directly is constant)
    v_off, v_mis = off.var(0, ddof=1)[ground], mis.var(0, ddof=1)[ground]
    ok = v_mis > 0
    ratio = v_off[ok] / v_mis[ok]
    print(dict(pixels=int(ground.sum()), samples=a.samples, mean_off=round(float(off[:, ground].mean()), 3),
               mean_mis=round(float(mis[:, ground].mean()), 3), var_off=round(float(v_off.mean()), 3),
               var_mis=round(float(v_mis.mean()), 5), ratio_of_mean_variances=round(float(v_off.mean() / v_mis.mean()), 1),
               median_pixel_ratio=round(float(np.median(ratio)), 1), pixels_where_off_never_saw_the_sun=int((v_off < v_mis).sum()),
               ms_per_sample_off=round(ms_off, 4), ms_per_sample_mis=round(ms_mis, 4),
               extra_ms_per_sample=round(ms_mis - ms_off, 4)), flush=True)


if __name__ == "__main__":
    main()
