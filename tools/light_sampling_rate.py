#!/usr/bin/env python3
"""Cost of light sampling (PrtLighting) on C3: ms per 256-spp step at 1080p with lighting off, nee and mis, and shadow
rays per second.  usage: python3 tools/light_sampling_rate.py [--steps N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallelraytracing_amd import renderer as prt, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    sc, cam, W, H, spp, D = scenes.config("C3")
    for mode in ("off", "nee", "mis"):
        film = prt.Film(W, H)
        r = prt.HipWavefrontRenderer(device=0, max_depth=D, seed=0)
        r.Init(film, sc, cam)
        r.set_samples_in_flight(spp)
        r.set_lighting(mode)
        r.ProgressiveRender(spp)  # warm-up
        r.reset_stats()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r.ProgressiveRender(spp)
        dt = (time.perf_counter() - t0) / a.steps
        ls = r.light_stats()
        print(f"{mode:4s} {1e3 * dt:8.1f} ms/step  closest-hit {r.stats().rays_total / a.steps / dt / 1e9:5.2f} G rays/s  "
              f"shadow {ls.shadow_rays / a.steps / dt / 1e9:5.2f} G rays/s  occluded {ls.shadow_occluded / max(ls.shadow_rays, 1):.3f}")
        del r


if __name__ == "__main__":
    main()
