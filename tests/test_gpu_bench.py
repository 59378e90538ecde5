"""bench.py on the GPU box (-m gpu): a plain run prints the headline line alone, and --dump-outputs writes what the last
timed step handed its caller, the same film whether or not --full adds its own measurements around the steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu


def _bench(out_dir, *extra):
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "C2", "--spp-per-step", "2",
            "--dump-outputs", str(out_dir)] + list(extra)
    p = subprocess.run([sys.executable, os.path.join(util.ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{"metric"')][-1])
    return line, np.load(out_dir / "rgb.npy"), np.load(out_dir / "weight.npy")


def test_plain_run_and_dumped_outputs_match_a_full_run(tmp_path):
    plain, rgb, w = _bench(tmp_path / "plain")
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and plain["secondary"] is None
    assert rgb.dtype == np.float32 and rgb.shape == (720, 1280, 3) and rgb.any()
    assert w.dtype == np.float32 and w.shape == (720, 1280)
    assert (w == 3 * 2).all()  # the film accumulates every step: (warmup + steps) x spp per step
    full, rgb_f, w_f = _bench(tmp_path / "full", "--full", "--no-cpu-baseline", "--no-secondary")
    assert full["roofline"] is not None and full["config"]["rays_timed"] == plain["config"]["rays_timed"]
    assert np.array_equal(rgb_f, rgb) and np.array_equal(w_f, w)
