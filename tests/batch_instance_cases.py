"""The cases of tests/test_gpu_batch_instances.py that a CPU test can check without a device (tests/test_batch_instance_cases.py):
the untextured scenes B .. E of tests/texture_replay.py under the lighting modes, at their own size and on the odd film, and the
choice of an adaptive threshold from a reference's frames alone.  No kernel code and no GPU is involved."""
import numpy as np

import adaptive_replay as ar
import texture_replay as tr
from util import prt

ODD = (37, 29)   # no multiple of a tile (8 x 8), a wave (64) or a producer block (256): 1073 pixels, 5 x 4 tiles, four of them partial

# scene_mode_sources[_env], texture_replay.lighting_case's names; both modes in every family of shade instances
LIT_CASES = tr.INSTANCE_LIGHTING_CASES
ODD_LIT_CASES = ("C_mis_analytic", "D_nee_analytic_env", "E_nee_mesh", "D_mis_mesh_env")
# clustered selection: the tables come from the device, so these are replayed in the GPU test only
CLUSTER_CASES = ("E_nee_mesh", "C_nee_mesh", "B_mis_mesh", "D_mis_mesh", "E_nee_mesh_env", "C_nee_mesh_env", "B_nee_mesh_env", "D_mis_mesh_env")
ODD_CLUSTER_CASES = (("D_mis_mesh", False), ("C_nee_mesh_env", False), ("D_mis_mesh_env", True))   # (name, textured)


def resized(c, size):
    """Case c on a film of another size: the same scene and camera position."""
    W, H = size
    return dict(c, W=W, H=H, cam=prt.Camera(c["cam"].position, front=c["cam"].front, width=W, height=H))


def lit_case(name, textured=False, odd=False):
    """texture_replay.lighting_case of the untextured scene (default), on the 37 x 29 film with odd."""
    c, mode, fn = tr.lighting_case(name, textured=textured)
    return (resized(c, ODD) if odd else c), mode, fn


def scene(name, textured=False):
    """Scenes E (no placed copy, 3 primitives), B (placed copies, 2 primitives), C (22 primitives: the primitive BVH) and D (C
    with placed copies), lighting off."""
    return {"B": tr.scene_b, "C": tr.scene_c, "D": tr.scene_d, "E": tr.scene_e}[name](textured=textured)


def facts(name):
    """(INST, ABVH with prim_bvh = 1) of a scene or case name"""
    return name[0] in "BD", name[0] in "CD"


def split_threshold(frames, W, H, min_spp, noise_floor=0.01):
    """A threshold of the adaptive loop that stops a proper, non-empty subset of the 8 x 8 tiles after min_spp samples, chosen
    from a reference's one-sample frames alone: a tile goes on while one of its pixels has noise > threshold, so the threshold
    is put in the middle of the widest relative gap between the sorted per-tile maxima of the noise (adaptive_replay.noise_map):
    the widest of the middle half of the tiles if that is above 1e-4, else the widest of all.  (With four samples the noise of a
    pixel is at most 1, which a pixel with one bright sample reaches, so on a scene without flat tiles the maxima crowd below 1.)
    The gap must exceed 1e-5: noise_map and the threshold are rounded to float32 (6e-8), the rule itself is float64 on both
    sides.  -> (threshold, tiles that stop, tiles that go on)."""
    A, Q = ar.moments(frames[:min_spp])
    noise = ar.noise_map(np.full((H, W), min_spp, np.float32), A, Q, noise_floor).astype(np.float64)
    v = np.sort(np.array([noise[y0:y1, x0:x1].max() for x0, y0, x1, y1 in ar.tiles(W, H)]))
    n = len(v)
    gap = np.array([0.0] + [(v[k] - v[k - 1]) / max(v[k], 1e-30) for k in range(1, n)])
    lo, hi = max(1, n // 4), max(2, n - n // 4)
    k = lo + int(np.argmax(gap[lo:hi]))
    if gap[k] <= 1e-4:
        k = int(np.argmax(gap))
    assert gap[k] > 1e-5, v
    thr = float(np.float32(0.5 * (v[k - 1] + v[k])))
    assert v[k - 1] * (1 + 1e-6) < thr < v[k] * (1 - 1e-6)
    return thr, k, n - k
