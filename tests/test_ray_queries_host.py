"""CPU-side tests of the ray-query entry points (prt_occluded, prt_occluded_device, prt_closest_hit_device): no CPU
fallback, argument checks of the C-ABI and of the Python layer, and the occupancy of the any-hit kernel's instances."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from util import prt

capi = prt.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _host_only():
    r = prt.HipWavefrontRenderer(device=-1)  # host-only context: utilities only
    r.set_scene_host_only(prt.Scene("CORNELL"))
    return r


def test_ray_queries_fail_loudly_without_a_device():
    r = _host_only()
    o = np.zeros((4, 3), np.float32)
    d = np.ones((4, 3), np.float32)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.occluded(o, d, np.ones(4, np.float32))
    L = capi.lib()
    buf = (C.c_uint8 * 64)()
    assert L.prt_occluded_device(r._ctx, 4, C.c_void_p(1), C.c_void_p(1), C.c_void_p(1), buf) == 2  # PRT_ERR_NO_DEVICE
    assert "no HIP device" in L.prt_last_error(r._ctx).decode()
    assert L.prt_closest_hit_device(r._ctx, 4, C.c_void_p(1), C.c_void_p(1), buf) == 2
    assert "no HIP device" in L.prt_last_error(r._ctx).decode()


def test_ray_query_argument_checks_of_the_c_abi():
    L = capi.lib()
    fp = C.POINTER(C.c_float)
    assert L.prt_occluded(None, 1, fp(), fp(), fp(), C.POINTER(C.c_uint8)()) == 1  # PRT_ERR_INVALID: no context
    assert L.prt_occluded_device(None, 1, None, None, None, None) == 1
    assert L.prt_closest_hit_device(None, 1, None, None, None) == 1
    # a context without a device reports that before anything else, whatever the other arguments (no scene, n == 0, nulls)
    r = prt.HipWavefrontRenderer(device=-1)
    assert L.prt_occluded(r._ctx, 0, fp(), fp(), fp(), C.POINTER(C.c_uint8)()) == 2
    assert L.prt_occluded_device(r._ctx, 0, None, None, None, None) == 2
    assert L.prt_closest_hit_device(r._ctx, 0, None, None, None) == 2


def test_occluded_python_argument_validation():
    r = _host_only()
    o = np.zeros((5, 3), np.float32)
    d = np.ones((5, 3), np.float32)
    # a scalar tmax is broadcast: validation passes and the call reaches the library (which has no device here)
    for t in (1.0, np.float32(2.5), np.inf, np.array(3.0)):
        with pytest.raises(prt.PrtError, match="no HIP device"):
            r.occluded(o, d, t)
    with pytest.raises(ValueError, match="tmax"):
        r.occluded(o, d, np.ones(4, np.float32))
    with pytest.raises(ValueError, match="tmax"):
        r.occluded(o, d, np.ones((5, 1), np.float32))
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        r.occluded(o, d[:4], 1.0)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        r.occluded(o.reshape(-1), d.reshape(-1), 1.0)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        r.occluded(np.zeros((5, 4), np.float32), np.zeros((5, 4), np.float32), 1.0)


def test_device_forms_validate_tensors():
    import torch
    r = _host_only()
    o = torch.zeros((5, 3), dtype=torch.float32)
    with pytest.raises(prt.PrtError, match="no HIP device"):  # host-only context: no device to put tensors on
        r.occluded(o, o, 1.0)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.closest_hit_device(o, o)


def test_hits_to_numpy_views_the_raw_records():
    import torch
    want = np.zeros(3, dtype=capi.HIT_DTYPE)
    want["prim"] = [-1, 7, 2]
    want["d2"] = [3.4e38, 1.5, 0.25]
    want["position"][1] = (1, 2, 3)
    want["normal"][2] = (0, 0, -1)
    raw = torch.from_numpy(want.view(np.int32).reshape(3, 10).copy())
    got = prt.hits_to_numpy(raw)
    assert got.dtype == np.dtype(capi.HIT_DTYPE) and got.shape == (3,)
    assert got.tobytes() == want.tobytes()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_occlusion_kernel_instances_keep_the_occupancy_of_the_walks_they_mirror():
    import resreport
    rows = {r["name"]: r for r in resreport.report()}

    def one(name):
        assert name in rows, (name, sorted(n for n in rows if "occluded" in n))
        return rows[name]

    r = one("k_occluded8_persistent<8, 5, false, true>")  # LEAN: mirrors the default closest-hit instance
    assert r["vgpr"] <= 96 and r["scratch"] == 0 and r["lds"] <= 32768 and r["occ"] >= 5, r
    r = one("k_occluded8_persistent<12, 4, true, false>")  # two-level (placed copies)
    assert r["vgpr"] <= 128 and r["scratch"] <= 16 and r["lds"] <= 40960 and r["occ"] >= 4, r
    for name, occ in (("k_occluded8_persistent<15, 4, false, false>", 4), ("k_occluded8_persistent<11, 5, false, false>", 5)):
        assert one(name)["occ"] >= occ, (name, rows[name])
    for name in ("k_pack_occlusion_rays", "k_occlusion_bytes"):
        assert one(name)["scratch"] == 0 and rows[name]["occ"] >= 8, rows[name]
    assert one("k_scan_prims_bounded")["scratch"] == 0
