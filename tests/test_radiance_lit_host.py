"""Host side of the light-sampled radiance query (include/prt.h "Radiance query", prt_radiance_lit; no GPU).

Every refusal of prt_radiance_lit and prt_radiance_lit_device is prt_radiance's, decided before a device is needed: on a
host-only context each comes back as PRT_ERR_INVALID with a message, in the header's order; what passes them fails loudly
with PRT_ERR_NO_DEVICE, whatever the lighting mode, and n == 0 is OK.  `info`, where given, is zeroed by a refused call.
The Python layer's lighting=True reaches the lit entry points, and tools/kernel_sha.py hashes the header the light-sampling
device functions moved into."""
import ctypes as C
import os

import numpy as np
import pytest

import util
from util import prt

capi = prt.capi
_fp = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)
INVALID, NO_DEVICE = 1, 2


def _ctx(with_scene=True, lighting=None):
    r = prt.HipWavefrontRenderer(device=-1)
    if with_scene:
        r.set_scene_host_only(prt.Scene("CORNELL"))
    if lighting:
        r.set_lighting(lighting)
    return r


def _call(r, q, n, o=True, d=True, rng=False, rgb=True, seg=False, info=True, device=False):
    k = max(n, 1) if n < 2 ** 20 else 1     # (refusals never touch the arrays: the huge counts get one element)
    a_o, a_d, a_rgb = (np.zeros((k, 3), np.float32) for _ in range(3))
    a_rng, a_seg = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    li = capi.PrtRadianceLitInfo(7, 7)
    pi = C.byref(li) if info else None
    qp = C.byref(q) if q is not None else None
    if device:
        p = lambda on, a: C.c_void_p(a.ctypes.data if on else None)   # noqa: E731  (never dereferenced: no device)
        rc = capi.lib().prt_radiance_lit_device(r._ctx, qp, n, p(o, a_o), p(d, a_d), p(rng, a_rng), p(rgb, a_rgb), p(seg, a_seg), pi)
    else:
        rc = capi.lib().prt_radiance_lit(r._ctx, qp, n, a_o.ctypes.data_as(_fp) if o else None, a_d.ctypes.data_as(_fp) if d else None,
                                         a_rng.ctypes.data_as(_u32p) if rng else None, a_rgb.ctypes.data_as(_fp) if rgb else None,
                                         a_seg.ctypes.data_as(_u32p) if seg else None, pi)
    if info:
        assert (li.shadow_rays, li.shadow_occluded) == (0, 0)     # a call that ran nothing reports nothing
    return rc, capi.lib().prt_last_error(r._ctx).decode()


@pytest.mark.parametrize("lighting", [None, "mis", "nee"])
@pytest.mark.parametrize("device", [False, True])
def test_refusals_need_no_device(device, lighting):
    Q = capi.PrtRadianceQuery
    ok = Q(5, 1, 0, 0)
    ctx = lambda scene=True: _ctx(scene, lighting)   # noqa: E731
    cases = [       # the header's order: query, samples, rng_state with samples > 1, the path count, scene, arrays
        ("null query", ctx(False), None, 4, {}, "query"),
        ("samples == 0", ctx(False), Q(5, 0, 0, 0), 4, {}, "samples"),
        ("samples above the cap", ctx(False), Q(5, capi.RADIANCE_MAX_SAMPLES + 1, 0, 0), 4, {}, "samples"),
        ("rng_state with samples > 1", ctx(False), Q(5, 2, 0, 0), 4, {"rng": True}, "rng_state"),
        ("n * samples above 2^32 - 1", ctx(False), Q(5, 4096, 0, 0), 2 ** 20, {}, "2^32"),
        ("n * samples above 2^32 - 1, n large", ctx(), Q(5, 2, 0, 0), 2 ** 31, {}, "2^32"),
        ("no scene", ctx(False), ok, 4, {}, "prt_set_scene"),
        ("no scene before the arrays", ctx(False), ok, 4, {"o": False}, "prt_set_scene"),
        ("null origins", ctx(), ok, 4, {"o": False}, "null array"),
        ("null dirs", ctx(), ok, 4, {"d": False}, "null array"),
        ("null rgb_sum", ctx(), ok, 4, {"rgb": False}, "null array"),
    ]
    for what, r, q, n, kw, word in cases:
        for info in (True, False):
            rc, msg = _call(r, q, n, device=device, info=info, **kw)
            assert rc == INVALID and word in msg, (what, rc, msg)
    assert capi.lib().prt_radiance_lit(None, C.byref(ok), 0, None, None, None, None, None, None) == INVALID     # no context
    r = ctx()
    assert _call(r, ok, 0, device=device)[0] == 0                       # n == 0 is OK and does nothing
    assert _call(r, ok, 0, o=False, d=False, rgb=False, info=False, device=device)[0] == 0
    assert _call(r, Q(5, 0, 0, 0), 0, device=device)[0] == INVALID      # ... but a bad query is refused whatever the count
    # at the cap, with the optional arrays, and n * samples = 2^32 - 1 exactly: valid, and there is no device to run on
    for q, n, kw in ((Q(5, capi.RADIANCE_MAX_SAMPLES, 0, 0), 4, {"seg": True}), (Q(5, 1, 0, 0), 4, {"rng": True}),
                     (Q(0, 1, 0, 0), 4, {}), (Q(5, 1, 0, 0), 2 ** 32 - 1, {}), (ok, 4, {"info": False})):
        rc, msg = _call(r, q, n, device=device, **kw)
        assert rc == NO_DEVICE and "no HIP device" in msg, (n, rc, msg)


def test_python_layer_reaches_the_lit_entry_points():
    r = _ctx(lighting="mis")
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.radiance(o, o, lighting=True)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.radiance(o, o, lighting=True, return_info=True)
    with pytest.raises(prt.PrtError, match="prt_radiance: samples"):      # the refusals are the unlit query's, word for word
        r.radiance(o, o, samples=0, lighting=True)
    with pytest.raises(prt.PrtError, match="rng_state"):
        r.radiance(o, o, rng_state=np.zeros(4, np.uint32), samples=3, lighting=True)
    with pytest.raises(ValueError):
        r.radiance(o, o[:3], lighting=True)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.render_probe((1, 2, 3), 4, 8, lighting=True)
    mean, info = r.radiance(o[:0], o[:0], lighting=True, return_info=True)      # n == 0: nothing runs, nothing is cast
    assert mean.shape == (0, 3) and info["shadow_rays"] == 0 and info["shadow_occluded"] == 0
    assert "shadow_rays" not in r.radiance(o[:0], o[:0], return_info=True)[1]   # the unlit query's info is what it was


def test_kernel_fingerprint_covers_the_light_device_header(tmp_path, monkeypatch):
    import importlib.util
    import shutil
    spec = importlib.util.spec_from_file_location("kernel_sha", os.path.join(util.ROOT, "tools", "kernel_sha.py"))
    ks = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks)
    assert os.path.exists(os.path.join(ks.CSRC, "prt_light_device.h"))
    base = ks.kernel_sha()
    copy = tmp_path / "csrc"
    shutil.copytree(ks.CSRC, copy, ignore=shutil.ignore_patterns("*.o", "*.so", "prt_render", ".build.lock"))
    monkeypatch.setattr(ks, "CSRC", str(copy))
    assert ks.kernel_sha() == base                 # the same bytes elsewhere: the same fingerprint
    with open(copy / "prt_light_device.h", "a") as f:
        f.write("// edited\n")
    assert ks.kernel_sha() != base
