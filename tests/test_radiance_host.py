"""Host side of the radiance query (include/prt.h "Radiance query"; no GPU): the probe's directions and the refusals.

probe_directions(H, W) gives the texel centres of a lat-long image in set_environment's convention.  Each direction must be a
unit vector to one fp32 ulp (2^-23: the three components are rounded once each from a float64 unit vector, which moves the
length by at most 2^-24) and must look up its own texel under the float64 mapping of tests/environment_replay.py: a centre
lies half a texel from every edge, fp32 rounding moves it by about 1e-7 texel.

Every refusal of prt_radiance that is decided before a device is needed must come back as PRT_ERR_INVALID with a message on
a host-only context; what passes them there fails loudly with PRT_ERR_NO_DEVICE, never silently."""
import ctypes as C

import numpy as np
import pytest

import environment_replay as er
import util
from util import prt

capi = prt.capi
_fp = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)
INVALID, NO_DEVICE = 1, 2


@pytest.mark.parametrize("H,W", [(4, 8), (5, 3), (16, 32)])
def test_probe_directions_are_unit_texel_centres(H, W):
    d = prt.probe_directions(H, W)
    assert d.shape == (H, W, 3) and d.dtype == np.float32
    length = np.sqrt((d.astype(np.float64) ** 2).sum(axis=-1))
    assert np.abs(length - 1.0).max() <= 2.0 ** -23, float(np.abs(length - 1.0).max())
    env = er.EnvMap(np.ones((H, W, 3), np.float32))
    i, j, edge = er.lookup64(env, d.reshape(-1, 3))
    ii, jj = np.mgrid[0:H, 0:W]
    assert np.array_equal(i, ii.ravel()) and np.array_equal(j, jj.ravel())
    assert np.abs(edge - 0.5).max() < 1e-5       # the centre: half a texel from the nearest edge
    assert d[0, :, 1].min() > 0 and d[-1, :, 1].max() < 0   # row 0 = the +Y pole


def _ctx(with_scene=True):
    r = prt.HipWavefrontRenderer(device=-1)
    if with_scene:
        r.set_scene_host_only(prt.Scene("CORNELL"))
    return r


def _call(r, q, n, o=True, d=True, rng=False, rgb=True, seg=False, device=False):
    k = max(n, 1) if n < 2 ** 20 else 1     # (refusals never touch the arrays: the huge counts get one element)
    a_o, a_d, a_rgb = (np.zeros((k, 3), np.float32) for _ in range(3))
    a_rng, a_seg = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    if device:
        p = lambda on, a: C.c_void_p(a.ctypes.data if on else None)   # noqa: E731  (never dereferenced: no device)
        rc = capi.lib().prt_radiance_device(r._ctx, C.byref(q) if q is not None else None, n, p(o, a_o), p(d, a_d), p(rng, a_rng),
                                            p(rgb, a_rgb), p(seg, a_seg))
    else:
        rc = capi.lib().prt_radiance(r._ctx, C.byref(q) if q is not None else None, n, a_o.ctypes.data_as(_fp) if o else None,
                                     a_d.ctypes.data_as(_fp) if d else None, a_rng.ctypes.data_as(_u32p) if rng else None,
                                     a_rgb.ctypes.data_as(_fp) if rgb else None, a_seg.ctypes.data_as(_u32p) if seg else None)
    return rc, capi.lib().prt_last_error(r._ctx).decode()


@pytest.mark.parametrize("device", [False, True])
def test_refusals_need_no_device(device):
    Q = capi.PrtRadianceQuery
    ok = Q(5, 1, 0, 0)
    cases = [
        ("no scene", _ctx(False), ok, 4, {}, "prt_set_scene"),
        ("null query", _ctx(), None, 4, {}, "query"),
        ("null origins", _ctx(), ok, 4, {"o": False}, "null array"),
        ("null dirs", _ctx(), ok, 4, {"d": False}, "null array"),
        ("null rgb_sum", _ctx(), ok, 4, {"rgb": False}, "null array"),
        ("samples == 0", _ctx(), Q(5, 0, 0, 0), 4, {}, "samples"),
        ("samples above the cap", _ctx(), Q(5, capi.RADIANCE_MAX_SAMPLES + 1, 0, 0), 4, {}, "samples"),
        ("rng_state with samples > 1", _ctx(), Q(5, 2, 0, 0), 4, {"rng": True}, "rng_state"),
        ("n * samples above 2^32 - 1", _ctx(), Q(5, 4096, 0, 0), 2 ** 20, {}, "2^32"),
        ("n * samples above 2^32 - 1, n large", _ctx(), Q(5, 2, 0, 0), 2 ** 31, {}, "2^32"),
    ]
    for what, r, q, n, kw, word in cases:
        rc, msg = _call(r, q, n, device=device, **kw)
        assert rc == INVALID and word in msg, (what, rc, msg)
    r = _ctx()
    assert _call(r, ok, 0, device=device)[0] == 0                       # n == 0 is OK and does nothing
    assert _call(r, ok, 0, o=False, d=False, rgb=False, device=device)[0] == 0
    assert _call(r, Q(5, 0, 0, 0), 0, device=device)[0] == INVALID      # ... but a bad query is refused whatever the count
    # at the cap, with the optional arrays, and n * samples = 2^32 - 1 exactly: valid, and there is no device to run on
    for q, n, kw in ((Q(5, capi.RADIANCE_MAX_SAMPLES, 0, 0), 4, {"seg": True}), (Q(5, 1, 0, 0), 4, {"rng": True}),
                     (Q(0, 1, 0, 0), 4, {}), (Q(5, 1, 0, 0), 2 ** 32 - 1, {})):
        rc, msg = _call(r, q, n, device=device, **kw)
        assert rc == NO_DEVICE and "no HIP device" in msg, (n, rc, msg)


def test_python_layer_refuses_without_a_device_and_checks_shapes():
    r = _ctx()
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.radiance(o, o)
    with pytest.raises(prt.PrtError, match="samples"):
        r.radiance(o, o, samples=0)
    with pytest.raises(prt.PrtError, match="rng_state"):
        r.radiance(o, o, rng_state=np.zeros(4, np.uint32), samples=3)
    with pytest.raises(ValueError):
        r.radiance(o, o[:3])
    with pytest.raises(ValueError):
        r.radiance(o, o, rng_state=np.zeros(3, np.uint32))
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.render_probe((1, 2, 3), 4, 8)
    assert util.ROOT
