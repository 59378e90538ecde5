"""CPU-side tests of the denoiser's interface (include/prt.h "First-hit feature images and the edge-avoiding film denoiser"):
every refusal of prt_denoise / prt_denoise_device / prt_film_denoise on a host-only context (they are checked before the
device is asked for), the ctypes struct, the defaults, and the symbols."""
import ctypes as C

import numpy as np
import pytest

from util import prt

capi = prt.capi
NAN = float("nan")
INVALID, NO_DEVICE = 1, 2  # PRT_ERR_INVALID, PRT_ERR_NO_DEVICE
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


def test_struct_defaults_and_symbols():
    assert C.sizeof(capi.PrtDenoise) == 20 and capi.PrtDenoise.demodulate.offset == 16
    k = capi.PrtDenoise()
    capi.lib().prt_denoise_defaults(C.byref(k))
    assert (k.iterations, k.sigma_l, k.normal_power_log2, k.demodulate) == (5, 4.0, 6, 1) and k.sigma_z == np.float32(0.1)
    capi.lib().prt_denoise_defaults(None)
    assert capi.DENOISE_MAX_PIXELS == 1 << 28
    for name in ("prt_denoise_defaults", "prt_denoise_variance", "prt_render_features", "prt_features_read", "prt_denoise",
                 "prt_denoise_device", "prt_film_denoise", "prt_group_film_denoise"):
        assert name in capi.SIGNATURES and getattr(capi.lib(), name)
    for cls in (prt.HipWavefrontRenderer, prt.HipWavefrontGroupRenderer):
        assert callable(cls.render_features) and callable(cls.denoise)
    assert callable(prt.HipWavefrontRenderer.denoise_arrays)


def _arrays(W=4, H=3):
    z3 = np.zeros((H, W, 3), np.float32)
    return dict(mean=z3.copy(), var=np.zeros((H, W), np.float32), albedo=z3.copy() + 1, normal=z3.copy(), position=z3.copy(),
                prim=np.zeros((H, W), np.int32), out=z3.copy())


def _call(r, cfg=None, W=4, H=3, null=None, device=False, **fields):
    k = capi.PrtDenoise()
    capi.lib().prt_denoise_defaults(C.byref(k))
    for name, v in fields.items():
        setattr(k, name, v)
    a = _arrays()
    if device:
        ptr = {n: (None if n == null else C.c_void_p(a[n].ctypes.data)) for n in a}  # never dereferenced: there is no device
        return capi.lib().prt_denoise_device(r._ctx, C.byref(k) if cfg is None else cfg, W, H, ptr["mean"], ptr["var"], ptr["albedo"],
                                             ptr["normal"], ptr["position"], ptr["prim"], ptr["out"], None)
    ptr = {n: (None if n == null else a[n].ctypes.data_as(_ip if n == "prim" else _fp)) for n in a}
    return capi.lib().prt_denoise(r._ctx, C.byref(k) if cfg is None else cfg, W, H, ptr["mean"], ptr["var"], ptr["albedo"],
                                  ptr["normal"], ptr["position"], ptr["prim"], ptr["out"], None)


REFUSALS = [
    ("iterations 7", dict(iterations=7)), ("sigma_l 0", dict(sigma_l=0.0)), ("sigma_l negative", dict(sigma_l=-1.0)),
    ("sigma_l nan", dict(sigma_l=NAN)), ("sigma_z 0", dict(sigma_z=0.0)), ("sigma_z negative", dict(sigma_z=-0.1)),
    ("sigma_z nan", dict(sigma_z=NAN)), ("normal_power_log2 9", dict(normal_power_log2=9)),
    ("W = 0", dict(W=0)), ("H = 0", dict(H=0)), ("above 2^28 pixels", dict(W=1 << 15, H=(1 << 13) + 1)),
    ("the product wraps 32 bits", dict(W=1 << 16, H=1 << 16)),
] + [(f"null {n}", dict(null=n)) for n in ("mean", "var", "albedo", "normal", "position", "prim", "out")]


@pytest.mark.parametrize("device", [False, True], ids=["host arrays", "device arrays"])
@pytest.mark.parametrize("what,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_on_a_host_only_context(what, kw, device):
    r = prt.HipWavefrontRenderer(device=-1)
    assert _call(r, device=device, **kw) == INVALID, what
    assert capi.lib().prt_last_error(r._ctx).decode().startswith("denoise:")


def test_valid_settings_reach_the_device_check():
    r = prt.HipWavefrontRenderer(device=-1)
    assert _call(r) == NO_DEVICE and _call(r, device=True) == NO_DEVICE
    assert _call(r, iterations=0) == NO_DEVICE and _call(r, iterations=6, normal_power_log2=8) == NO_DEVICE
    assert _call(r, normal_power_log2=0, demodulate=0, sigma_l=1e-30, sigma_z=float("inf")) == NO_DEVICE
    assert _call(r, W=1 << 14, H=1 << 14) == NO_DEVICE                      # exactly 2^28 pixels
    a = _arrays()
    L = capi.lib()
    args = [a[n].ctypes.data_as(_ip if n == "prim" else _fp) for n in ("mean", "var", "albedo", "normal", "position", "prim", "out")]
    assert L.prt_denoise(r._ctx, None, 4, 3, *args, None) == NO_DEVICE     # NULL = the defaults
    assert L.prt_denoise(None, None, 4, 3, *args, None) == INVALID
    with pytest.raises(prt.PrtError):
        r.denoise_arrays(a["mean"], a["var"], a["albedo"], a["normal"], a["position"], a["prim"])
    with pytest.raises(TypeError):
        r.denoise_arrays(a["mean"], a["var"], a["albedo"], a["normal"], a["position"], a["prim"], sigma=1.0)
    with pytest.raises(ValueError):
        r.denoise_arrays(a["mean"], a["var"][:2], a["albedo"], a["normal"], a["position"], a["prim"])


def test_film_denoise_and_features_on_a_host_only_context():
    L = capi.lib()
    r = prt.HipWavefrontRenderer(device=-1)
    out = np.zeros((3, 4, 3), np.float32)
    po = out.ctypes.data_as(_fp)
    assert L.prt_film_denoise(r._ctx, None, po, None) == INVALID            # statistics off
    assert b"statistics" in L.prt_last_error(r._ctx)
    r.set_film_statistics(True)
    assert L.prt_film_denoise(r._ctx, None, None, None) == INVALID          # a null array
    bad = capi.PrtDenoise(7, 4.0, 0.1, 6, 1)
    assert L.prt_film_denoise(r._ctx, C.byref(bad), po, None) == INVALID
    assert L.prt_film_denoise(r._ctx, None, po, None) == NO_DEVICE
    # a partitioned film is refused with a message that names the group call, before the device is asked for
    assert L.prt_set_film(r._ctx, 16, 16, 1, 3) == 0
    assert L.prt_film_denoise(r._ctx, None, po, None) == INVALID
    assert b"prt_group_film_denoise" in L.prt_last_error(r._ctx)
    assert L.prt_render_features(r._ctx) == NO_DEVICE
    assert L.prt_features_read(r._ctx, None, None, None, None, None) == INVALID   # no current feature set
    assert L.prt_features_read(None, None, None, None, None, None) == INVALID
    assert L.prt_group_film_denoise(None, None, po, None) == INVALID
