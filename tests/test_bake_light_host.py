"""The texel's light sample and the lit query's scatter pdf on a host-only context (no GPU): the new symbols exist, every
refusal of prt_bake_irradiance_opt / prt_bake_light_samples / prt_radiance_lit_pb is decided before a device is asked for
(null options, reserved != 0, then the bake's and the query's own, in that order), a valid call then reports that there is
no device, and the Python layer refuses pb= and texel_light= without lighting=True."""
import ctypes as C

import numpy as np
import pytest

from parallelraytracing_amd import capi
from test_bake_host import host_context
from util import prt

F = np.float32
INVALID, NO_DEVICE = 1, 2
_fp = C.POINTER(C.c_float)


def fp(a):
    return a.ctypes.data_as(_fp)


def test_the_new_symbols_exist_and_the_struct_is_four_words():
    L = capi.lib()
    for name in ("prt_radiance_lit_pb", "prt_radiance_lit_pb_device", "prt_bake_irradiance_opt", "prt_bake_irradiance_opt_device",
                 "prt_bake_light_samples"):
        assert getattr(L, name) is not None, name
    assert C.sizeof(capi.PrtBakeOptions) == 16
    assert [n for n, _ in capi.PrtBakeOptions._fields_] == ["lighting", "texel_light", "dilate", "reserved"]


def test_options_are_refused_before_the_bakes_own_refusals():
    r, mesh, _ = host_context()
    uv = np.ascontiguousarray(mesh.GetUVs(), F)
    L = capi.lib()
    out = np.zeros((4, 4, 3), F)
    q = capi.PrtRadianceQuery(5, 1, 0, 0)
    bad_target = capi.PrtBakeTarget(7, 0, fp(uv), 4, 4)        # an unknown kind: refused too, but after the options
    good = capi.PrtBakeTarget(capi.BAKE_MESH, 0, fp(uv), 4, 4)
    for entry in (L.prt_bake_irradiance_opt, L.prt_bake_irradiance_opt_device):
        dst = fp(out) if entry is L.prt_bake_irradiance_opt else C.c_void_p(out.ctypes.data)
        assert entry(r._ctx, C.byref(bad_target), C.byref(q), None, dst, None, None) == INVALID
        assert b"null options" in L.prt_last_error(r._ctx)
        opt = capi.PrtBakeOptions(1, 1, 0, 3)
        assert entry(r._ctx, C.byref(bad_target), C.byref(q), C.byref(opt), dst, None, None) == INVALID
        assert b"reserved" in L.prt_last_error(r._ctx)
        opt = capi.PrtBakeOptions(1, 1, 0, 0)
        assert entry(r._ctx, C.byref(bad_target), C.byref(q), C.byref(opt), dst, None, None) == INVALID
        assert b"kind" in L.prt_last_error(r._ctx)
        assert entry(r._ctx, None, C.byref(q), C.byref(opt), dst, None, None) == INVALID
        assert b"null target" in L.prt_last_error(r._ctx)
        assert entry(r._ctx, C.byref(good), None, C.byref(opt), dst, None, None) == INVALID
        assert b"query" in L.prt_last_error(r._ctx)
        q0 = capi.PrtRadianceQuery(5, 0, 0, 0)
        assert entry(r._ctx, C.byref(good), C.byref(q0), C.byref(opt), dst, None, None) == INVALID
        assert b"samples" in L.prt_last_error(r._ctx)
        assert entry(r._ctx, C.byref(good), C.byref(q), C.byref(opt), None, None, None) == INVALID
        assert b"rgb_sum" in L.prt_last_error(r._ctx)
        for o in (opt, capi.PrtBakeOptions(0, 1, 2, 0), capi.PrtBakeOptions(0, 0, 0, 0)):      # valid: past every refusal
            assert entry(r._ctx, C.byref(good), C.byref(q), C.byref(o), dst, None, None) == NO_DEVICE
    fresh = prt.HipWavefrontRenderer(device=-1)                  # no scene: the bake's first refusal, after the options'
    opt = capi.PrtBakeOptions(1, 1, 0, 0)
    assert L.prt_bake_irradiance_opt(fresh._ctx, C.byref(good), C.byref(q), C.byref(opt), fp(out), None, None) == INVALID
    assert b"prt_set_scene" in L.prt_last_error(fresh._ctx)
    assert L.prt_bake_irradiance_opt(fresh._ctx, C.byref(good), C.byref(q), None, fp(out), None, None) == INVALID
    assert b"null options" in L.prt_last_error(fresh._ctx)


@pytest.mark.parametrize("kw,text", [
    (dict(mesh=1), "mesh 1"), (dict(instance=0), "placed copy"), (dict(mesh=0, size=(0, 4)), "map"), (dict(mesh=0, size=(4, 16385)), "map"),
    (dict(mesh=0, uvs=None), "no UVs"), (dict(mesh=0, uvs="nan"), "not finite"), (dict(mesh=0, uvs="big"), "2\\^20")])
def test_the_bakes_refusals_hold_for_the_new_entry_points(kw, text):
    r, mesh, _ = host_context()
    uv = mesh.GetUVs()
    kw = dict(kw)
    if "uvs" not in kw:
        kw["uvs"] = uv
    elif isinstance(kw["uvs"], str):
        bad = uv.copy()
        bad[9, 1] = {"nan": np.nan, "big": 2.0 ** 20 + 1.0}[kw["uvs"]]
        kw["uvs"] = bad
    kw.setdefault("size", (4, 4))
    with pytest.raises(prt.PrtError, match=text):
        r.bake_irradiance(lighting=True, texel_light=True, **kw)
    with pytest.raises(prt.PrtError, match=text):
        r.bake_light_samples(**kw)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.bake_irradiance(mesh=0, size=(4, 4), uvs=uv, lighting=True, texel_light=True)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.bake_light_samples(mesh=0, size=(4, 4), uvs=uv, sample=3)


def test_no_scene_is_refused_first_by_the_sample_view():
    r = prt.HipWavefrontRenderer(device=-1)
    with pytest.raises(prt.PrtError, match="prt_set_scene"):
        r.bake_light_samples(mesh=0, size=(4, 4), uvs=np.zeros((24, 2), F))
    with pytest.raises(prt.PrtError, match="prt_set_scene"):
        r.bake_irradiance(mesh=0, size=(0, 0), samples=0, lighting=True, texel_light=True)


def test_the_lit_query_with_pb_refuses_what_the_lit_query_refuses():
    r, _, _ = host_context()
    L = capi.lib()
    o, d, out = np.zeros((3, 3), F), np.ones((3, 3), F), np.zeros((3, 3), F)
    pb = np.full(3, 0.25, F)
    rng = np.arange(3, dtype=np.uint32)
    u32 = rng.ctypes.data_as(C.POINTER(C.c_uint32))
    q = capi.PrtRadianceQuery(5, 2, 0, 0)
    for pbp in (fp(pb), None):
        assert L.prt_radiance_lit_pb(r._ctx, None, 3, fp(o), fp(d), None, pbp, fp(out), None, None) == INVALID
        assert b"null query" in L.prt_last_error(r._ctx)
        q0 = capi.PrtRadianceQuery(5, 0, 0, 0)
        assert L.prt_radiance_lit_pb(r._ctx, C.byref(q0), 3, fp(o), fp(d), None, pbp, fp(out), None, None) == INVALID
        assert b"samples" in L.prt_last_error(r._ctx)
        assert L.prt_radiance_lit_pb(r._ctx, C.byref(q), 3, fp(o), fp(d), u32, pbp, fp(out), None, None) == INVALID
        assert b"rng_state" in L.prt_last_error(r._ctx)
        assert L.prt_radiance_lit_pb(r._ctx, C.byref(q), 3, None, fp(d), None, pbp, fp(out), None, None) == INVALID
        assert b"null array" in L.prt_last_error(r._ctx)
        assert L.prt_radiance_lit_pb(r._ctx, C.byref(q), 0, None, None, None, pbp, None, None, None) == 0      # n == 0: nothing to do
        assert L.prt_radiance_lit_pb(r._ctx, C.byref(q), 3, fp(o), fp(d), None, pbp, fp(out), None, None) == NO_DEVICE
        vp = C.c_void_p
        assert L.prt_radiance_lit_pb_device(r._ctx, C.byref(q0), 3, vp(o.ctypes.data), vp(d.ctypes.data), None,
                                            vp(pb.ctypes.data) if pbp else None, vp(out.ctypes.data), None, None) == INVALID
        assert L.prt_radiance_lit_pb_device(r._ctx, C.byref(q), 3, vp(o.ctypes.data), vp(d.ctypes.data), None,
                                            vp(pb.ctypes.data) if pbp else None, vp(out.ctypes.data), None, None) == NO_DEVICE
    fresh = prt.HipWavefrontRenderer(device=-1)
    assert L.prt_radiance_lit_pb(fresh._ctx, C.byref(q), 3, fp(o), fp(d), None, fp(pb), fp(out), None, None) == INVALID
    assert b"prt_set_scene" in L.prt_last_error(fresh._ctx)


def test_python_refuses_pb_and_texel_light_without_lighting():
    r, mesh, _ = host_context()
    o, d = np.zeros((3, 3), F), np.ones((3, 3), F)
    with pytest.raises(ValueError, match="lighting=True"):
        r.radiance(o, d, pb=np.zeros(3, F))
    with pytest.raises(ValueError, match="pb: 2 values for 3 rays"):
        r.radiance(o, d, lighting=True, pb=np.zeros(2, F))
    with pytest.raises(ValueError, match="lighting=True"):
        r.bake_irradiance(mesh=0, size=(4, 4), uvs=mesh.GetUVs(), texel_light=True)
    with pytest.raises(prt.PrtError, match="no HIP device"):      # the valid forms get past Python and past the refusals
        r.radiance(o, d, lighting=True, pb=np.zeros(3, F))
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.bake_irradiance(mesh=0, size=(4, 4), uvs=mesh.GetUVs(), lighting=True, texel_light=True)
