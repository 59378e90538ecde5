"""Surface baking on a host-only context (no GPU): every refusal of include/prt.h "Surface baking" is decided before a
device is asked for, in the order of the header, and a valid call then reports that there is no device.  The scene stays
usable: the same context answers a valid call the same way afterwards."""
import ctypes as C

import numpy as np
import pytest

import bake_replay as br
from parallelraytracing_amd import capi
from util import prt

F = np.float32


def host_context(textures=False):
    mesh = br.cube_mesh()
    sc = prt.scenes.mesh_scene(mesh)
    if textures:
        sc.SetMaterialTexture(2, sc.AddTexture(prt.scenes.checker(4)))
    r = prt.HipWavefrontRenderer(device=-1)
    r.set_scene_host_only(sc)
    return r, mesh, sc


def test_no_scene_is_refused_first():
    r = prt.HipWavefrontRenderer(device=-1)
    with pytest.raises(prt.PrtError, match="prt_set_scene"):
        r.bake_surface(mesh=0, size=(4, 4), uvs=np.zeros((24, 2), F))
    with pytest.raises(prt.PrtError, match="prt_set_scene"):
        r.bake_irradiance(mesh=0, size=(0, 0), samples=0)


@pytest.mark.parametrize("kw,text", [
    (dict(mesh=1), "mesh 1"), (dict(instance=0), "placed copy"), (dict(mesh=0, size=(0, 4)), "map"), (dict(mesh=0, size=(4, 16385)), "map"),
    (dict(mesh=0, uvs=None), "no UVs"), (dict(mesh=0, uvs="nan"), "not finite"), (dict(mesh=0, uvs="inf"), "not finite"),
    (dict(mesh=0, uvs="big"), "2\\^20"), (dict(mesh=0, samples=0), "samples"), (dict(mesh=0, samples=4097), "samples")])
def test_refusals_are_decided_without_a_device(kw, text):
    r, mesh, _ = host_context()
    uv = mesh.GetUVs()
    special = {"nan": np.nan, "inf": -np.inf, "big": 2.0 ** 20 + 1.0}
    kw = dict(kw)
    if "uvs" not in kw:
        kw["uvs"] = uv
    elif isinstance(kw["uvs"], str):
        bad = uv.copy()
        bad[9, 1] = special[kw["uvs"]]
        kw["uvs"] = bad
    kw.setdefault("size", (4, 4))
    with pytest.raises(prt.PrtError, match=text):
        r.bake_irradiance(**kw)
    if "samples" not in kw:
        for fn in (r.bake_surface, r.bake_rays):
            with pytest.raises(prt.PrtError, match=text):
                fn(**kw)
    with pytest.raises(prt.PrtError, match="no HIP device"):      # the scene is still there, and the valid call gets past the refusals
        r.bake_irradiance(mesh=0, size=(4, 4), uvs=uv)


def test_unknown_kind_null_target_and_null_query():
    r, mesh, _ = host_context()
    uv = np.ascontiguousarray(mesh.GetUVs(), F)
    L = capi.lib()
    t = capi.PrtBakeTarget(7, 0, uv.ctypes.data_as(C.POINTER(C.c_float)), 4, 4)
    assert L.prt_bake_surface(r._ctx, C.byref(t), None, None, None, None, None) == 1      # PRT_ERR_INVALID
    assert b"kind" in L.prt_last_error(r._ctx)
    assert L.prt_bake_surface(r._ctx, None, None, None, None, None, None) == 1
    t.kind = capi.BAKE_MESH
    out = np.zeros((4, 4, 3), F)
    assert L.prt_bake_irradiance(r._ctx, C.byref(t), None, 0, 0, out.ctypes.data_as(C.POINTER(C.c_float)), None, None) == 1
    assert b"query" in L.prt_last_error(r._ctx)
    q = capi.PrtRadianceQuery(5, 1, 0, 0)
    assert L.prt_bake_irradiance(r._ctx, C.byref(t), C.byref(q), 0, 0, out.ctypes.data_as(C.POINTER(C.c_float)), None, None) == 2   # PRT_ERR_NO_DEVICE
    big = capi.PrtBakeTarget(capi.BAKE_MESH, 0, uv.ctypes.data_as(C.POINTER(C.c_float)), 16384, 16384)
    q = capi.PrtRadianceQuery(5, 16, 0, 0)                  # 2^28 texels x 16 samples = 2^32 paths
    assert L.prt_bake_irradiance(r._ctx, C.byref(big), C.byref(q), 0, 0, out.ctypes.data_as(C.POINTER(C.c_float)), None, None) == 1
    assert b"2^32" in L.prt_last_error(r._ctx)


def test_binding_supplies_uvs_only_where_the_set_had_them():
    r, mesh, _ = host_context(textures=True)        # the cube's material is textured: the binding carries the PLY's UVs
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.bake_surface(mesh=0, size=(4, 4))
    bare = prt.Mesh(vertices=mesh.GetVertices(), normals=mesh.GetNormals(), indices=mesh.GetIndices())
    sc = prt.scenes.mesh_scene(bare)
    sc.SetMaterialTexture(0, sc.AddTexture(prt.scenes.checker(4)))      # a binding, but none of its UVs are this mesh's
    r2 = prt.HipWavefrontRenderer(device=-1)
    r2.set_scene_host_only(sc)
    with pytest.raises(prt.PrtError, match="no UVs"):
        r2.bake_surface(mesh=0, size=(4, 4))


def test_bake_chunk_is_a_parameter():
    r, _, _ = host_context()
    r.set_param("bake_chunk", 2)
    r.set_param("bake_chunk", 0)
    with pytest.raises(prt.PrtError):
        r.set_param("bake_chunk", -1)
    with pytest.raises(prt.PrtError):
        r.set_param("bake_chunk", 4097)
