"""Refit from device arrays, the part that needs no GPU: the numpy restatement of the vertex-normal rule
(tests/refit_device_replay.py) equals what the library gives a mesh created without normals, bit for bit; the new entry
points exist, refuse a host-only context with PRT_ERR_NO_DEVICE and report zeros there."""
import ctypes as C
import os

import numpy as np
import pytest

import refit_device_replay as rr
import util
from util import prt

capi = prt.capi
PRT_ERR_NO_DEVICE = 2


def _ply(name):
    m = prt.Mesh(prt.scenes.asset(name))
    return m.GetVertices(), m.GetIndices()


MESHES = {
    "icosahedron": lambda: _ply("icosahedron.ply"),
    "cube_uv": lambda: _ply("cube_uv.ply"),
    "bunny": lambda: _ply("bunny.ply"),
    "degenerate": rr.degenerate_mesh,
}


@pytest.mark.parametrize("name", list(MESHES))
def test_restated_normals_equal_the_library_bit_for_bit(name):
    v, i = MESHES[name]()
    want = prt.Mesh(vertices=v, indices=i).GetNormals()
    got = rr.vertex_normals(v, i)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.nonzero((got != want).any(axis=1))[0][:10]
    if name == "degenerate":
        for k in (6, 7, 8, 11):   # zero-area face only / unreferenced
            assert got[k].tolist() == [0.0, 1.0, 0.0]
        assert np.all(np.isfinite(got)) and abs(float(np.linalg.norm(got[9].astype(np.float64))) - 1.0) < 1e-6


def test_corner_table_lists_every_corner_once_in_ascending_order():
    v, i = rr.degenerate_mesh()
    start, corner = rr.corner_csr(i, len(v))
    assert start[0] == 0 and start[-1] == i.size and sorted(corner.tolist()) == list(range(i.size))
    for k in range(len(v)):
        run = corner[start[k]:start[k + 1]]
        assert np.all(np.diff(run) > 0) and np.all(i.reshape(-1)[run] == k)
    assert corner[start[9]:start[10]].tolist() == [15, 16, 20] and start[12] == start[11]   # the repeated vertex once per corner, the unreferenced one never


def test_entry_points_exist_and_a_host_only_context_is_refused():
    L = capi.lib()
    for sym in ("prt_refit_meshes_device", "prt_mesh_normals_device", "prt_refit_info"):
        assert hasattr(L, sym) and sym in capi.SIGNATURES
    r = prt.HipWavefrontRenderer(device=-1)
    info = r.refit_info()
    assert set(info) == {"refits", "last_form", "normals_computed", "host_copies_stale", "device_ms", "wall_ms", "h2d_bytes", "d2h_bytes"}
    assert all(v == 0 for v in info.values())
    mesh = prt.Mesh(prt.scenes.asset("icosahedron.ply"))
    r.set_scene_host_only(prt.scenes.mesh_scene(mesh))
    arr = (capi.PrtMeshDeviceArrays * 1)()
    assert L.prt_refit_meshes_device(r._ctx, arr, 1) == PRT_ERR_NO_DEVICE
    assert L.prt_mesh_normals_device(r._ctx, 0, None, None) == PRT_ERR_NO_DEVICE
    assert all(v == 0 for v in r.refit_info().values())
    assert C.sizeof(capi.PrtRefitInfo) == 40 and C.sizeof(capi.PrtMeshDeviceArrays) == 16
    assert L.prt_refit_info(r._ctx, None) != 0
