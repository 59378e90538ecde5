"""Host-side mirror of the reference's scene / camera / film / renderer interfaces, over the C-ABI.

Same names and call contract as the reference (C++) so that callers and tests read alike:
  Scene(preset)                      src/core/scene.h:17-62
  Mesh(ply_path)                     src/core/mesh.h:8-21
  Camera(position, front, w, h)      src/core/camera.h:7-16
  Film(width, height)                src/core/film.h:10-47
  HipWavefrontRenderer.Init / ProgressiveRender / SetCamera     src/core/renderer.h:8-16
Nothing here computes pixels: every method marshals PODs into libprt.so (HIP).  A C++ adapter with the
same shape lives in host/prt_renderer.hpp.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Tuple

import numpy as np

from . import capi
from .capi import (PrtBvhInfo, PrtCameraDesc, PrtHit, PrtInstance, PrtMaterial, PrtMesh, PrtPrimitive, PrtSampling,
                   PrtSceneDesc, PrtStats)

_fp = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)

SKY = (0.4, 0.3, 0.6)  # src/backend/cpu/renderer.h:31
DEFAULT_MAX_DEPTH = 20  # src/backend/cpu/renderer.h:34


class PrtError(RuntimeError):
    pass


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def glm_normalize(v) -> np.ndarray:
    """glm::normalize in fp32: v * (1 / sqrt((x*x + y*y) + z*z))."""
    v = np.asarray(v, np.float32)
    d = np.float32(np.float32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return (v * np.float32(np.float32(1.0) / np.sqrt(d))).astype(np.float32)


def make_transform(scale, euler_deg, translation) -> Tuple[np.ndarray, np.ndarray]:
    """Scene::MakeTransform (src/core/scene.cpp:9-17): column-major mat and inverse."""
    s, e, t = _f32(scale), _f32(euler_deg), _f32(translation)
    mat = np.empty(16, np.float32)
    inv = np.empty(16, np.float32)
    capi.lib().prt_make_transform(s.ctypes.data_as(_fp), e.ctypes.data_as(_fp), t.ctypes.data_as(_fp),
                                  mat.ctypes.data_as(_fp), inv.ctypes.data_as(_fp))
    return mat, inv


class Mesh:
    """Triangle mesh: vertices / normals / indices, as the reference's Mesh (src/core/mesh.h:12-14)."""

    def __init__(self, ply_path: Optional[str] = None, *, vertices=None, normals=None, indices=None, uvs=None):
        L = capi.lib()
        h = C.c_void_p()
        if ply_path is not None:
            err = C.create_string_buffer(256)
            rc = L.prt_mesh_load_ply(ply_path.encode(), C.byref(h), err, len(err))
            if rc:
                raise PrtError(f"PLY load failed ({ply_path}): {err.value.decode()}")
        else:
            v = _f32(vertices).reshape(-1, 3)
            i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
            n = None if normals is None else _f32(normals).reshape(-1, 3)
            rc = L.prt_mesh_create(v.ctypes.data_as(_fp), None if n is None else n.ctypes.data_as(_fp), v.shape[0],
                                   i.ctypes.data_as(_u32p), i.shape[0], C.byref(h))
            if rc:
                raise PrtError("prt_mesh_create failed (index out of range?)")
        self._h = h
        if uvs is not None:
            self.SetUVs(uvs)

    def __del__(self):
        if getattr(self, "_h", None):
            capi.lib().prt_mesh_free(self._h)
            self._h = None

    @property
    def n_vertices(self) -> int:
        return capi.lib().prt_mesh_vertex_count(self._h)

    @property
    def n_triangles(self) -> int:
        return capi.lib().prt_mesh_triangle_count(self._h)

    @property
    def had_normals(self) -> bool:
        return bool(capi.lib().prt_mesh_had_normals(self._h))

    def GetVertices(self) -> np.ndarray:
        return np.ctypeslib.as_array(capi.lib().prt_mesh_positions(self._h), (self.n_vertices, 3)).copy()

    def GetNormals(self) -> np.ndarray:
        return np.ctypeslib.as_array(capi.lib().prt_mesh_normals(self._h), (self.n_vertices, 3)).copy()

    def GetIndices(self) -> np.ndarray:
        return np.ctypeslib.as_array(capi.lib().prt_mesh_indices(self._h), (self.n_triangles, 3)).copy()

    @property
    def had_uvs(self) -> bool:
        return bool(capi.lib().prt_mesh_had_uvs(self._h))

    def GetUVs(self) -> Optional[np.ndarray]:
        """Per-vertex texture coordinates [n_vertices, 2] (a PLY's s/t, u/v or texture_u/texture_v), or None."""
        p = capi.lib().prt_mesh_uvs(self._h)
        return np.ctypeslib.as_array(p, (self.n_vertices, 2)).copy() if p else None

    def SetUVs(self, uvs) -> "Mesh":
        """uvs [n_vertices, 2], or None to drop them."""
        if uvs is None:
            capi.lib().prt_mesh_set_uvs(self._h, None)
            return self
        a = _f32(uvs)
        if a.shape != (self.n_vertices, 2):
            raise ValueError(f"uvs: shape {a.shape}, expected ({self.n_vertices}, 2)")
        if capi.lib().prt_mesh_set_uvs(self._h, a.ctypes.data_as(_fp)):
            raise PrtError("prt_mesh_set_uvs failed")
        return self

    def refine(self, target_triangles: int) -> "Mesh":
        if capi.lib().prt_mesh_refine(self._h, int(target_triangles)):
            raise PrtError("prt_mesh_refine failed (non-manifold edge)")
        return self

    def transform(self, mat, inv) -> "Mesh":
        m, i = _f32(mat), _f32(inv)
        capi.lib().prt_mesh_transform(self._h, m.ctypes.data_as(_fp), i.ctypes.data_as(_fp))
        return self

    def append(self, other: "Mesh") -> "Mesh":
        capi.lib().prt_mesh_append(self._h, other._h)
        return self

    def copy(self) -> "Mesh":
        return Mesh(vertices=self.GetVertices(), normals=self.GetNormals(), indices=self.GetIndices(), uvs=self.GetUVs())


class Scene:
    """Materials + analytic primitives (+ triangle meshes).  Scene(preset) reproduces the reference's
    hard-coded presets (src/core/scene.cpp:42-55); the default preset is RANDOM_BALLS_LARGE
    (src/core/scene.h:20).  preset=None gives an empty scene to fill by hand."""

    def __init__(self, preset: Optional[str] = "RANDOM_BALLS_LARGE", sky=SKY):
        self.materials: List[PrtMaterial] = []
        self.primitives: List[PrtPrimitive] = []
        self.meshes: List[Tuple[Mesh, int]] = []
        self.instanced_meshes: List[Mesh] = []
        self.instances: List[PrtInstance] = []
        self.sky = tuple(float(x) for x in sky)
        self.textures: List[Tuple[np.ndarray, int, int]] = []  # (rgb [H, W, 3], filter, wrap)
        self.material_texture: dict = {}                       # material -> texture
        self._keep = None
        self._keep_tex = None
        if preset is not None:
            pid = capi.PRESET_NAMES[preset] if isinstance(preset, str) else int(preset)
            nm, npr = C.c_uint32(0), C.c_uint32(0)
            if capi.lib().prt_scene_preset(pid, None, C.byref(nm), None, C.byref(npr)):
                raise PrtError(f"unknown preset {preset}")
            mats = (PrtMaterial * nm.value)()
            prims = (PrtPrimitive * npr.value)()
            capi.lib().prt_scene_preset(pid, mats, C.byref(nm), prims, C.byref(npr))
            self.materials = list(mats)
            self.primitives = list(prims)

    # MaterialPool::Add* (src/core/material.h:170-192)
    def _add_material(self, mtype, rgb, scalar) -> int:
        m = PrtMaterial()
        m.type = mtype
        m.rgb[:] = [float(x) for x in rgb]
        m.scalar = float(scalar)
        self.materials.append(m)
        return len(self.materials) - 1

    def AddLambertian(self, albedo) -> int:
        return self._add_material(capi.MAT_LAMBERTIAN, albedo, 0.0)

    def AddMetal(self, albedo, roughness) -> int:
        return self._add_material(capi.MAT_METAL, albedo, roughness)

    def AddDielectric(self, ri) -> int:
        return self._add_material(capi.MAT_DIELECTRIC, (0, 0, 0), ri)

    def AddEmissive(self, emission) -> int:
        return self._add_material(capi.MAT_EMISSIVE, emission, 0.0)

    # Scene::AddPrimitive (src/core/scene.cpp:19-36)
    def _add_prim(self, shape, p0, p1, material, scale, euler_deg, translation):
        p = PrtPrimitive()
        p.shape_type = shape
        p.shape_param[0] = float(p0)
        p.shape_param[1] = float(p1)
        p.material_id = int(material)
        mat, inv = make_transform(scale, euler_deg, translation)
        p.mat[:] = mat.tolist()
        p.inv[:] = inv.tolist()
        # (scale, euler, translation) the record was made from: a Python-side note for tools that rebuild a scene under another
        # transform (tests/scale_cases.py); not part of the C record, lost on a copy of it
        p.srt = (tuple(float(v) for v in scale), tuple(float(v) for v in euler_deg), tuple(float(v) for v in translation))
        self.primitives.append(p)

    def AddCircle(self, radius, material, scale=(1, 1, 1), euler_deg=(0, 0, 0), translation=(0, 0, 0)):
        self._add_prim(capi.SHAPE_CIRCLE, radius, 0.0, material, scale, euler_deg, translation)

    def AddQuad(self, width, height, material, scale=(1, 1, 1), euler_deg=(0, 0, 0), translation=(0, 0, 0)):
        self._add_prim(capi.SHAPE_QUAD, width, height, material, scale, euler_deg, translation)

    def AddMesh(self, mesh: Mesh, material: int):
        """World-space triangles (identity Transform); appended after all analytic primitives."""
        self.meshes.append((mesh, int(material)))

    def AddInstance(self, mesh: Mesh, material: int, scale=1.0, euler_deg=(0, 0, 0), translation=(0, 0, 0)):
        """A placed copy of `mesh`: Triangle primitives sharing one Transform (src/core/primitive.h:7-12), built by
        Scene::MakeTransform (src/core/scene.cpp:9-17).  Uniform scale only (include/prt.h, PrtInstance)."""
        for k, m in enumerate(self.instanced_meshes):
            if m is mesh:
                mi = k
                break
        else:
            self.instanced_meshes.append(mesh)
            mi = len(self.instanced_meshes) - 1
        inst = PrtInstance()
        inst.mesh = mi
        inst.material_id = int(material)
        sc = (scale, scale, scale) if np.isscalar(scale) else scale
        mat, inv = make_transform(sc, euler_deg, translation)
        inst.mat[:] = mat.tolist()
        inst.inv[:] = inv.tolist()
        inst.srt = (tuple(float(v) for v in sc), tuple(float(v) for v in euler_deg), tuple(float(v) for v in translation))
        self.instances.append(inst)
        return len(self.instances) - 1

    def SetInstanceTransform(self, i: int, scale=1.0, euler_deg=(0, 0, 0), translation=(0, 0, 0)):
        """Placed copy `i` (the index AddInstance returned) gets a new transform; arguments as for AddInstance.  A renderer
        initialised with this scene follows through UpdateInstances (no rebuild of any mesh tree)."""
        inst = self.instances[i]
        sc = (scale, scale, scale) if np.isscalar(scale) else scale
        mat, inv = make_transform(sc, euler_deg, translation)
        inst.mat[:] = mat.tolist()
        inst.inv[:] = inv.tolist()
        inst.srt = (tuple(float(v) for v in sc), tuple(float(v) for v in euler_deg), tuple(float(v) for v in translation))

    # ---- image textures (include/prt.h "Image textures") ----
    def AddTexture(self, rgb, filter="nearest", wrap="repeat") -> int:
        """An image [H, W, 3] of albedo, row 0 = top; filter "nearest" | "bilinear", wrap "repeat" | "clamp"."""
        a = _f32(rgb).copy()
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("texture: rgb must be [H, W, 3]")
        f = capi.TEX_FILTERS[filter] if isinstance(filter, str) else int(filter)
        w = capi.TEX_WRAPS[wrap] if isinstance(wrap, str) else int(wrap)
        self.textures.append((a, f, w))
        return len(self.textures) - 1

    def SetMaterialTexture(self, material: int, texture: Optional[int]):
        """The albedo of a Lambertian or Metal material comes from `texture` (an index AddTexture returned); None: its rgb."""
        if texture is None:
            self.material_texture.pop(int(material), None)
        else:
            self.material_texture[int(material)] = int(texture)

    def texture_set(self) -> Optional["capi.PrtTextureSet"]:
        """The PrtTextureSet of this scene (meshes' UVs included), or None if it has no textures at all."""
        if not self.textures and not self.material_texture:
            return None
        L = capi.lib()
        tex = (capi.PrtTexture * max(1, len(self.textures)))()
        for k, (a, f, w) in enumerate(self.textures):
            tex[k].rgb = a.ctypes.data_as(_fp)
            tex[k].width, tex[k].height, tex[k].filter, tex[k].wrap = a.shape[1], a.shape[0], f, w
        mt = (C.c_uint32 * max(1, len(self.materials)))(*[self.material_texture.get(m, capi.TEXTURE_NONE)
                                                        for m in range(len(self.materials))])
        uv = (_fp * max(1, len(self.meshes)))(*[L.prt_mesh_uvs(m._h) for m, _ in self.meshes])
        iuv = (_fp * max(1, len(self.instanced_meshes)))(*[L.prt_mesh_uvs(m._h) for m in self.instanced_meshes])
        ts = capi.PrtTextureSet(tex, len(self.textures), mt, len(self.materials), uv, len(self.meshes), iuv,
                                len(self.instanced_meshes))
        self._keep_tex = (tex, mt, uv, iuv)
        return ts

    @property
    def n_triangles(self) -> int:
        return (sum(m.n_triangles for m, _ in self.meshes)
                + sum(self.instanced_meshes[i.mesh].n_triangles for i in self.instances))

    def desc(self) -> PrtSceneDesc:
        mats = (PrtMaterial * max(1, len(self.materials)))(*self.materials)
        prims = (PrtPrimitive * max(1, len(self.primitives)))(*self.primitives)
        meshes = (PrtMesh * max(1, len(self.meshes)))()
        L = capi.lib()
        for i, (m, mat) in enumerate(self.meshes):
            meshes[i].positions = L.prt_mesh_positions(m._h)
            meshes[i].normals = L.prt_mesh_normals(m._h)
            meshes[i].indices = L.prt_mesh_indices(m._h)
            meshes[i].n_vertices = m.n_vertices
            meshes[i].n_triangles = m.n_triangles
            meshes[i].material_id = mat
        d = PrtSceneDesc()
        d.materials = mats
        d.primitives = prims
        d.meshes = meshes
        d.n_materials = len(self.materials)
        d.n_primitives = len(self.primitives)
        d.n_meshes = len(self.meshes)
        d.sky[:] = self.sky
        imeshes = (PrtMesh * max(1, len(self.instanced_meshes)))()
        for i, m in enumerate(self.instanced_meshes):
            imeshes[i].positions = L.prt_mesh_positions(m._h)
            imeshes[i].normals = L.prt_mesh_normals(m._h)
            imeshes[i].indices = L.prt_mesh_indices(m._h)
            imeshes[i].n_vertices = m.n_vertices
            imeshes[i].n_triangles = m.n_triangles
        insts = (PrtInstance * max(1, len(self.instances)))(*self.instances)
        d.instanced_meshes = imeshes
        d.instances = insts
        d.n_instanced_meshes = len(self.instanced_meshes)
        d.n_instances = len(self.instances)
        self._keep = (mats, prims, meshes, imeshes, insts)
        return d


class Camera:
    """Camera(position, front, width, height) (src/core/camera.h:10-16); main() places it at (5,5,8)
    looking at the origin (src/main.cpp:142-150)."""

    def __init__(self, position=(5.0, 5.0, 8.0), front=None, width=1920.0, height=1080.0):
        self.position = tuple(float(x) for x in position)
        if front is None:  # glm::normalize(focus - center) with focus = origin (src/main.cpp:142-146)
            front = glm_normalize(-np.asarray(self.position, np.float32))
        self.front = tuple(float(x) for x in front)
        self.width = float(width)
        self.height = float(height)

    def desc(self) -> PrtCameraDesc:
        d = PrtCameraDesc()
        d.position[:] = self.position
        d.front[:] = self.front
        d.width = self.width
        d.height = self.height
        return d


class Film:
    """Accumulation buffer (src/core/film.h:10-76).  The sums live on the GPU; accum / weights are the
    host copies filled by HipWavefrontRenderer.download()."""

    def __init__(self, width: int, height: int):
        self.width = int(width)
        self.height = int(height)
        self.accum = np.zeros((self.height, self.width, 3), np.float32)
        self.weights = np.zeros((self.height, self.width), np.float32)
        self.display = np.zeros((self.height, self.width, 4), np.uint8)
        self._renderer = None

    def GetWidth(self):
        return self.width

    def GetHeight(self):
        return self.height

    def Clear(self):
        self.accum[:] = 0
        self.weights[:] = 0
        self.display[:] = 0
        if self._renderer is not None:
            self._renderer._check(capi.lib().prt_film_clear(self._renderer._ctx))

    def mean(self) -> np.ndarray:
        w = np.maximum(self.weights, 1e-30)[..., None]
        return np.where(self.weights[..., None] > 0, self.accum / w, 0.0).astype(np.float32)


def device_memory_info() -> Tuple[int, int]:
    """(live_bytes, alloc_calls) of prt_device_memory_info: device bytes the library's contexts own now, allocation calls so far."""
    live, calls = C.c_uint64(0), C.c_uint64(0)
    capi.lib().prt_device_memory_info(C.byref(live), C.byref(calls))
    return int(live.value), int(calls.value)


def hits_to_numpy(t) -> np.ndarray:
    """The [n, 10] int32 tensor of HipWavefrontRenderer.closest_hit_device as PrtHit records (capi.HIT_DTYPE)."""
    a = np.ascontiguousarray(t.cpu().numpy(), dtype=np.int32).reshape(-1, 10)
    return a.view(np.dtype(capi.HIT_DTYPE)).reshape(-1)


def _denoise_config(**cfg) -> "capi.PrtDenoise":
    """PrtDenoise with the library's defaults (prt_denoise_defaults), then the given fields."""
    k = capi.PrtDenoise()
    capi.lib().prt_denoise_defaults(C.byref(k))
    for name, v in cfg.items():
        if name in ("sigma_l", "sigma_z"):
            setattr(k, name, float(v))
        elif name in ("iterations", "normal_power_log2", "demodulate"):
            setattr(k, name, int(v))
        else:
            raise TypeError(f"denoise: unknown setting {name!r} (iterations, sigma_l, sigma_z, normal_power_log2, demodulate)")
    return k


def _temporal_config(**cfg) -> "capi.PrtTemporal":
    """PrtTemporal with the library's defaults (prt_temporal_defaults), then the given fields."""
    k = capi.PrtTemporal()
    capi.lib().prt_temporal_defaults(C.byref(k))
    for name, v in cfg.items():
        if name not in ("max_history", "normal_min", "plane_tol"):
            raise TypeError(f"temporal: unknown setting {name!r} (max_history, normal_min, plane_tol)")
        setattr(k, name, float(v))
    return k


def _basis_dict(k: "capi.PrtCameraBasis") -> dict:
    d = {name: np.array(list(getattr(k, name)), np.float32) for name in ("pos", "right", "up", "front")}
    d.update(W=np.float32(k.W), H=np.float32(k.H), tan_fov_y=np.float32(k.tan_fov_y))
    return d


def _basis_struct(d) -> "capi.PrtCameraBasis":
    if isinstance(d, capi.PrtCameraBasis):
        return d
    k = capi.PrtCameraBasis()
    for name in ("pos", "right", "up", "front"):
        v = np.asarray(d[name], np.float32).reshape(3)
        setattr(k, name, (C.c_float * 3)(*[float(x) for x in v]))
    k.W, k.H, k.tan_fov_y = float(d["W"]), float(d["H"]), float(d["tan_fov_y"])
    return k


def _read_features(check, ctx, W: int, H: int) -> dict:
    L = capi.lib()
    check(L.prt_render_features(ctx))
    out = dict(albedo=np.zeros((H, W, 3), np.float32), normal=np.zeros((H, W, 3), np.float32),
               position=np.zeros((H, W, 3), np.float32), depth=np.zeros((H, W), np.float32), prim=np.zeros((H, W), np.int32))
    check(L.prt_features_read(ctx, out["albedo"].ctypes.data_as(_fp), out["normal"].ctypes.data_as(_fp),
                              out["position"].ctypes.data_as(_fp), out["depth"].ctypes.data_as(_fp),
                              out["prim"].ctypes.data_as(C.POINTER(C.c_int32))))
    ft = capi.PrtFeatureTrace()
    check(L.prt_get_feature_trace(ctx, C.byref(ft)))
    if ft.max_specular > 0:   # the guide set through specular chains, beside the first-hit set
        g = dict(albedo=np.zeros((H, W, 3), np.float32), normal=np.zeros((H, W, 3), np.float32),
                 position=np.zeros((H, W, 3), np.float32), depth=np.zeros((H, W), np.float32), prim=np.zeros((H, W), np.int32),
                 bounces=np.zeros((H, W), np.uint32))
        check(L.prt_features_read_guide(ctx, g["albedo"].ctypes.data_as(_fp), g["normal"].ctypes.data_as(_fp),
                                        g["position"].ctypes.data_as(_fp), g["depth"].ctypes.data_as(_fp),
                                        g["prim"].ctypes.data_as(C.POINTER(C.c_int32)), g["bounces"].ctypes.data_as(_u32p)))
        out["guide"] = g
    fs = capi.PrtFeatureSampling()
    check(L.prt_get_feature_sampling(ctx, C.byref(fs)))
    if fs.samples > 0:        # the sampled set: the render's own primary rays averaged per pixel
        g = dict(albedo=np.zeros((H, W, 3), np.float32), normal=np.zeros((H, W, 3), np.float32),
                 position=np.zeros((H, W, 3), np.float32), depth=np.zeros((H, W), np.float32), prim=np.zeros((H, W), np.int32),
                 hits=np.zeros((H, W), np.uint32))
        check(L.prt_features_read_sampled(ctx, g["albedo"].ctypes.data_as(_fp), g["normal"].ctypes.data_as(_fp),
                                          g["position"].ctypes.data_as(_fp), g["depth"].ctypes.data_as(_fp),
                                          g["prim"].ctypes.data_as(C.POINTER(C.c_int32)), g["hits"].ctypes.data_as(_u32p)))
        out["sampled"] = g
    return out


class HipWavefrontRenderer:
    """The MI355X backend behind the reference's Renderer interface (src/core/renderer.h:8-16)."""

    def __init__(self, device: int = 0, max_depth: int = DEFAULT_MAX_DEPTH, seed: int = 0, rank: int = 0,
                 world_size: int = 1):
        self._ctx = C.c_void_p()
        L = capi.lib()
        rc = L.prt_create(device, C.byref(self._ctx))
        if rc:
            msg = L.prt_last_error(self._ctx).decode()
            L.prt_destroy(self._ctx)
            self._ctx = None
            raise PrtError(f"prt_create({device}) failed: {msg}")
        self.max_depth = int(max_depth)
        self.seed = int(seed)
        self.rank = int(rank)
        self.world_size = int(world_size)
        self.frame_index = 0
        self.film: Optional[Film] = None

    def __del__(self):
        if getattr(self, "_ctx", None):
            capi.lib().prt_destroy(self._ctx)
            self._ctx = None

    def _check(self, rc: int):
        if rc:
            raise PrtError(capi.lib().prt_last_error(self._ctx).decode())

    # ---- the reference interface -----------------------------------------------------------------
    def Init(self, film: Film, scene: Scene, camera: Camera):
        L = capi.lib()
        d = scene.desc()
        self._check(L.prt_set_scene(self._ctx, C.byref(d)))
        self._mesh_vertices = [m.n_vertices for m, _ in scene.meshes]  # (RefitDevice checks its tensors against them)
        if scene.textures or scene.material_texture:  # (prt_set_scene dropped the previous scene's binding)
            self.set_textures(scene)
        self._check(L.prt_set_film(self._ctx, film.width, film.height, self.rank, self.world_size))
        self.film = film
        film._renderer = self
        self.frame_index = 0
        self.SetCamera(camera)

    def SetCamera(self, camera: Camera):
        d = camera.desc()
        self._check(capi.lib().prt_set_camera(self._ctx, C.byref(d)))

    def ProgressiveRender(self, spp: int = 1):
        """Adds `spp` (default exactly one) sample per pixel to the film."""
        self._check(capi.lib().prt_render(self._ctx, spp, self.max_depth, self.seed, self.frame_index))
        self.frame_index += spp

    # ---- extensions ----------------------------------------------------------------------------------
    def render_async(self, spp: int = 1):
        self._check(capi.lib().prt_render_async(self._ctx, spp, self.max_depth, self.seed, self.frame_index))
        self.frame_index += spp

    def synchronize(self):
        self._check(capi.lib().prt_synchronize(self._ctx))

    def set_stream(self, hip_stream: int):
        self._check(capi.lib().prt_set_stream(self._ctx, C.c_void_p(hip_stream)))

    def set_samples_in_flight(self, n: int):
        self._check(capi.lib().prt_set_samples_in_flight(self._ctx, n))

    def set_sampling(self, jitter: int = 0, rr_depth: int = 0, clamp: float = 0.0) -> PrtSampling:
        """Optional sampling upgrades (include/prt.h PrtSampling); all zero = the reference CPU backend."""
        sp = PrtSampling(int(jitter), int(rr_depth), float(clamp))
        self._check(capi.lib().prt_set_sampling(self._ctx, C.byref(sp)))
        return sp

    def set_lens(self, fov_y: float = 0.0, aperture: float = 0.0, focus_distance: float = 0.0) -> capi.PrtLens:
        """Thin lens and field of view (include/prt.h PrtLens): fov_y in radians (0 = the reference's 1 rad), aperture = the
        lens radius in world units (0 = pinhole), focus_distance = distance along `front` of the plane in focus.  All zero =
        the reference's camera.  Stays with the renderer across SetCamera / Init."""
        ln = capi.PrtLens(float(fov_y), float(aperture), float(focus_distance))
        self._check(capi.lib().prt_set_lens(self._ctx, C.byref(ln)))
        return ln

    def get_lens(self) -> capi.PrtLens:
        ln = capi.PrtLens()
        self._check(capi.lib().prt_get_lens(self._ctx, C.byref(ln)))
        return ln

    def set_feature_trace(self, max_specular: int = 0, roughness_max: float = 0.1) -> capi.PrtFeatureTrace:
        """Guide features through specular chains (include/prt.h PrtFeatureTrace): follow up to max_specular (0..8) mirror
        or glass vertices of every centre ray; a Metal with roughness <= roughness_max is a mirror.  0 (the default) = first
        hit only.  While on, render_features() gains "guide", and denoise() / temporal_step(denoise=...) filter by it.  Stays
        with the renderer across SetCamera / Init."""
        ft = capi.PrtFeatureTrace(int(max_specular), float(roughness_max))
        self._check(capi.lib().prt_set_feature_trace(self._ctx, C.byref(ft)))
        return ft

    def get_feature_trace(self) -> capi.PrtFeatureTrace:
        ft = capi.PrtFeatureTrace()
        self._check(capi.lib().prt_get_feature_trace(self._ctx, C.byref(ft)))
        return ft

    def set_feature_sampling(self, samples: int = 0, seed=None, first_sample: int = 0) -> capi.PrtFeatureSampling:
        """Sampled guide features (include/prt.h PrtFeatureSampling): the features averaged over `samples` (0..64) of the
        render's own primary rays per pixel, those of samples first_sample .. first_sample + samples - 1 under `seed`
        (None: the renderer's own seed), through the lens and the jitter, each followed as set_feature_trace says.  0 (the
        default) = off.  While on, render_features() gains "sampled", and denoise() / temporal_step(denoise=...) filter by
        it.  Stays with the renderer across SetCamera / Init."""
        fs = capi.PrtFeatureSampling(int(samples), int(self.seed if seed is None else seed) & 0xFFFFFFFF, int(first_sample))
        self._check(capi.lib().prt_set_feature_sampling(self._ctx, C.byref(fs)))
        return fs

    def get_feature_sampling(self) -> capi.PrtFeatureSampling:
        fs = capi.PrtFeatureSampling()
        self._check(capi.lib().prt_get_feature_sampling(self._ctx, C.byref(fs)))
        return fs

    def set_film_statistics(self, on: bool = True):
        """Second moments of every pixel's luminance beside the film (include/prt.h "Film statistics and adaptive sampling").
        Switching them clears the film (and restarts the sample index)."""
        L = capi.lib()
        if bool(on) != bool(L.prt_get_film_statistics(self._ctx)):
            self.frame_index = 0
        self._check(L.prt_set_film_statistics(self._ctx, 1 if on else 0))

    def film_statistics(self) -> Tuple[np.ndarray, np.ndarray]:
        """(sum of y, sum of y^2) per pixel, film layout (H, W) float32; zero for pixels this rank does not own."""
        f = self.film
        a = np.zeros((f.height, f.width), np.float32)
        q = np.zeros((f.height, f.width), np.float32)
        self._check(capi.lib().prt_film_statistics_read(self._ctx, a.ctypes.data_as(_fp), q.ctypes.data_as(_fp)))
        return a, q

    def noise_map(self, noise_floor: float = 0.01) -> np.ndarray:
        """Relative standard error of every pixel's mean luminance (prt_film_noise_read), (H, W) float32; +inf below 2 samples."""
        f = self.film
        out = np.zeros((f.height, f.width), np.float32)
        self._check(capi.lib().prt_film_noise_read(self._ctx, float(noise_floor), out.ctypes.data_as(_fp)))
        return out

    def render_adaptive(self, threshold: float, min_spp: int = 8, step_spp: int = 8, max_spp: int = 64,
                        noise_floor: float = 0.01, first_sample: Optional[int] = None) -> "capi.PrtAdaptiveInfo":
        """Tile-adaptive sampling (prt_render_adaptive): min_spp samples everywhere, then step_spp at a time to the 8x8 tiles
        that still hold an unconverged pixel, up to max_spp.  Needs set_film_statistics(True).  first_sample defaults to the
        renderer's running index, which then moves on by max_spp (so a later call never reuses an index)."""
        cfg = capi.PrtAdaptive(int(min_spp), int(step_spp), int(max_spp), float(threshold), float(noise_floor))
        info = capi.PrtAdaptiveInfo()
        first = self.frame_index if first_sample is None else int(first_sample)
        self._check(capi.lib().prt_render_adaptive(self._ctx, C.byref(cfg), self.max_depth, self.seed, first, C.byref(info)))
        if first_sample is None:
            self.frame_index += int(max_spp)
        return info

    def set_film(self, film: Film):
        """The film alone (prt_set_film), for the entry points that need neither scene nor camera."""
        self._check(capi.lib().prt_set_film(self._ctx, film.width, film.height, self.rank, self.world_size))
        self.film = film
        film._renderer = self
        self.frame_index = 0

    def local_tile_count(self) -> int:
        """8x8 tiles of the film that this rank owns (global tile g belongs to rank g % world_size)."""
        f = self.film
        tiles = ((f.width + 7) // 8) * ((f.height + 7) // 8)
        return (tiles - self.rank + self.world_size - 1) // self.world_size if tiles > self.rank else 0

    def tile_select(self, n, sum_y, sum_y2, threshold: float, noise_floor: float = 0.01, prev=None):
        """prt_tile_select: the adaptive loop's selection stage on (H, W) float32 images of film weight and moments.  prev:
        local tile indices (None: every local tile).  Returns (list, count, pixels): list has len(prev) entries, the first
        `count` of them the active tiles in the order of prev, the others 0xFFFFFFFF."""
        f = self.film
        imgs = [np.ascontiguousarray(a, np.float32) for a in (n, sum_y, sum_y2)]
        if any(a.shape != (f.height, f.width) for a in imgs):
            raise ValueError("n, sum_y and sum_y2 must be [H, W]")
        if prev is None:
            n_prev, p_prev = self.local_tile_count(), None
        else:
            prev = np.ascontiguousarray(prev, np.uint32).reshape(-1)
            n_prev, p_prev = prev.size, prev.ctypes.data_as(_u32p)
        lst = np.zeros(max(n_prev, 1), np.uint32)
        counts = np.zeros(2, np.uint32)
        self._check(capi.lib().prt_tile_select(self._ctx, *[a.ctypes.data_as(_fp) for a in imgs], p_prev, n_prev, float(threshold),
                                               float(noise_floor), lst.ctypes.data_as(_u32p), counts.ctypes.data_as(_u32p)))
        return lst[:n_prev], int(counts[0]), int(counts[1])

    def render_features(self) -> dict:
        """First-hit feature images of the pixel-centre rays (prt_render_features): albedo, normal, position (H, W, 3)
        float32, depth (H, W) float32, prim (H, W) int32 (-1: a miss); the whole image whatever the partition.  They do not
        follow mirrors or glass and do not average over a lens or jitter.  While set_feature_trace(max_specular > 0) is on,
        "guide" holds the same five images at the end of each pixel's specular chain, plus bounces (H, W) uint32.  While
        set_feature_sampling(samples > 0) is on, "sampled" holds the five images averaged over that many of the render's own
        primary rays per pixel (lens and jitter included, each ray followed like the guide set's; the normal renormalised,
        prim that of the first sample that hit), plus hits (H, W) uint32: how many of the pixel's samples hit something."""
        f = self.film
        return _read_features(self._check, self._ctx, f.width, f.height)

    def denoise(self, return_variance: bool = False, **cfg):
        """The film through the edge-avoiding filter (prt_film_denoise; include/prt.h "The filter contract"): the (H, W, 3)
        float32 denoised mean, with return_variance also the (H, W) filtered variance.  Needs set_film_statistics(True) and a
        film that owns the whole image.  cfg: iterations, sigma_l, sigma_z, normal_power_log2, demodulate."""
        k = _denoise_config(**cfg)
        f = self.film
        out = np.zeros((f.height, f.width, 3), np.float32)
        var = np.zeros((f.height, f.width), np.float32) if return_variance else None
        self._check(capi.lib().prt_film_denoise(self._ctx, C.byref(k), out.ctypes.data_as(_fp),
                                                var.ctypes.data_as(_fp) if return_variance else None))
        return (out, var) if return_variance else out

    def denoise_arrays(self, mean, var, albedo, normal, position, prim, return_variance: bool = False, **cfg):
        """The filter on arrays of the caller's (prt_denoise / prt_denoise_device): mean, albedo, normal, position (H, W, 3)
        float32, var (H, W) float32, prim (H, W) int32.  numpy arrays: the host form, numpy results.  torch tensors on the
        renderer's device: the device form, tensors on that device, ordered after torch's current stream."""
        k = _denoise_config(**cfg)
        try:
            import torch
            is_t = any(isinstance(a, torch.Tensor) for a in (mean, var, albedo, normal, position, prim))
        except ImportError:
            is_t = False
        if is_t:
            H, W = (int(mean.shape[0]), int(mean.shape[1])) if isinstance(mean, torch.Tensor) and mean.dim() == 3 else (-1, -1)
            for name, t in (("mean", mean), ("albedo", albedo), ("normal", normal), ("position", position)):
                self._check_tensor(name, t, (H, W, 3))
            self._check_tensor("var", var, (H, W))
            if not isinstance(prim, torch.Tensor) or prim.dtype != torch.int32:
                raise ValueError("prim: expected a torch.int32 tensor")
            if prim.device != mean.device or tuple(prim.shape) != (H, W) or not prim.is_contiguous():
                raise ValueError(f"prim: expected a contiguous ({H}, {W}) tensor on {mean.device}")
            out = torch.empty((H, W, 3), dtype=torch.float32, device=mean.device)
            vout = torch.empty((H, W), dtype=torch.float32, device=mean.device) if return_variance else None
            self._on_context_stream(lambda: capi.lib().prt_denoise_device(
                self._ctx, C.byref(k), W, H, C.c_void_p(mean.data_ptr()), C.c_void_p(var.data_ptr()), C.c_void_p(albedo.data_ptr()),
                C.c_void_p(normal.data_ptr()), C.c_void_p(position.data_ptr()), C.c_void_p(prim.data_ptr()),
                C.c_void_p(out.data_ptr()), C.c_void_p(vout.data_ptr()) if return_variance else None))
            return (out, vout) if return_variance else out
        m = _f32(mean)
        if m.ndim != 3 or m.shape[2] != 3:
            raise ValueError(f"mean: expected an (H, W, 3) array, got {m.shape}")
        H, W = m.shape[:2]
        a, nr, ps, v = _f32(albedo), _f32(normal), _f32(position), _f32(var)
        pr = np.ascontiguousarray(prim, dtype=np.int32)
        for name, arr, shape in (("albedo", a, (H, W, 3)), ("normal", nr, (H, W, 3)), ("position", ps, (H, W, 3)),
                                 ("var", v, (H, W)), ("prim", pr, (H, W))):
            if arr.shape != shape:
                raise ValueError(f"{name}: shape {arr.shape}, expected {shape}")
        out = np.zeros((H, W, 3), np.float32)
        vout = np.zeros((H, W), np.float32) if return_variance else None
        self._check(capi.lib().prt_denoise(self._ctx, C.byref(k), W, H, m.ctypes.data_as(_fp), v.ctypes.data_as(_fp),
                                           a.ctypes.data_as(_fp), nr.ctypes.data_as(_fp), ps.ctypes.data_as(_fp),
                                           pr.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(_fp),
                                           vout.ctypes.data_as(_fp) if return_variance else None))
        return (out, vout) if return_variance else out

    def camera_basis(self) -> dict:
        """The camera as the kernels have it (prt_get_camera_basis): pos, right, up, front (3 float32 each), W, H, tan_fov_y."""
        k = capi.PrtCameraBasis()
        self._check(capi.lib().prt_get_camera_basis(self._ctx, C.byref(k)))
        return _basis_dict(k)

    def temporal_step(self, return_variance: bool = False, return_history: bool = False, denoise=None, **cfg):
        """One frame step of the temporal reprojection on the film (prt_film_temporal; include/prt.h "Temporal reprojection"):
        the (H, W, 3) float32 frame blended with the history the renderer keeps, through the spatial filter if denoise is a
        dict of its settings ({} = the defaults; None = no filter).  With return_variance / return_history also the (H, W)
        variance / history length.  The film is not touched: clear it between frames.  cfg: max_history, normal_min,
        plane_tol."""
        k = _temporal_config(**cfg)
        dn = None if denoise is None else _denoise_config(**denoise)
        f = self.film
        out = np.zeros((f.height, f.width, 3), np.float32)
        var = np.zeros((f.height, f.width), np.float32) if return_variance else None
        hist = np.zeros((f.height, f.width), np.float32) if return_history else None
        self._check(capi.lib().prt_film_temporal(self._ctx, C.byref(k), C.byref(dn) if dn is not None else None, out.ctypes.data_as(_fp),
                                                 var.ctypes.data_as(_fp) if return_variance else None,
                                                 hist.ctypes.data_as(_fp) if return_history else None))
        res = (out,) + ((var,) if return_variance else ()) + ((hist,) if return_history else ())
        return res if len(res) > 1 else out

    def temporal_reset(self):
        self._check(capi.lib().prt_temporal_reset(self._ctx))

    def temporal_info(self) -> "capi.PrtTemporalInfo":
        info = capi.PrtTemporalInfo()
        self._check(capi.lib().prt_temporal_info(self._ctx, C.byref(info)))
        return info

    def temporal_prev_surface(self, position, normal, prim, prev_instances=()):
        """prt_temporal_prev_surface: where the points (n, 3) with normals (n, 3) and prims (n,) of the current scene were
        when its placed copies had the transforms of prev_instances (PrtInstance records; empty: nothing moved)."""
        p, nr = _f32(position).reshape(-1, 3), _f32(normal).reshape(-1, 3)
        pr = np.ascontiguousarray(prim, dtype=np.int32).reshape(-1)
        if not (len(p) == len(nr) == len(pr)):
            raise ValueError("position, normal and prim must have one entry per point")
        insts = (PrtInstance * max(1, len(prev_instances)))(*prev_instances)
        po, no = np.zeros_like(p), np.zeros_like(nr)
        self._check(capi.lib().prt_temporal_prev_surface(self._ctx, len(p), p.ctypes.data_as(_fp), nr.ctypes.data_as(_fp),
                                                         pr.ctypes.data_as(C.POINTER(C.c_int32)), insts, len(prev_instances),
                                                         po.ctypes.data_as(_fp), no.ctypes.data_as(_fp)))
        return po, no

    def temporal_arrays(self, basis, c, n, A, Q, prim, Pprev, Nprev, history=None, return_variance: bool = True, return_status: bool = True,
                        **cfg):
        """The reprojection on arrays of the caller's (prt_temporal_reproject / _device).  basis: camera_basis()'s dict of the
        PREVIOUS frame; c, Pprev, Nprev (H, W, 3) float32; n, A, Q (H, W) float32; prim (H, W) int32; history: None or a dict
        of hc, hP, hN (H, W, 3), hn, h1, h2 (H, W) and hprim (H, W) int32.  numpy arrays: the host form, numpy results.
        torch tensors on the renderer's device: the device form, ordered after torch's current stream.  Returns a dict of c,
        n, m1, m2 and, if asked, var and status (uint8)."""
        k = _temporal_config(**cfg)
        K = _basis_struct(basis)
        h = history or {}
        names3, names1 = ("c", "Pprev", "Nprev"), ("n", "A", "Q")
        cur = dict(c=c, n=n, A=A, Q=Q, prim=prim, Pprev=Pprev, Nprev=Nprev)
        hist_names = ("hc", "hn", "h1", "h2", "hP", "hN", "hprim")
        if history is not None and set(h) != set(hist_names):
            raise ValueError(f"history: expected the keys {hist_names}")
        try:
            import torch
            is_t = any(isinstance(a, torch.Tensor) for a in list(cur.values()) + list(h.values()))
        except ImportError:
            is_t = False
        L = capi.lib()
        if is_t:
            H, W = (int(c.shape[0]), int(c.shape[1])) if isinstance(c, torch.Tensor) and c.dim() == 3 else (-1, -1)

            def chk(name, t):
                if name in ("prim", "hprim"):
                    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
                        raise ValueError(f"{name}: expected a torch.int32 tensor")
                    if t.device != c.device or tuple(t.shape) != (H, W) or not t.is_contiguous():
                        raise ValueError(f"{name}: expected a contiguous ({H}, {W}) tensor on {c.device}")
                else:
                    self._check_tensor(name, t, (H, W, 3) if name in names3 + ("hc", "hP", "hN") else (H, W))
            for name, t in list(cur.items()) + list(h.items()):
                chk(name, t)
            o = dict(c=torch.empty((H, W, 3), dtype=torch.float32, device=c.device))
            for name in ("n", "m1", "m2") + (("var",) if return_variance else ()):
                o[name] = torch.empty((H, W), dtype=torch.float32, device=c.device)
            if return_status:
                o["status"] = torch.empty((H, W), dtype=torch.uint8, device=c.device)
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            self._on_context_stream(lambda: L.prt_temporal_reproject_device(
                self._ctx, C.byref(k), W, H, C.byref(K), *[ptr(cur[x]) for x in ("c", "n", "A", "Q", "prim", "Pprev", "Nprev")],
                *[ptr(h.get(x)) for x in hist_names], ptr(o["c"]), ptr(o["n"]), ptr(o["m1"]), ptr(o["m2"]), ptr(o.get("var")),
                ptr(o.get("status"))))
            return o
        a = {x: _f32(cur[x]) for x in names3 + names1}
        a["prim"] = np.ascontiguousarray(prim, dtype=np.int32)
        if a["c"].ndim != 3 or a["c"].shape[2] != 3:
            raise ValueError(f"c: expected an (H, W, 3) array, got {a['c'].shape}")
        H, W = a["c"].shape[:2]
        if history is not None:
            for x in hist_names:
                a[x] = np.ascontiguousarray(h[x], dtype=np.int32) if x == "hprim" else _f32(h[x])
        for name, arr in a.items():
            shape = (H, W, 3) if name in names3 + ("hc", "hP", "hN") else (H, W)
            if arr.shape != shape:
                raise ValueError(f"{name}: shape {arr.shape}, expected {shape}")
        o = dict(c=np.zeros((H, W, 3), np.float32), n=np.zeros((H, W), np.float32), m1=np.zeros((H, W), np.float32),
                 m2=np.zeros((H, W), np.float32))
        if return_variance:
            o["var"] = np.zeros((H, W), np.float32)
        if return_status:
            o["status"] = np.zeros((H, W), np.uint8)
        ip = C.POINTER(C.c_int32)
        ptr = lambda x, t=_fp: a[x].ctypes.data_as(t) if x in a else None
        self._check(L.prt_temporal_reproject(
            self._ctx, C.byref(k), W, H, C.byref(K), ptr("c"), ptr("n"), ptr("A"), ptr("Q"), ptr("prim", ip), ptr("Pprev"), ptr("Nprev"),
            ptr("hc"), ptr("hn"), ptr("h1"), ptr("h2"), ptr("hP"), ptr("hN"), ptr("hprim", ip), o["c"].ctypes.data_as(_fp),
            o["n"].ctypes.data_as(_fp), o["m1"].ctypes.data_as(_fp), o["m2"].ctypes.data_as(_fp),
            o["var"].ctypes.data_as(_fp) if return_variance else None,
            o["status"].ctypes.data_as(C.POINTER(C.c_uint8)) if return_status else None))
        return o

    def set_lighting(self, mode) -> int:
        """Light sampling toward the analytic emitters (include/prt.h PrtLighting): "off" | "mis" | "nee" or 0 | 1 | 2."""
        m = capi.LIGHTING_MODES[mode] if isinstance(mode, str) else int(mode)
        self._check(capi.lib().prt_set_lighting(self._ctx, C.byref(capi.PrtLighting(m))))
        return m

    def set_light_sources(self, sources) -> int:
        """Which emitters the light set holds (include/prt.h "Triangle lights"): "analytic" (default) | "all" (analytic
        emitters + the triangles of emissive meshes and placed copies), or a PRT_LIGHT_SOURCES_* mask."""
        m = capi.LIGHT_SOURCES[sources] if isinstance(sources, str) else int(sources)
        self._check(capi.lib().prt_set_light_sources(self._ctx, m))
        return m

    def set_light_selection(self, selection="power", max_clusters: int = 32) -> int:
        """How a light is picked (include/prt.h "Clustered light selection"): "power" (default) | "clustered" (a spatial
        cluster by power / distance^2 to its box, then a light inside it), or a PRT_LIGHT_SELECTION_* value.  Takes
        effect only with set_light_sources("all")."""
        m = capi.LIGHT_SELECTIONS[selection] if isinstance(selection, str) else int(selection)
        self._check(capi.lib().prt_set_light_selection(self._ctx, C.byref(capi.PrtLightSelection(m, int(max_clusters)))))
        return m

    def light_cluster_info(self) -> "capi.PrtLightClusterInfo":
        s = capi.PrtLightClusterInfo()
        self._check(capi.lib().prt_light_cluster_info(self._ctx, C.byref(s)))
        return s

    def light_clusters(self) -> dict:
        """The clusters of the current scene: lo, hi [K, 3], r2, phi [K] float32, power_width [K] uint64 (they sum to
        2^32), n_members [K].  Host-only contexts too."""
        n = C.c_uint32(0)
        L = capi.lib()
        self._check(L.prt_light_clusters(self._ctx, 0, C.byref(n), None, None, None, None, None, None))
        K = n.value
        o = dict(lo=np.zeros((K, 3), np.float32), hi=np.zeros((K, 3), np.float32), r2=np.zeros(K, np.float32),
                 phi=np.zeros(K, np.float32), power_width=np.zeros(K, np.uint64), n_members=np.zeros(K, np.uint32))
        self._check(L.prt_light_clusters(self._ctx, K, C.byref(n), o["lo"].ctypes.data_as(_fp), o["hi"].ctypes.data_as(_fp),
                                         o["r2"].ctypes.data_as(_fp), o["phi"].ctypes.data_as(_fp),
                                         o["power_width"].ctypes.data_as(C.POINTER(C.c_uint64)), o["n_members"].ctypes.data_as(_u32p)))
        return o

    def light_cluster_members(self) -> Tuple[np.ndarray, np.ndarray]:
        """Per light of the light set (light_info's order): (cluster [n] uint32, inner width U_j - U_{j-1} [n] uint64)."""
        n = C.c_uint32(0)
        L = capi.lib()
        self._check(L.prt_light_cluster_members(self._ctx, 0, C.byref(n), None, None))
        cl, w = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint64)
        self._check(L.prt_light_cluster_members(self._ctx, n.value, C.byref(n), cl.ctypes.data_as(_u32p),
                                                w.ctypes.data_as(C.POINTER(C.c_uint64))))
        return cl, w

    def light_cluster_pmf(self, x) -> np.ndarray:
        """prt_light_cluster_pmf: the device's thresholds M_c [n, K] uint32 of the cluster choice at the points x [n, 3];
        P_c = (M_c - M_{c-1}) / 2^24."""
        p = _f32(x).reshape(-1, 3)
        K = self.light_cluster_info().n_clusters
        M = np.zeros((p.shape[0], K), np.uint32)
        self._check(capi.lib().prt_light_cluster_pmf(self._ctx, p.shape[0], p.ctypes.data_as(_fp), M.ctypes.data_as(_u32p)))
        return M

    def set_environment(self, rgb, light_share: float = 0.5):
        """Environment light (include/prt.h "Environment light"): rgb [H, W, 3] lat-long radiance, row 0 = the +Y pole; None
        = back to the scene's constant sky.  light_share = the probability that a light sample goes to the image."""
        self._check(_set_environment(capi.lib().prt_set_environment, self._ctx, rgb, light_share))

    def environment_info(self) -> "capi.PrtEnvironmentInfo":
        s = capi.PrtEnvironmentInfo()
        self._check(capi.lib().prt_environment_info(self._ctx, C.byref(s)))
        return s

    def set_textures(self, scene: Optional["Scene"]):
        """Binds `scene`'s textures (Scene.AddTexture / SetMaterialTexture, the meshes' UVs) to the current scene, which must
        be the one `scene` describes; a scene without textures, or None, removes the binding.  Init does this itself;
        Refit and UpdateInstances keep the binding (include/prt.h "Image textures")."""
        ts = scene.texture_set() if scene is not None else None
        self._check(capi.lib().prt_set_textures(self._ctx, None if ts is None else C.byref(ts)))

    def texture_info(self) -> "capi.PrtTextureInfo":
        s = capi.PrtTextureInfo()
        self._check(capi.lib().prt_texture_info(self._ctx, C.byref(s)))
        return s

    def texture_eval(self, texture, uv) -> np.ndarray:
        """prt_texture_eval: the render's own lookup, rgb [n, 3] for uv [n, 2] in `texture` (one index, or one per uv)."""
        u = _f32(uv).reshape(-1, 2)
        n = u.shape[0]
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(texture, np.uint32), (n,)))
        rgb = np.zeros((n, 3), np.float32)
        self._check(capi.lib().prt_texture_eval(self._ctx, n, t.ctypes.data_as(_u32p), u.ctypes.data_as(_fp), rgb.ctypes.data_as(_fp)))
        return rgb

    def hit_uv(self, origins, dirs) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """prt_hit_uv: (hits as closest_hit returns them, uv [n, 2], albedo [n, 3]) through the shade kernels' device code."""
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        n = o.shape[0]
        hits = np.zeros(n, dtype=capi.HIT_DTYPE)
        uv, alb = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32)
        self._check(capi.lib().prt_hit_uv(self._ctx, n, o.ctypes.data_as(_fp), d.ctypes.data_as(_fp),
                                          hits.ctypes.data_as(C.POINTER(PrtHit)), uv.ctypes.data_as(_fp), alb.ctypes.data_as(_fp)))
        return hits, uv, alb

    def environment_intervals(self) -> Tuple[np.ndarray, np.ndarray]:
        """The exact interval widths (row [H] uint64, column [H, W] uint64); texel pmf = row x column / 2^64.  Host-only
        contexts too."""
        i = self.environment_info()
        row, col = np.zeros(i.height, np.uint64), np.zeros((i.height, i.width), np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._check(capi.lib().prt_environment_intervals(self._ctx, row.ctypes.data_as(u64p), col.ctypes.data_as(u64p)))
        return row, col

    def environment_eval(self, dirs) -> dict:
        """prt_environment_eval: the render's own lookup per unit direction: rgb [n, 3], texel [n] (i * W + j), pdf_w [n]."""
        d = _f32(dirs).reshape(-1, 3)
        n = d.shape[0]
        rgb, texel, pdf = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
        self._check(capi.lib().prt_environment_eval(self._ctx, n, d.ctypes.data_as(_fp), rgb.ctypes.data_as(_fp),
                                                    texel.ctypes.data_as(_u32p), pdf.ctypes.data_as(_fp)))
        return {"rgb": rgb, "texel": texel, "pdf_w": pdf}

    def light_intervals(self) -> np.ndarray:
        """With "all": the integer width T_l - T_{l-1} of every light's interval ([n] uint64); pmf = width / 2^32 exactly."""
        n = C.c_uint32(0)
        self._check(capi.lib().prt_light_intervals(self._ctx, 0, C.byref(n), None))
        w = np.zeros(n.value, np.uint64)
        self._check(capi.lib().prt_light_intervals(self._ctx, n.value, C.byref(n), w.ctypes.data_as(C.POINTER(C.c_uint64))))
        return w

    def light_info(self) -> Tuple[np.ndarray, np.ndarray]:
        """The light set of the current scene: (primitive index [n] uint32, pmf [n] float32).  Host-only contexts too."""
        n = C.c_uint32(0)
        self._check(capi.lib().prt_light_info(self._ctx, 0, C.byref(n), None, None))
        prim = np.zeros(n.value, np.uint32)
        pmf = np.zeros(n.value, np.float32)
        self._check(capi.lib().prt_light_info(self._ctx, n.value, C.byref(n), prim.ctypes.data_as(_u32p), pmf.ctypes.data_as(_fp)))
        return prim, pmf

    def light_stats(self) -> "capi.PrtLightStats":
        s = capi.PrtLightStats()
        self._check(capi.lib().prt_get_light_stats(self._ctx, C.byref(s)))
        return s

    def sample_light(self, in_dirs, hits: np.ndarray, keys) -> dict:
        """prt_sample_light: one light sample per (hit, key) through the render's device code."""
        d = _f32(in_dirs).reshape(-1, 3)
        n = d.shape[0]
        hits = np.ascontiguousarray(hits)
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        sd, contrib = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        tmax, pl, pb, wl, wb = (np.zeros(n, np.float32) for _ in range(5))
        light = np.zeros(n, np.uint32)
        self._check(capi.lib().prt_sample_light(self._ctx, n, d.ctypes.data_as(_fp), hits.ctypes.data_as(C.POINTER(PrtHit)),
                                                k.ctypes.data_as(_u32p), sd.ctypes.data_as(_fp), tmax.ctypes.data_as(_fp),
                                                light.ctypes.data_as(_u32p), contrib.ctypes.data_as(_fp),
                                                pl.ctypes.data_as(_fp), pb.ctypes.data_as(_fp), wl.ctypes.data_as(_fp),
                                                wb.ctypes.data_as(_fp)))
        return {"dir": sd, "tmax": tmax, "light": light, "contrib": contrib, "pdf_light": pl, "pdf_bsdf": pb, "w_light": wl,
                "w_bsdf": wb}

    def set_variant(self, v: int):
        self._check(capi.lib().prt_set_variant(self._ctx, v))

    def set_param(self, name: str, value: int):
        self._check(capi.lib().prt_set_param(self._ctx, name.encode(), int(value)))

    def download(self) -> Film:
        f = self.film
        self._check(capi.lib().prt_film_read(self._ctx, f.accum.ctypes.data_as(_fp), f.weights.ctypes.data_as(_fp)))
        return f

    def UpdateDisplay(self, exposure: float = 1.0, gamma: float = 2.2) -> np.ndarray:
        """Film::UpdateDisplayGPU (src/core/film.cu:123-132): RGBA8, row 0 = top."""
        f = self.film
        self._check(capi.lib().prt_film_display(self._ctx, exposure, gamma,
                                                f.display.ctypes.data_as(C.POINTER(C.c_uint8))))
        return f.display

    def film_local(self) -> Tuple[int, int]:
        p = C.c_void_p()
        n = C.c_uint64()
        self._check(capi.lib().prt_film_local(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def film_resolve(self, d_gathered: int, d_rgb: int, d_weight: int, stream: int = 0):
        """stream: a raw HIP stream to launch on (0 = the renderer's own stream)."""
        self._check(capi.lib().prt_film_resolve_on(self._ctx, C.c_void_p(stream), C.c_void_p(d_gathered), self.world_size,
                                                   C.c_void_p(d_rgb), C.c_void_p(d_weight)))

    def film_tonemap(self, d_rgb: int, d_weight: int, d_rgba8: int, exposure: float = 1.0, gamma: float = 2.2):
        self._check(capi.lib().prt_film_tonemap(self._ctx, C.c_void_p(d_rgb), C.c_void_p(d_weight), exposure, gamma,
                                                C.c_void_p(d_rgba8)))

    def camera_rays(self, px, py):
        px, py = _f32(px).ravel(), _f32(py).ravel()
        n = px.size
        o = np.empty((n, 3), np.float32)
        d = np.empty((n, 3), np.float32)
        self._check(capi.lib().prt_camera_rays(self._ctx, n, px.ctypes.data_as(_fp), py.ctypes.data_as(_fp),
                                               o.ctypes.data_as(_fp), d.ctypes.data_as(_fp)))
        return o, d

    def camera_rays_lens(self, px, py, keys):
        """The render's primary rays under the current lens for pixel-space points (px, py) and RNG states `keys` (the
        path's state before the lens draws).  Returns (origins, dirs, keys after): two draws further while aperture > 0."""
        px, py = _f32(px).ravel(), _f32(py).ravel()
        k = np.array(keys, dtype=np.uint32).ravel()  # a copy: advanced in place
        n = px.size
        if py.size != n or k.size != n:
            raise ValueError("px, py and keys must have the same number of elements")
        o = np.empty((n, 3), np.float32)
        d = np.empty((n, 3), np.float32)
        self._check(capi.lib().prt_camera_rays_lens(self._ctx, n, px.ctypes.data_as(_fp), py.ctypes.data_as(_fp),
                                                    k.ctypes.data_as(C.POINTER(C.c_uint32)), o.ctypes.data_as(_fp),
                                                    d.ctypes.data_as(_fp)))
        return o, d, k

    def closest_hit(self, origins, dirs) -> np.ndarray:
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        hits = np.zeros(o.shape[0], dtype=capi.HIT_DTYPE)
        self._check(capi.lib().prt_closest_hit(self._ctx, o.shape[0], o.ctypes.data_as(_fp), d.ctypes.data_as(_fp),
                                               hits.ctypes.data_as(C.POINTER(PrtHit))))
        return hits

    # ---- ray queries on device-resident data (torch tensors) and occlusion -------------------------------------
    def _torch_device(self):
        import torch
        dev = capi.lib().prt_get_device(self._ctx)
        if dev < 0:
            raise PrtError("no HIP device bound to this context: device tensors need one")
        return torch.device("cuda", dev)

    def _check_tensor(self, name: str, t, shape):
        import torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a torch tensor on {self._torch_device()}, got {type(t).__name__}")
        if t.device != self._torch_device():
            raise ValueError(f"{name}: tensor is on {t.device}, the renderer's device is {self._torch_device()}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: dtype {t.dtype}, expected torch.float32")
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {shape}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: tensor is not contiguous")

    def _on_context_stream(self, fn):
        """Runs fn() (which enqueues on the context's stream) ordered after torch's current stream, and makes that
        stream wait for what fn enqueued: the results are then safe to use in ordinary torch code."""
        import torch
        dev = self._torch_device()
        h = C.c_void_p()
        self._check(capi.lib().prt_get_stream(self._ctx, C.byref(h)))
        cur = torch.cuda.current_stream(dev)
        if (h.value or 0) == cur.cuda_stream:
            self._check(fn())
            return
        ext = torch.cuda.ExternalStream(h.value, device=dev)
        before = torch.cuda.Event()
        before.record(cur)
        ext.wait_event(before)
        self._check(fn())
        after = torch.cuda.Event()
        after.record(ext)
        cur.wait_event(after)

    def closest_hit_device(self, origins, dirs):
        """prt_closest_hit_device on torch tensors ([n, 3] float32 on the renderer's device): the raw 40-byte PrtHit
        records as an [n, 10] int32 tensor on that device (hits_to_numpy views them as capi.HIT_DTYPE)."""
        import torch
        n = int(origins.shape[0]) if getattr(origins, "dim", lambda: 0)() == 2 else -1
        self._check_tensor("origins", origins, (n, 3))
        self._check_tensor("dirs", dirs, (n, 3))
        out = torch.empty((n, 10), dtype=torch.int32, device=origins.device)
        if n:
            self._on_context_stream(lambda: capi.lib().prt_closest_hit_device(
                self._ctx, n, C.c_void_p(origins.data_ptr()), C.c_void_p(dirs.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def occluded(self, origins, dirs, tmax):
        """Occlusion (shadow-ray) query: True where something blocks the ray before distance tmax, i.e. where the
        closest hit lies at d2 < fl32(tmax^2) (prt_occluded).  numpy inputs: the host form, a bool ndarray.  torch
        tensors on the renderer's device: the device form, a torch.bool tensor on that device, ordered after torch's
        current stream.  tmax: one value per ray, or a scalar for all of them."""
        try:
            import torch
            is_t = isinstance(origins, torch.Tensor) or isinstance(dirs, torch.Tensor)
        except ImportError:
            is_t = False
        if is_t:
            n = int(origins.shape[0]) if isinstance(origins, torch.Tensor) and origins.dim() == 2 else -1
            self._check_tensor("origins", origins, (n, 3))
            self._check_tensor("dirs", dirs, (n, 3))
            if isinstance(tmax, torch.Tensor):
                if tmax.dim() == 0:
                    tmax = tmax.to(device=origins.device).expand(n).contiguous()
                self._check_tensor("tmax", tmax, (n,))
            elif np.ndim(tmax) == 0:
                tmax = torch.full((n,), float(tmax), dtype=torch.float32, device=origins.device)
            else:
                raise ValueError("tmax: expected a scalar or a torch tensor with the rays")
            out = torch.empty(n, dtype=torch.uint8, device=origins.device)
            if n:
                self._on_context_stream(lambda: capi.lib().prt_occluded_device(
                    self._ctx, n, C.c_void_p(origins.data_ptr()), C.c_void_p(dirs.data_ptr()), C.c_void_p(tmax.data_ptr()),
                    C.c_void_p(out.data_ptr())))
            return out.bool()
        o, d = _f32(origins), _f32(dirs)
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError(f"origins / dirs: expected two [n, 3] arrays, got {o.shape} and {d.shape}")
        n = o.shape[0]
        t = np.asarray(tmax, np.float32)
        if t.ndim == 0:
            t = np.full(n, t, np.float32)
        elif t.shape != (n,):
            raise ValueError(f"tmax: shape {t.shape}, expected a scalar or ({n},)")
        t = np.ascontiguousarray(t)
        out = np.zeros(n, np.uint8)
        self._check(capi.lib().prt_occluded(self._ctx, n, o.ctypes.data_as(_fp), d.ctypes.data_as(_fp),
                                            t.ctypes.data_as(_fp), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.astype(bool)

    def scatter(self, in_dirs, hits: np.ndarray, rng_state):
        d = _f32(in_dirs).reshape(-1, 3)
        n = d.shape[0]
        hits = np.ascontiguousarray(hits)
        rng = np.ascontiguousarray(rng_state, dtype=np.uint32).copy()
        sc = np.zeros(n, np.uint32)
        att, em, oo, od = (np.zeros((n, 3), np.float32) for _ in range(4))
        self._check(capi.lib().prt_scatter(self._ctx, n, d.ctypes.data_as(_fp), hits.ctypes.data_as(C.POINTER(PrtHit)),
                                           rng.ctypes.data_as(_u32p), sc.ctypes.data_as(_u32p),
                                           att.ctypes.data_as(_fp), em.ctypes.data_as(_fp), oo.ctypes.data_as(_fp),
                                           od.ctypes.data_as(_fp)))
        return sc.astype(bool), att, em, oo, od, rng

    def radiance(self, o, d, rng_state=None, samples: int = 1, seed=None, first_sample: int = 0, max_depth=None,
                 return_info: bool = False, lighting: bool = False, pb=None):
        """The radiance arriving along n caller-supplied rays (prt_radiance, include/prt.h "Radiance query"): whole paths
        of up to max_depth segments (default: the renderer's) on the device, `samples` per ray.  o, d: [n, 3] float32,
        numpy arrays (the host form) or torch tensors on the renderer's device (the device form, ordered after torch's
        current stream).  rng_state [n] (uint32; torch: int32 or uint32 bits) gives every path its starting state and needs
        samples == 1; without it sample s of ray i starts from path_seed(i, first_sample + s, seed), seed = the renderer's
        unless given.  Returns the mean [n, 3] = sum / samples in fp32; with return_info also {"sum": the fp32 sum the
        library returns, "segments": [n] segments walked, "rng_state": the final states, or None}.
        lighting=True: the light-sampled query (prt_radiance_lit): the estimator a render would use now (set_lighting,
        set_light_sources, set_light_selection, the environment's light share); the same paths, less noise under small
        emitters.  With return_info the info then also has "shadow_rays" and "shadow_occluded" of this call.
        pb [n] float32 (numpy or torch, as o / d; needs lighting=True): the rays were scattered by a Lambertian vertex of the
        caller's with pdf pb[i] = max(0, n.d) / pi, so what the first segment meets is weighted as after a vertex of the
        path's own (prt_radiance_lit_pb): the continuation of a first vertex shaded outside the library."""
        if pb is not None and not lighting:
            raise ValueError("pb: the scatter pdf of the caller's segment weights light-sampled paths only: pass lighting=True")
        lit = capi.PrtRadianceLitInfo() if (lighting and return_info) else None
        q = capi.PrtRadianceQuery(int(self.max_depth if max_depth is None else max_depth), int(samples),
                                  int(self.seed if seed is None else seed) & 0xFFFFFFFF, int(first_sample) & 0xFFFFFFFF)
        try:
            import torch
            is_t = isinstance(o, torch.Tensor) or isinstance(d, torch.Tensor)
        except ImportError:
            is_t = False
        if is_t:
            n = int(o.shape[0]) if isinstance(o, torch.Tensor) and o.dim() == 2 else -1
            self._check_tensor("o", o, (n, 3))
            self._check_tensor("d", d, (n, 3))
            rng = None
            if rng_state is not None:
                if not isinstance(rng_state, torch.Tensor) or rng_state.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or \
                        tuple(rng_state.shape) != (n,) or rng_state.device != o.device:
                    raise ValueError(f"rng_state: expected an int32 / uint32 tensor of shape ({n},) on {o.device}")
                rng = rng_state.contiguous().clone()
            total = torch.zeros((n, 3), dtype=torch.float32, device=o.device)
            seg = torch.zeros(n, dtype=torch.int32, device=o.device)
            # (n == 0 still goes through the library: it refuses a bad query whatever the count)
            args = (self._ctx, C.byref(q), n, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                    C.c_void_p(rng.data_ptr() if rng is not None else None), C.c_void_p(total.data_ptr()), C.c_void_p(seg.data_ptr()))
            if pb is not None:
                if not isinstance(pb, torch.Tensor):
                    raise ValueError("pb: expected a torch tensor with the rays")
                self._check_tensor("pb", pb, (n,))
                self._on_context_stream(lambda: capi.lib().prt_radiance_lit_pb_device(
                    *args[:6], C.c_void_p(pb.data_ptr()), *args[6:], C.byref(lit) if lit is not None else None))
            elif lighting:
                self._on_context_stream(lambda: capi.lib().prt_radiance_lit_device(*args, C.byref(lit) if lit is not None else None))
            else:
                self._on_context_stream(lambda: capi.lib().prt_radiance_device(*args))
            # (a tensor divisor: torch turns a division by a Python number into a multiplication by its reciprocal)
            mean = total / torch.full((1, 1), float(q.samples), dtype=torch.float32, device=o.device)
        else:
            o, d = _f32(o), _f32(d)
            if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
                raise ValueError(f"o / d: expected two [n, 3] arrays, got {o.shape} and {d.shape}")
            n = o.shape[0]
            rng = None
            if rng_state is not None:
                rng = np.array(rng_state, dtype=np.uint32).ravel()  # a copy: advanced in place
                if rng.size != n:
                    raise ValueError(f"rng_state: {rng.size} states for {n} rays")
            total = np.zeros((n, 3), np.float32)
            seg = np.zeros(n, np.uint32)
            args = (self._ctx, C.byref(q), n, o.ctypes.data_as(_fp), d.ctypes.data_as(_fp),
                    rng.ctypes.data_as(_u32p) if rng is not None else None, total.ctypes.data_as(_fp), seg.ctypes.data_as(_u32p))
            if pb is not None:
                pbv = np.ascontiguousarray(_f32(pb).ravel())
                if pbv.size != n:
                    raise ValueError(f"pb: {pbv.size} values for {n} rays")
                self._check(capi.lib().prt_radiance_lit_pb(*args[:6], pbv.ctypes.data_as(_fp), *args[6:],
                                                           C.byref(lit) if lit is not None else None))
            elif lighting:
                self._check(capi.lib().prt_radiance_lit(*args, C.byref(lit) if lit is not None else None))
            else:
                self._check(capi.lib().prt_radiance(*args))
            mean = total / np.float32(q.samples)
        if return_info:
            info = {"sum": total, "segments": seg, "rng_state": rng}
            if lit is not None:
                info["shadow_rays"] = int(lit.shadow_rays)
                info["shadow_occluded"] = int(lit.shadow_occluded)
            return mean, info
        return mean

    def render_probe(self, position, H: int, W: int, samples: int = 1, seed=None, first_sample: int = 0, max_depth=None,
                     lighting: bool = False) -> np.ndarray:
        """A lat-long radiance probe at `position`: [H, W, 3] float32, the mean radiance along probe_directions(H, W),
        texel index = ray index.  The layout is set_environment's, so a probe of one scene can light another.
        lighting: radiance()'s."""
        d = probe_directions(H, W).reshape(-1, 3)
        o = np.broadcast_to(_f32(position).reshape(1, 3), d.shape)
        return self.radiance(o, d, samples=samples, seed=seed, first_sample=first_sample, max_depth=max_depth,
                             lighting=lighting).reshape(H, W, 3)

    # ---- SH probes (include/prt.h "SH probes") --------------------------------------------------------------------
    def probe_sh_rays(self, positions, sample: int = 0, seed=None) -> dict:
        """The ray of sample `sample` of every probe (prt_probe_sh_rays): {"o", "d" [P, 3], "rng_state" [P] uint32}.
        radiance(o, d, rng_state=...) follows the paths probe_sh follows."""
        x = np.ascontiguousarray(_f32(positions).reshape(-1, 3))
        P = x.shape[0]
        o, d = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32)
        rng = np.zeros(P, np.uint32)
        self._check(capi.lib().prt_probe_sh_rays(self._ctx, P, x.ctypes.data_as(_fp), int(self.seed if seed is None else seed) & 0xFFFFFFFF,
                                                 int(sample) & 0xFFFFFFFF, o.ctypes.data_as(_fp), d.ctypes.data_as(_fp), rng.ctypes.data_as(_u32p)))
        return {"o": o, "d": d, "rng_state": rng}

    def probe_sh(self, positions, order: int = 2, samples: int = 64, seed=None, first_sample: int = 0, max_depth=None,
                 lighting: bool = False, out: str = "numpy", return_info: bool = False):
        """Light probes (prt_probe_sh): the radiance arriving at P points as real spherical-harmonic coefficients
        [P, (order + 1)^2, 3]: `samples` uniformly distributed directions per point, followed by the radiance query
        (lighting: radiance()'s) and projected on the device in a fixed order.  The value is
        sum * float32(4 pi) / float32(samples); sh_irradiance(coeffs, n) turns it into the irradiance on a surface of normal
        n.  positions [P, 3]: a numpy array (the host form) or a torch tensor on the renderer's device (the device form,
        ordered after torch's current stream; positions are taken as they are).  out = "torch": a tensor on the renderer's
        device through the device form.  return_info: also {"sum": the raw fp32 sums, "info": the counts of the call}."""
        if out not in ("numpy", "torch"):
            raise ValueError(f"out: {out!r}, expected 'numpy' or 'torch'")
        if int(order) < 0 or int(order) > 0xFFFFFFFF:
            raise ValueError(f"order: {order}")
        opt = capi.PrtProbeShOptions(int(order), int(bool(lighting)), (C.c_uint32 * 2)(0, 0))
        q = capi.PrtRadianceQuery(int(self.max_depth if max_depth is None else max_depth), int(samples),
                                  int(self.seed if seed is None else seed) & 0xFFFFFFFF, int(first_sample) & 0xFFFFFFFF)
        K = (int(order) + 1) ** 2 if int(order) <= capi.SH_MAX_ORDER else 1      # (the library refuses the order; the array is a placeholder)
        info = capi.PrtProbeShInfo()
        try:
            import torch
            is_t = isinstance(positions, torch.Tensor)
        except ImportError:
            is_t = False
        if is_t or out == "torch":
            import torch
            dev = self._torch_device()
            if is_t:
                P = int(positions.shape[0]) if positions.dim() == 2 else -1
                self._check_tensor("positions", positions, (P, 3))
                x = positions
            else:
                x = torch.from_numpy(np.ascontiguousarray(_f32(positions).reshape(-1, 3))).to(dev)
                P = int(x.shape[0])
            total = torch.zeros((P, K, 3), dtype=torch.float32, device=dev)
            self._on_context_stream(lambda: capi.lib().prt_probe_sh_device(
                self._ctx, C.byref(opt), C.byref(q), P, C.c_void_p(x.data_ptr()), C.c_void_p(total.data_ptr()),
                C.byref(info) if return_info else None))
            if out == "torch":
                # (tensor operands: torch turns a division by a Python number into a multiplication by its reciprocal)
                coeffs = total * torch.full((1, 1, 1), float(np.float32(4.0 * np.pi)), dtype=torch.float32, device=dev) \
                    / torch.full((1, 1, 1), float(q.samples), dtype=torch.float32, device=dev)
            else:
                total = total.cpu().numpy()
                coeffs = total * np.float32(4.0 * np.pi) / np.float32(q.samples)
        else:
            x = np.ascontiguousarray(_f32(positions).reshape(-1, 3))
            P = x.shape[0]
            total = np.zeros((P, K, 3), np.float32)
            self._check(capi.lib().prt_probe_sh(self._ctx, C.byref(opt), C.byref(q), P, x.ctypes.data_as(_fp), total.ctypes.data_as(_fp),
                                                C.byref(info) if return_info else None))
            coeffs = total * np.float32(4.0 * np.pi) / np.float32(q.samples)
        if return_info:
            return coeffs, {"sum": total, "info": {name: getattr(info, name) for name, _ in capi.PrtProbeShInfo._fields_}}
        return coeffs

    # ---- surface baking (include/prt.h "Surface baking") ---------------------------------------------------------
    def _bake_target(self, mesh, instance, size, uvs):
        """The PrtBakeTarget of world-space mesh `mesh` or placed copy `instance` on a size = (H, W) map, and what keeps
        its UV array alive.  uvs: [n_vertices, 2] for this call, None: the texture binding's."""
        if (mesh is None) == (instance is None):
            raise ValueError("bake: give exactly one of mesh= (a world-space mesh) and instance= (a placed copy)")
        H, W = (int(v) for v in size)
        if H < 0 or W < 0 or H > 0xFFFFFFFF or W > 0xFFFFFFFF:
            raise ValueError(f"bake: size {size}")
        index = int(mesh if mesh is not None else instance)
        if index < 0:
            raise ValueError(f"bake: index {index}")
        uv = None if uvs is None else np.ascontiguousarray(_f32(uvs).reshape(-1, 2))
        t = capi.PrtBakeTarget(capi.BAKE_MESH if mesh is not None else capi.BAKE_INSTANCE, index,
                               uv.ctypes.data_as(_fp) if uv is not None else None, W, H)
        return t, uv, H, W

    @staticmethod
    def _bake_info(info: "capi.PrtBakeInfo") -> dict:
        return {name: getattr(info, name) for name, _ in capi.PrtBakeInfo._fields_}

    def bake_surface(self, mesh=None, instance=None, size=(64, 64), uvs=None) -> dict:
        """The surface under every texel of a size = (H, W) map over the UV layout of world-space mesh `mesh` or placed copy
        `instance` (prt_bake_surface): {"owner" [H, W] uint32 (capi.BAKE_NONE: uncovered), "coverage" [H, W] uint8,
        "bary" [H, W, 2] (b1, b2), "position", "normal" [H, W, 3] in world space, "info"}."""
        t, keep, H, W = self._bake_target(mesh, instance, size, uvs)
        owner = np.zeros((H, W), np.uint32)
        bary = np.zeros((H, W, 2), np.float32)
        pos, nrm = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
        info = capi.PrtBakeInfo()
        self._check(capi.lib().prt_bake_surface(self._ctx, C.byref(t), owner.ctypes.data_as(_u32p), bary.ctypes.data_as(_fp),
                                                pos.ctypes.data_as(_fp), nrm.ctypes.data_as(_fp), C.byref(info)))
        return {"owner": owner, "coverage": (owner != capi.BAKE_NONE).astype(np.uint8), "bary": bary, "position": pos, "normal": nrm,
                "info": self._bake_info(info)}

    def bake_rays(self, mesh=None, instance=None, size=(64, 64), uvs=None, sample: int = 0, seed=None) -> dict:
        """The ray of sample `sample` of every texel (prt_bake_rays): {"o", "d" [H, W, 3], "rng_state" [H, W] uint32}, zero
        where the texel is uncovered.  radiance(o, d, rng_state=...) over the covered texels follows a bake's paths."""
        t, keep, H, W = self._bake_target(mesh, instance, size, uvs)
        o, d = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
        rng = np.zeros((H, W), np.uint32)
        self._check(capi.lib().prt_bake_rays(self._ctx, C.byref(t), int(self.seed if seed is None else seed) & 0xFFFFFFFF,
                                             int(sample) & 0xFFFFFFFF, o.ctypes.data_as(_fp), d.ctypes.data_as(_fp), rng.ctypes.data_as(_u32p)))
        return {"o": o, "d": d, "rng_state": rng}

    def bake_light_samples(self, mesh=None, instance=None, size=(64, 64), uvs=None, sample: int = 0, seed=None) -> dict:
        """The light sample of sample `sample` of every texel (prt_bake_light_samples): {"dir" [H, W, 3], "tmax" [H, W] (0: no
        shadow ray is cast), "light" [H, W] uint32 (capi.BAKE_NONE: no sample, capi.LIGHT_ENVIRONMENT), "contrib" [H, W, 3]
        (clamped, before visibility), "ray_pb" [H, W]: the pdf of bake_rays' direction}, zero / none where uncovered."""
        t, keep, H, W = self._bake_target(mesh, instance, size, uvs)
        w, contrib = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
        tmax, pb = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
        light = np.full((H, W), capi.BAKE_NONE, np.uint32)
        self._check(capi.lib().prt_bake_light_samples(self._ctx, C.byref(t), int(self.seed if seed is None else seed) & 0xFFFFFFFF,
                                                      int(sample) & 0xFFFFFFFF, w.ctypes.data_as(_fp), tmax.ctypes.data_as(_fp),
                                                      light.ctypes.data_as(_u32p), contrib.ctypes.data_as(_fp), pb.ctypes.data_as(_fp)))
        return {"dir": w, "tmax": tmax, "light": light, "contrib": contrib, "ray_pb": pb}

    def bake_irradiance(self, mesh=None, instance=None, size=(64, 64), uvs=None, samples: int = 16, seed=None, first_sample: int = 0,
                        max_depth=None, lighting: bool = False, dilate: int = 0, out: str = "numpy", return_info: bool = False,
                        texel_light: bool = False):
        """An irradiance map [H, W, 3] over the UV layout of a mesh (prt_bake_irradiance): every covered texel is a
        Lambertian vertex of albedo 1 whose `samples` paths the radiance query follows; the value is
        sum * float32(pi) / float32(samples), so a Lambertian surface of albedo rho shows rho / pi times it.  lighting:
        radiance()'s.  dilate: passes of the gutter fill.  out = "torch": a tensor on the renderer's device through the
        device form.  return_info: also {"sum": the raw fp32 sums, "coverage": [H, W] uint8 (0 none, 1 owned, 2 filled),
        "info": the counts of the call}.  texel_light (needs lighting=True): a light sample at the texel itself, and the
        texel's own ray MIS-weighted (prt_bake_irradiance_opt): direct light with the noise of a lit render's first vertex."""
        if out not in ("numpy", "torch"):
            raise ValueError(f"out: {out!r}, expected 'numpy' or 'torch'")
        if texel_light and not lighting:
            raise ValueError("texel_light: the texel's light sample belongs to a light-sampled bake: pass lighting=True")
        if int(dilate) < 0 or int(dilate) > 0xFFFFFFFF:
            raise ValueError(f"dilate: {dilate}")
        opt = capi.PrtBakeOptions(int(bool(lighting)), int(bool(texel_light)), int(dilate), 0)
        t, keep, H, W = self._bake_target(mesh, instance, size, uvs)
        q = capi.PrtRadianceQuery(int(self.max_depth if max_depth is None else max_depth), int(samples),
                                  int(self.seed if seed is None else seed) & 0xFFFFFFFF, int(first_sample) & 0xFFFFFFFF)
        info = capi.PrtBakeInfo()
        if out == "torch":
            import torch
            dev = self._torch_device()
            total = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
            cov = torch.zeros((H, W), dtype=torch.uint8, device=dev)
            self._on_context_stream(lambda: capi.lib().prt_bake_irradiance_opt_device(
                self._ctx, C.byref(t), C.byref(q), C.byref(opt), C.c_void_p(total.data_ptr()), C.c_void_p(cov.data_ptr()),
                C.byref(info) if return_info else None))
            # (tensor operands: torch turns a division by a Python number into a multiplication by its reciprocal)
            irr = total * torch.full((1, 1, 1), float(np.float32(np.pi)), dtype=torch.float32, device=dev) \
                / torch.full((1, 1, 1), float(q.samples), dtype=torch.float32, device=dev)
        else:
            total = np.zeros((H, W, 3), np.float32)
            cov = np.zeros((H, W), np.uint8)
            self._check(capi.lib().prt_bake_irradiance_opt(self._ctx, C.byref(t), C.byref(q), C.byref(opt),
                                                           total.ctypes.data_as(_fp), cov.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                           C.byref(info) if return_info else None))
            irr = total * np.float32(np.pi) / np.float32(q.samples)
        if return_info:
            return irr, {"sum": total, "coverage": cov, "info": self._bake_info(info)}
        return irr

    # ---- bake statistics and adaptive sampling (include/prt.h "Bake statistics and adaptive sampling") -----------------
    def bake_irradiance_adaptive(self, mesh=None, instance=None, size=(64, 64), uvs=None, threshold: float = 0.05, min_spp: int = 16,
                                 step_spp: int = 16, max_spp: int = 256, noise_floor: float = 0.01, lighting: bool = False,
                                 texel_light: bool = False, dilate: int = 0, seed=None, first_sample: int = 0, max_depth=None,
                                 out: str = "numpy", return_info: bool = True) -> dict:
        """A bake with per-texel statistics that goes on sampling only where the map is unconverged
        (prt_bake_irradiance_adaptive): min_spp samples to every covered texel, then step_spp at a time to the covered texels
        of the 8x8 blocks that still hold an unconverged one (the film's rule on the texel's luminance moments), up to max_spp.
        A texel that ends with count n equals that texel of bake_irradiance(samples=n) bit for bit.  max_spp == min_spp: the
        uniform bake with statistics.  Returns {"irradiance" [H, W, 3] = float32(pi) * the mean (after `dilate` passes of the
        gutter fill, which touch the mean alone), "sum" [H, W, 3], "count", "sum_y", "sum_y2" [H, W] float32, "coverage"
        [H, W] uint8 (0 none, 1 owned, 2 filled), and with return_info "info": the PrtBakeInfo fields and "adaptive": the
        PrtBakeAdaptiveInfo fields}.  out = "torch": tensors on the renderer's device through the device form.

        Denoising a lightmap is a composition of what exists, no new filter:

            r = R.bake_irradiance_adaptive(mesh=0, size=(H, W), threshold=0.05, lighting=True, texel_light=True)
            n = np.maximum(r["count"], 2.0)
            m = r["sum_y"] / n
            V = np.maximum(r["sum_y2"] / n - m * m, 0.0)            # per-sample variance of the luminance
            var = (V / n).astype(np.float32)                         # variance of the mean: what the filter weighs
            g = R.bake_surface(mesh=0, size=(H, W))                  # the guides
            prim = np.where(g["coverage"] != 0, g["owner"], -1).astype(np.int32)
            mean = r["sum"] / np.maximum(r["count"], 1.0)[..., None]
            smooth = R.denoise_arrays(mean, var, np.ones_like(mean), g["normal"], g["position"], prim)"""
        if out not in ("numpy", "torch"):
            raise ValueError(f"out: {out!r}, expected 'numpy' or 'torch'")
        if texel_light and not lighting:
            raise ValueError("texel_light: the texel's light sample belongs to a light-sampled bake: pass lighting=True")
        if int(dilate) < 0 or int(dilate) > 0xFFFFFFFF:
            raise ValueError(f"dilate: {dilate}")
        for name, v in (("min_spp", min_spp), ("step_spp", step_spp), ("max_spp", max_spp)):
            if int(v) < 0 or int(v) > 0xFFFFFFFF:
                raise ValueError(f"{name}: {v}")
        opt = capi.PrtBakeOptions(int(bool(lighting)), int(bool(texel_light)), int(dilate), 0)
        cfg = capi.PrtBakeAdaptive(int(min_spp), int(step_spp), int(max_spp), float(threshold), float(noise_floor))
        t, keep, H, W = self._bake_target(mesh, instance, size, uvs)
        q = capi.PrtRadianceQuery(int(self.max_depth if max_depth is None else max_depth), 0,
                                  int(self.seed if seed is None else seed) & 0xFFFFFFFF, int(first_sample) & 0xFFFFFFFF)
        info, ainfo = capi.PrtBakeInfo(), capi.PrtBakeAdaptiveInfo()
        if out == "torch":
            import torch
            dev = self._torch_device()
            total, mean = (torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
            cnt, sy, sy2 = (torch.zeros((H, W), dtype=torch.float32, device=dev) for _ in range(3))
            cov = torch.zeros((H, W), dtype=torch.uint8, device=dev)
            self._on_context_stream(lambda: capi.lib().prt_bake_irradiance_adaptive_device(
                self._ctx, C.byref(t), C.byref(q), C.byref(opt), C.byref(cfg), *[C.c_void_p(a.data_ptr()) for a in (total, cnt, sy, sy2, mean, cov)],
                C.byref(info) if return_info else None, C.byref(ainfo)))
            irr = mean * torch.full((1, 1, 1), float(np.float32(np.pi)), dtype=torch.float32, device=dev)
        else:
            total, mean = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
            cnt, sy, sy2 = (np.zeros((H, W), np.float32) for _ in range(3))
            cov = np.zeros((H, W), np.uint8)
            self._check(capi.lib().prt_bake_irradiance_adaptive(
                self._ctx, C.byref(t), C.byref(q), C.byref(opt), C.byref(cfg), *[a.ctypes.data_as(_fp) for a in (total, cnt, sy, sy2, mean)],
                cov.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info) if return_info else None, C.byref(ainfo)))
            irr = mean * np.float32(np.pi)
        r = {"irradiance": irr, "mean": mean, "sum": total, "count": cnt, "sum_y": sy, "sum_y2": sy2, "coverage": cov}
        if return_info:
            r["info"] = self._bake_info(info)
            r["adaptive"] = {name: getattr(ainfo, name) for name, _ in capi.PrtBakeAdaptiveInfo._fields_}
        return r

    def bake_block_select(self, coverage, count, sum_y, sum_y2, threshold: float, noise_floor: float = 0.01, prev=None):
        """prt_bake_block_select: the adaptive bake's selection on [H, W] arrays of coverage bytes, counts and moments.  prev:
        block indices (None: every block, row-major).  Returns (block_list, texel_list): the entries of prev that are active,
        in prev's order, and the covered texels of those blocks in ascending order."""
        cov = np.ascontiguousarray(coverage, np.uint8)
        imgs = [np.ascontiguousarray(a, np.float32) for a in (count, sum_y, sum_y2)]
        if cov.ndim != 2 or any(a.shape != cov.shape for a in imgs):
            raise ValueError("coverage, count, sum_y and sum_y2 must be [H, W]")
        H, W = cov.shape
        if prev is None:
            n_prev, p_prev = ((W + 7) // 8) * ((H + 7) // 8), None
        else:
            prev = np.ascontiguousarray(prev, np.uint32).reshape(-1)
            n_prev, p_prev = prev.size, prev.ctypes.data_as(_u32p)
        blist = np.zeros(max(n_prev, 1), np.uint32)
        tlist = np.zeros(max(H * W, 1), np.uint32)
        counts = np.zeros(2, np.uint32)
        self._check(capi.lib().prt_bake_block_select(self._ctx, W, H, cov.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                     *[a.ctypes.data_as(_fp) for a in imgs], p_prev, n_prev, float(threshold),
                                                     float(noise_floor), blist.ctypes.data_as(_u32p), tlist.ctypes.data_as(_u32p),
                                                     counts.ctypes.data_as(_u32p)))
        if np.any(blist[int(counts[0]):n_prev] != 0xFFFFFFFF) or np.any(tlist[int(counts[1]):H * W] != 0xFFFFFFFF):
            raise PrtError("prt_bake_block_select: an entry past a list's length is not 0xFFFFFFFF")
        return blist[:int(counts[0])].copy(), tlist[:int(counts[1])].copy()

    def enable_timing(self, on: bool = True):
        self._check(capi.lib().prt_enable_timing(self._ctx, int(on)))

    def stats(self) -> PrtStats:
        s = PrtStats()
        self._check(capi.lib().prt_get_stats(self._ctx, C.byref(s)))
        return s

    def reset_stats(self):
        self._check(capi.lib().prt_reset_stats(self._ctx))

    def measure_traversal(self, sample: int = 0) -> PrtStats:
        s = PrtStats()
        self._check(capi.lib().prt_measure_traversal(self._ctx, self.max_depth, self.seed, sample, C.byref(s)))
        return s

    def bvh_info(self) -> PrtBvhInfo:
        b = PrtBvhInfo()
        self._check(capi.lib().prt_bvh_info(self._ctx, C.byref(b)))
        return b

    def kernel_occupancy(self):
        o = capi.PrtOccupancy()
        self._check(capi.lib().prt_kernel_occupancy(self._ctx, C.byref(o)))
        return o

    def Refit(self, scene: "Scene"):
        """prt_refit_meshes: `scene`'s world-space meshes carry new vertex positions / normals over the topology the
        renderer was initialised with; the 8-wide tree is refitted on the device (no rebuild)."""
        d = scene.desc()
        scene._keep = d
        self._check(capi.lib().prt_refit_meshes(self._ctx, d.meshes, d.n_meshes))
        self._scene = scene

    def RefitDevice(self, positions, normals=None):
        """prt_refit_meshes_device: Refit for vertex arrays that are on the renderer's device.  positions: one torch
        tensor, or a list with one per world-space mesh, float32, contiguous, (n_vertices, 3); normals: the same, None
        (area-weighted vertex normals are computed on the device), or a list with None entries.  The tensors are read
        in stream order after torch's current stream; nothing is copied to the host but the emissive triangles."""
        pos, nrm = _device_mesh_arrays(self, getattr(self, "_mesh_vertices", []), positions, normals)
        arr = (capi.PrtMeshDeviceArrays * max(1, len(pos)))()
        for m, (p, q) in enumerate(zip(pos, nrm)):
            arr[m].positions = p.data_ptr()
            arr[m].normals = None if q is None else q.data_ptr()
        self._on_context_stream(lambda: capi.lib().prt_refit_meshes_device(self._ctx, arr, len(pos)))

    def mesh_normals_device(self, mesh: int, positions):
        """prt_mesh_normals_device: the vertex normals the library computes for world-space mesh `mesh` of the scene
        (Mesh(vertices=, indices=) without normals, bit for bit) for positions on the device: an (n_vertices, 3) tensor."""
        import torch
        counts = getattr(self, "_mesh_vertices", [])
        if not 0 <= int(mesh) < len(counts):
            raise ValueError(f"mesh {mesh}: the scene has {len(counts)} world-space meshes")
        self._check_tensor("positions", positions, (counts[int(mesh)], 3))
        out = torch.empty_like(positions)
        self._on_context_stream(lambda: capi.lib().prt_mesh_normals_device(
            self._ctx, int(mesh), C.c_void_p(positions.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def refit_info(self) -> dict:
        """prt_refit_info as a dict: refits, last_form (0 none, 1 host arrays, 2 device arrays), normals_computed,
        host_copies_stale, device_ms, wall_ms, h2d_bytes, d2h_bytes of the last Refit / RefitDevice."""
        info = capi.PrtRefitInfo()
        self._check(capi.lib().prt_refit_info(self._ctx, C.byref(info)))
        return {k: getattr(info, k) for k, _ in capi.PrtRefitInfo._fields_}

    def UpdateInstances(self, scene: "Scene", mode: str = "refit"):
        """prt_set_instance_transforms: `scene`'s placed copies carry new transforms (Scene.SetInstanceTransform) over the
        meshes and materials the renderer was initialised with.  mode "refit" keeps the top-level tree's topology and
        refits it on the device, "rebuild" builds a new top level; no mesh tree is touched, the film is not cleared."""
        insts = (PrtInstance * max(1, len(scene.instances)))(*scene.instances)
        self._check(capi.lib().prt_set_instance_transforms(self._ctx, insts, len(scene.instances), capi.INSTANCE_MODES[mode]))
        self._scene = scene

    def instance_update_info(self) -> "capi.PrtInstanceUpdateInfo":
        info = capi.PrtInstanceUpdateInfo()
        self._check(capi.lib().prt_instance_update_info(self._ctx, C.byref(info)))
        return info

    def instances_read(self) -> dict:
        """prt_instances_read: slot_instance, root, slot_base, prim_base, one uint32 per instance of the top-level tree."""
        n = C.c_uint32(0)
        L = capi.lib()
        self._check(L.prt_instances_read(self._ctx, 0, C.byref(n), None, None, None, None))
        out = {k: np.zeros(n.value, np.uint32) for k in ("slot_instance", "root", "slot_base", "prim_base")}
        self._check(L.prt_instances_read(self._ctx, n.value, C.byref(n), *[out[k].ctypes.data_as(_u32p) for k in out]))
        return out

    def measure_shade_divergence(self, sample: int = 0) -> np.ndarray:
        """prt_measure_shade_divergence: [max_depth, 16] counters of the material mix per wave of the shade kernel."""
        out = np.zeros((self.max_depth, 16), np.uint64)
        self._check(capi.lib().prt_measure_shade_divergence(self._ctx, self.max_depth, self.seed, int(sample),
                                                            out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def kernel_instance(self) -> str:
        """Name of the traversal kernel instance the scene and tunables select (prt_kernel_instance)."""
        buf = C.create_string_buffer(64)
        self._check(capi.lib().prt_kernel_instance(self._ctx, buf, 64))
        return buf.value.decode()

    def shade_instance(self) -> str:
        """Name of the shade kernel instance the last batch launched, as its launch spelled it (prt_shade_instance);
        "" before the first batch."""
        buf = C.create_string_buffer(96)
        self._check(capi.lib().prt_shade_instance(self._ctx, buf, 96))
        return buf.value.decode()

    def batch_instances(self) -> dict:
        """What the last batch launched, stage by stage (prt_batch_instance): {"raygen", "shade0", "shade", "accumulate"} ->
        instance name, "" for a stage that launched nothing ("shade0": bounce 0 only where its instance differs)."""
        return _batch_instances(self._check, self._ctx)

    def last_segment(self):
        """(setting the last batch's plan took for the last-segment route, rays that batch handed to its last tree walk)
        (prt_last_segment); (0, 0) before the first batch."""
        active, front = C.c_uint32(0), C.c_uint32(0)
        self._check(capi.lib().prt_last_segment(self._ctx, C.byref(active), C.byref(front)))
        return active.value, front.value

    def primary_reuse(self):
        """(1 if the last batch started at its first shade launch on the primary stage the context held, else 0; batches that
        did since the context was created) (prt_primary_reuse); (0, 0) before the first batch."""
        active, reused = C.c_uint32(0), C.c_uint32(0)
        self._check(capi.lib().prt_primary_reuse(self._ctx, C.byref(active), C.byref(reused)))
        return active.value, reused.value

    def bvh_read(self):
        b = self.bvh_info()
        nodes = np.zeros((b.n_nodes, 16), np.float32)
        tris = np.zeros((b.n_triangles, 12), np.float32)
        self._check(capi.lib().prt_bvh_read(self._ctx, nodes.ctypes.data_as(_fp), tris.ctypes.data_as(_fp)))
        return nodes, tris

    def bvh_read4(self) -> np.ndarray:
        b = self.bvh_info()
        nodes4 = np.zeros((b.n_nodes4, 32), np.float32)
        self._check(capi.lib().prt_bvh_read4(self._ctx, nodes4.ctypes.data_as(_fp)))
        return nodes4

    def bvh_read8(self) -> np.ndarray:
        """The compressed 8-wide tree: [n_nodes8, 20] uint32 (layout: csrc/bvh.h)."""
        b = self.bvh_info()
        nodes8 = np.zeros((b.n_nodes8, 20), np.uint32)
        self._check(capi.lib().prt_bvh_read8(self._ctx, nodes8.ctypes.data_as(C.POINTER(C.c_uint32))))
        return nodes8

    def set_scene_host_only(self, scene: Scene):
        """For host-only contexts (device < 0): build the BVH without a GPU."""
        d = scene.desc()
        self._check(capi.lib().prt_set_scene(self._ctx, C.byref(d)))
        if scene.textures or scene.material_texture:
            self.set_textures(scene)


class HipWavefrontGroupRenderer:
    """Several GPUs of one node behind the Renderer interface: the binding of the C multi-GPU host path
    (include/prt.h prt_group_*; C++ form: host/prt_renderer.hpp HipWavefrontRenderer(devices)).  One context and one host
    thread per entry of `devices`, image tiled over them, one gather per ProgressiveRender call to devices[0] (RCCL over
    xGMI, or peer copies when a device appears more than once).  Everything happens inside libprt.so."""

    def __init__(self, devices, max_depth: int = DEFAULT_MAX_DEPTH, seed: int = 0):
        self._grp = C.c_void_p()
        L = capi.lib()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        rc = L.prt_group_create(devs, len(devices), C.byref(self._grp))
        if rc:
            msg = L.prt_group_last_error(self._grp).decode()
            L.prt_group_destroy(self._grp)
            self._grp = None
            raise PrtError(f"prt_group_create({list(devices)}) failed: {msg}")
        self.max_depth = int(max_depth)
        self.seed = int(seed)
        self.frame_index = 0
        self.film: Optional[Film] = None

    def __del__(self):
        if getattr(self, "_grp", None):
            capi.lib().prt_group_destroy(self._grp)
            self._grp = None

    def _check(self, rc: int):
        if rc:
            raise PrtError(capi.lib().prt_group_last_error(self._grp).decode())

    @property
    def transport(self) -> str:
        return capi.lib().prt_group_transport(self._grp).decode()

    @property
    def n_devices(self) -> int:
        return capi.lib().prt_group_size(self._grp)

    def Init(self, film: Film, scene: Scene, camera: Camera):
        L = capi.lib()
        d = scene.desc()
        self._check(L.prt_group_set_scene(self._grp, C.byref(d)))
        self._mesh_vertices = [m.n_vertices for m, _ in scene.meshes]
        if scene.textures or scene.material_texture:
            self.set_textures(scene)
        self._check(L.prt_group_set_film(self._grp, film.width, film.height))
        self.film = film
        self.frame_index = 0
        self.SetCamera(camera)

    def SetCamera(self, camera: Camera):
        d = camera.desc()
        self._check(capi.lib().prt_group_set_camera(self._grp, C.byref(d)))

    def Refit(self, scene: Scene):
        """prt_group_refit_meshes: every rank refits its copy of the tree to `scene`'s deformed meshes (same topology)."""
        d = scene.desc()
        scene._keep = d
        self._check(capi.lib().prt_group_refit_meshes(self._grp, d.meshes, d.n_meshes))

    def RefitDevice(self, positions, normals=None):
        """HipWavefrontRenderer.RefitDevice on every rank, one after the other (the C interface has no group form: a
        device array lives on one device).  The tensors are on rank 0's device; the other ranks get copies made by torch."""
        L = capi.lib()
        for rank in range(self.n_devices):
            view = _RankView(L.prt_group_context(self._grp, rank))
            dev = view._torch_device()
            move = lambda t: t if t is None or not hasattr(t, "to") or rank == 0 else t.to(dev)
            one = lambda x: [move(t) for t in x] if isinstance(x, (list, tuple)) else move(x)
            view._mesh_vertices = self._mesh_vertices
            view.RefitDevice(one(positions), one(normals))

    def refit_info(self, rank: int = 0) -> dict:
        return self._rank_view(rank).refit_info()

    def UpdateInstances(self, scene: Scene, mode: str = "refit"):
        """prt_group_set_instance_transforms: every rank moves its copy of the top level to `scene`'s new transforms."""
        insts = (PrtInstance * max(1, len(scene.instances)))(*scene.instances)
        self._check(capi.lib().prt_group_set_instance_transforms(self._grp, insts, len(scene.instances), capi.INSTANCE_MODES[mode]))

    def instance_update_info(self, rank: int = 0) -> "capi.PrtInstanceUpdateInfo":
        info = capi.PrtInstanceUpdateInfo()
        L = capi.lib()
        if L.prt_instance_update_info(L.prt_group_context(self._grp, int(rank)), C.byref(info)):
            raise PrtError(f"prt_instance_update_info failed on rank {rank}")
        return info

    def ProgressiveRender(self, spp: int = 1):
        self._check(capi.lib().prt_group_render(self._grp, spp, self.max_depth, self.seed, self.frame_index))
        self.frame_index += spp

    def Clear(self):
        self._check(capi.lib().prt_group_film_clear(self._grp))
        self.frame_index = 0

    def set_samples_in_flight(self, n: int):
        self._check(capi.lib().prt_group_set_samples_in_flight(self._grp, n))

    def set_param(self, name: str, value: int):
        self._check(capi.lib().prt_group_set_param(self._grp, name.encode(), int(value)))

    def set_sampling(self, jitter: int = 0, rr_depth: int = 0, clamp: float = 0.0) -> PrtSampling:
        sp = PrtSampling(int(jitter), int(rr_depth), float(clamp))
        self._check(capi.lib().prt_group_set_sampling(self._grp, C.byref(sp)))
        return sp

    def set_lens(self, fov_y: float = 0.0, aperture: float = 0.0, focus_distance: float = 0.0) -> capi.PrtLens:
        """Thin lens and field of view on every rank (HipWavefrontRenderer.set_lens)."""
        ln = capi.PrtLens(float(fov_y), float(aperture), float(focus_distance))
        self._check(capi.lib().prt_group_set_lens(self._grp, C.byref(ln)))
        return ln

    def set_feature_trace(self, max_specular: int = 0, roughness_max: float = 0.1) -> capi.PrtFeatureTrace:
        """Guide features through specular chains on every rank (HipWavefrontRenderer.set_feature_trace)."""
        ft = capi.PrtFeatureTrace(int(max_specular), float(roughness_max))
        self._check(capi.lib().prt_group_set_feature_trace(self._grp, C.byref(ft)))
        return ft

    def set_feature_sampling(self, samples: int = 0, seed=None, first_sample: int = 0) -> capi.PrtFeatureSampling:
        """Sampled guide features on every rank (HipWavefrontRenderer.set_feature_sampling)."""
        fs = capi.PrtFeatureSampling(int(samples), int(self.seed if seed is None else seed) & 0xFFFFFFFF, int(first_sample))
        self._check(capi.lib().prt_group_set_feature_sampling(self._grp, C.byref(fs)))
        return fs

    def get_feature_sampling(self) -> capi.PrtFeatureSampling:
        """Rank 0's setting (every rank holds the same)."""
        fs = capi.PrtFeatureSampling()
        L = capi.lib()
        if L.prt_get_feature_sampling(L.prt_group_context(self._grp, 0), C.byref(fs)):
            raise PrtError("prt_get_feature_sampling failed")
        return fs

    def set_film_statistics(self, on: bool = True):
        """HipWavefrontRenderer.set_film_statistics on every rank."""
        L = capi.lib()
        if bool(on) != bool(L.prt_get_film_statistics(L.prt_group_context(self._grp, 0))):
            self.frame_index = 0
        self._check(L.prt_group_set_film_statistics(self._grp, 1 if on else 0))

    def _per_rank(self, read) -> np.ndarray:
        """Assembles an (H, W) map from the ranks' own read-backs: every pixel from the rank that owns its 8x8 tile."""
        L = capi.lib()
        f = self.film
        n = self.n_devices
        ys, xs = np.mgrid[0:f.height, 0:f.width]
        owner = ((ys // 8) * ((f.width + 7) // 8) + xs // 8) % n
        out = np.zeros((f.height, f.width), np.float32)
        for r in range(n):
            ctx = L.prt_group_context(self._grp, r)
            part = np.zeros((f.height, f.width), np.float32)
            if read(ctx, part):
                raise PrtError(L.prt_last_error(ctx).decode())
            out[owner == r] = part[owner == r]
        return out

    def film_statistics(self) -> Tuple[np.ndarray, np.ndarray]:
        L = capi.lib()
        return (self._per_rank(lambda ctx, p: L.prt_film_statistics_read(ctx, p.ctypes.data_as(_fp), None)),
                self._per_rank(lambda ctx, p: L.prt_film_statistics_read(ctx, None, p.ctypes.data_as(_fp))))

    def noise_map(self, noise_floor: float = 0.01) -> np.ndarray:
        L = capi.lib()
        return self._per_rank(lambda ctx, p: L.prt_film_noise_read(ctx, float(noise_floor), p.ctypes.data_as(_fp)))

    def render_adaptive(self, threshold: float, min_spp: int = 8, step_spp: int = 8, max_spp: int = 64,
                        noise_floor: float = 0.01, first_sample: Optional[int] = None) -> "capi.PrtAdaptiveInfo":
        """HipWavefrontRenderer.render_adaptive: every rank loops over its own tiles, then the gather; info summed."""
        cfg = capi.PrtAdaptive(int(min_spp), int(step_spp), int(max_spp), float(threshold), float(noise_floor))
        info = capi.PrtAdaptiveInfo()
        first = self.frame_index if first_sample is None else int(first_sample)
        self._check(capi.lib().prt_group_render_adaptive(self._grp, C.byref(cfg), self.max_depth, self.seed, first, C.byref(info)))
        if first_sample is None:
            self.frame_index += int(max_spp)
        return info

    def render_features(self) -> dict:
        """HipWavefrontRenderer.render_features on rank 0 (every rank holds the scene; the pass covers the whole image)."""
        L = capi.lib()
        ctx = L.prt_group_context(self._grp, 0)

        def check(rc):
            if rc:
                raise PrtError(L.prt_last_error(ctx).decode())
        return _read_features(check, ctx, self.film.width, self.film.height)

    def denoise(self, return_variance: bool = False, **cfg):
        """HipWavefrontRenderer.denoise for the gathered film (prt_group_film_denoise): the single renderer's result bit for bit."""
        k = _denoise_config(**cfg)
        f = self.film
        out = np.zeros((f.height, f.width, 3), np.float32)
        var = np.zeros((f.height, f.width), np.float32) if return_variance else None
        self._check(capi.lib().prt_group_film_denoise(self._grp, C.byref(k), out.ctypes.data_as(_fp),
                                                      var.ctypes.data_as(_fp) if return_variance else None))
        return (out, var) if return_variance else out

    def temporal_step(self, *args, **kwargs):
        """The temporal step has no group form yet: the refusal prt_film_temporal gives a partitioned context."""
        raise PrtError("temporal_step: a group form of the temporal step does not exist yet (prt_film_temporal needs a film that owns the "
                       "whole image: HipWavefrontRenderer with world_size 1)")

    def set_lighting(self, mode) -> int:
        m = capi.LIGHTING_MODES[mode] if isinstance(mode, str) else int(mode)
        self._check(capi.lib().prt_group_set_lighting(self._grp, C.byref(capi.PrtLighting(m))))
        return m

    def set_light_sources(self, sources) -> int:
        m = capi.LIGHT_SOURCES[sources] if isinstance(sources, str) else int(sources)
        self._check(capi.lib().prt_group_set_light_sources(self._grp, m))
        return m

    def set_environment(self, rgb, light_share: float = 0.5):
        """HipWavefrontRenderer.set_environment on every rank."""
        self._check(_set_environment(capi.lib().prt_group_set_environment, self._grp, rgb, light_share))

    def set_textures(self, scene: Optional[Scene]):
        """HipWavefrontRenderer.set_textures on every rank."""
        ts = scene.texture_set() if scene is not None else None
        self._check(capi.lib().prt_group_set_textures(self._grp, None if ts is None else C.byref(ts)))

    def texture_info(self, rank: int = 0) -> "capi.PrtTextureInfo":
        s = capi.PrtTextureInfo()
        L = capi.lib()
        if L.prt_texture_info(L.prt_group_context(self._grp, int(rank)), C.byref(s)):
            raise PrtError(f"prt_texture_info failed on rank {rank}")
        return s

    def set_light_selection(self, selection="power", max_clusters: int = 32) -> int:
        """HipWavefrontRenderer.set_light_selection on every rank."""
        m = capi.LIGHT_SELECTIONS[selection] if isinstance(selection, str) else int(selection)
        self._check(capi.lib().prt_group_set_light_selection(self._grp, C.byref(capi.PrtLightSelection(m, int(max_clusters)))))
        return m

    def batch_instances(self, rank: int = 0) -> dict:
        """HipWavefrontRenderer.batch_instances of one rank's context (every rank plans its batches from the same facts)."""
        v = self._rank_view(rank)
        return _batch_instances(v._check, v._ctx)

    def _rank_view(self, rank: int = 0) -> "_RankView":
        return _RankView(capi.lib().prt_group_context(self._grp, int(rank)))

    def light_cluster_info(self, rank: int = 0) -> "capi.PrtLightClusterInfo":
        return self._rank_view(rank).light_cluster_info()

    def light_clusters(self) -> dict:
        """The clusters as rank 0 holds them (every rank holds the same)."""
        return self._rank_view().light_clusters()

    def light_cluster_members(self) -> Tuple[np.ndarray, np.ndarray]:
        return self._rank_view().light_cluster_members()

    def light_cluster_pmf(self, x, rank: int = 0) -> np.ndarray:
        return self._rank_view(rank).light_cluster_pmf(x)

    def light_info(self) -> Tuple[np.ndarray, np.ndarray]:
        """The light set as rank 0 holds it (every rank holds the same)."""
        L = capi.lib()
        ctx = L.prt_group_context(self._grp, 0)
        n = C.c_uint32(0)
        if L.prt_light_info(ctx, 0, C.byref(n), None, None):
            raise PrtError(L.prt_last_error(ctx).decode())
        prim = np.zeros(n.value, np.uint32)
        pmf = np.zeros(n.value, np.float32)
        if L.prt_light_info(ctx, n.value, C.byref(n), prim.ctypes.data_as(_u32p), pmf.ctypes.data_as(_fp)):
            raise PrtError(L.prt_last_error(ctx).decode())
        return prim, pmf

    def light_stats(self) -> "capi.PrtLightStats":
        s = capi.PrtLightStats()
        self._check(capi.lib().prt_group_get_light_stats(self._grp, C.byref(s)))
        return s

    def download(self) -> Film:
        f = self.film
        self._check(capi.lib().prt_group_film_read(self._grp, f.accum.ctypes.data_as(_fp), f.weights.ctypes.data_as(_fp)))
        return f

    def UpdateDisplay(self, exposure: float = 1.0, gamma: float = 2.2) -> np.ndarray:
        f = self.film
        self._check(capi.lib().prt_group_film_display(self._grp, exposure, gamma, f.display.ctypes.data_as(C.POINTER(C.c_uint8))))
        return f.display

    def stats(self) -> PrtStats:
        s = PrtStats()
        self._check(capi.lib().prt_group_get_stats(self._grp, C.byref(s)))
        return s


class _RankView:
    """One rank's context of a group (borrowed, never destroyed) behind the single renderer's cluster read-backs."""

    def __init__(self, ctx):
        self._ctx = ctx

    def _check(self, rc: int):
        if rc != 0:
            raise PrtError(capi.lib().prt_last_error(self._ctx).decode())

    light_cluster_info = HipWavefrontRenderer.light_cluster_info
    light_clusters = HipWavefrontRenderer.light_clusters
    light_cluster_members = HipWavefrontRenderer.light_cluster_members
    light_cluster_pmf = HipWavefrontRenderer.light_cluster_pmf
    _torch_device = HipWavefrontRenderer._torch_device
    _check_tensor = HipWavefrontRenderer._check_tensor
    _on_context_stream = HipWavefrontRenderer._on_context_stream
    RefitDevice = HipWavefrontRenderer.RefitDevice
    refit_info = HipWavefrontRenderer.refit_info


def _device_mesh_arrays(renderer, counts, positions, normals):
    """RefitDevice's arguments as two lists with one entry per world-space mesh, checked (dtype, shape, device,
    contiguity, length) before the library sees a pointer: it has no way to know how long a device array is."""
    pos = list(positions) if isinstance(positions, (list, tuple)) else [positions]
    nrm = list(normals) if isinstance(normals, (list, tuple)) else [normals] * len(pos) if normals is None else [normals]
    if len(pos) != len(counts):
        raise ValueError(f"positions: {len(pos)} tensors, the scene has {len(counts)} world-space meshes")
    if len(nrm) != len(counts):
        raise ValueError(f"normals: {len(nrm)} entries, the scene has {len(counts)} world-space meshes")
    for m, (p, q) in enumerate(zip(pos, nrm)):
        renderer._check_tensor(f"positions[{m}]", p, (counts[m], 3))
        if q is not None:
            renderer._check_tensor(f"normals[{m}]", q, (counts[m], 3))
    return pos, nrm


def _batch_instances(check, ctx) -> dict:
    out = {}
    buf = C.create_string_buffer(96)
    for stage, k in capi.STAGES.items():
        check(capi.lib().prt_batch_instance(ctx, k, buf, 96))
        out[stage] = buf.value.decode()
    return out


def instance_names(stage: str) -> list:
    """Every kernel instance a batch can launch in `stage` ("raygen", "shade", "accumulate"; "shade0" walks the shade list), in
    the order of the instance lists of csrc/prt_route.h (prt_instance_name)."""
    out = []
    buf = C.create_string_buffer(96)
    while capi.lib().prt_instance_name(capi.STAGES[stage], len(out), buf, 96) == 0:
        out.append(buf.value.decode())
    return out


def _set_environment(fn, handle, rgb, light_share) -> int:
    if rgb is None:
        return fn(handle, None)
    a = _f32(rgb)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("environment: rgb must be [H, W, 3]")
    e = capi.PrtEnvironment(a.ctypes.data_as(_fp), a.shape[1], a.shape[0], float(light_share))
    return fn(handle, C.byref(e))


def probe_directions(H: int, W: int) -> np.ndarray:
    """Unit directions [H, W, 3] float32 of the texel centres of a lat-long image in set_environment's convention (row 0 =
    +Y pole; include/prt.h "Environment light"): u = (j + 1/2) / W, v = (i + 1/2) / H, phi = 2 pi u - pi, theta = pi v,
    w = (sin theta cos phi, cos theta, sin theta sin phi).  Evaluated in float64 and rounded once, so each direction is a
    unit vector to fp32 rounding and looks up its own texel (a centre is half a texel from every edge)."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("probe_directions: H and W must be at least 1")
    # (sin / cos through the C library, one call per row and column: the C++ adapter's RenderProbe spells the same lines)
    phi = [2.0 * math.pi * ((j + 0.5) / W) - math.pi for j in range(W)]
    theta = [math.pi * ((i + 0.5) / H) for i in range(H)]
    cp, sp = np.array([math.cos(p) for p in phi])[None, :], np.array([math.sin(p) for p in phi])[None, :]
    ct, st = np.array([math.cos(t) for t in theta])[:, None], np.array([math.sin(t) for t in theta])[:, None]
    x, y, z = st * cp, np.broadcast_to(ct, (H, W)), st * sp
    inv = 1.0 / np.sqrt((x * x + y * y) + z * z)
    return np.stack([x * inv, y * inv, z * inv], axis=-1).astype(np.float32)


def sh_basis(d, order: int = 2) -> np.ndarray:
    """The real spherical harmonics of include/prt.h "SH probes" at directions d [..., 3] (used as given, not normalised):
    [..., (order + 1)^2] float32, through the library's own lines (prt_sh_eval; no context, no device)."""
    a = _f32(d)
    if a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError(f"sh_basis: d must be [..., 3], got {a.shape}")
    if not 0 <= int(order) <= capi.SH_MAX_ORDER:
        raise ValueError(f"sh_basis: order {order}, expected 0 .. {capi.SH_MAX_ORDER}")
    K = (int(order) + 1) ** 2
    flat = np.ascontiguousarray(a.reshape(-1, 3))
    Y = np.zeros((flat.shape[0], K), np.float32)
    if capi.lib().prt_sh_eval(flat.shape[0], flat.ctypes.data_as(_fp), int(order), Y.ctypes.data_as(_fp)):
        raise PrtError("prt_sh_eval failed")
    return Y.reshape(a.shape[:-1] + (K,))


def bake_noise(count, sum_y, sum_y2, noise_floor: float = 0.01):
    """The relative standard error of every texel's mean luminance from an adaptive bake's count and moments (prt_bake_noise;
    a pure host function): 0 where count == 0 (an uncovered texel), +inf where count < 2, else sqrt(V / (count - 1)) /
    (m + noise_floor) with m = sum_y / count, V = max(0, sum_y2 / count - m^2).  The arrays' shape is kept."""
    c, a, q = (np.ascontiguousarray(x, np.float32) for x in (count, sum_y, sum_y2))
    if a.shape != c.shape or q.shape != c.shape:
        raise ValueError("count, sum_y and sum_y2 must have one shape")
    out = np.zeros(c.shape, np.float32)
    if capi.lib().prt_bake_noise(c.size, c.ctypes.data_as(_fp), a.ctypes.data_as(_fp), q.ctypes.data_as(_fp), float(noise_floor),
                                 out.ctypes.data_as(_fp)):
        raise PrtError("prt_bake_noise failed")
    return out


def sh_irradiance(coeffs, normals) -> np.ndarray:
    """The irradiance E [..., 3] float32 that radiance coefficients [..., K, 3] (K = 1, 4 or 9: what probe_sh returns) give
    on a surface of normal `normals` [..., 3] (prt_sh_irradiance; a pure host function).  The leading shapes broadcast: one
    set of coefficients under many normals, or one normal for many probes.  Not clamped."""
    c, n = _f32(coeffs), _f32(normals)
    if c.ndim < 2 or c.shape[-1] != 3 or c.shape[-2] not in (1, 4, 9):
        raise ValueError(f"sh_irradiance: coeffs must be [..., 1 | 4 | 9, 3], got {c.shape}")
    if n.ndim < 1 or n.shape[-1] != 3:
        raise ValueError(f"sh_irradiance: normals must be [..., 3], got {n.shape}")
    K = c.shape[-2]
    lead = np.broadcast_shapes(c.shape[:-2], n.shape[:-1])
    cf = np.ascontiguousarray(np.broadcast_to(c, lead + (K, 3)).reshape(-1, K, 3))
    nf = np.ascontiguousarray(np.broadcast_to(n, lead + (3,)).reshape(-1, 3))
    E = np.zeros((cf.shape[0], 3), np.float32)
    if capi.lib().prt_sh_irradiance(cf.shape[0], cf.ctypes.data_as(_fp), nf.ctypes.data_as(_fp), {1: 0, 4: 1, 9: 2}[K], E.ctypes.data_as(_fp)):
        raise PrtError("prt_sh_irradiance failed")
    return E.reshape(lead + (3,))


def probe_grid(lo, hi, counts) -> np.ndarray:
    """Cell-centred probe positions [nx * ny * nz, 3] float32 of an nx x ny x nz grid over the box lo .. hi, x fastest:
    probe (i, j, k) has index (k * ny + j) * nx + i and lies at lo + (index + 1/2) * (hi - lo) / count per axis (float64,
    rounded once)."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    nx, ny, nz = (int(v) for v in counts)
    if min(nx, ny, nz) < 1:
        raise ValueError(f"probe_grid: counts {counts}, expected at least 1 each way")
    ax = [lo[a] + (np.arange(n) + 0.5) * ((hi[a] - lo[a]) / n) for a, n in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)


def read_pfm(path: str) -> np.ndarray:
    """prt_read_pfm: a colour PFM as [H, W, 3] float32, top row first."""
    p, w, h = _fp(), C.c_uint32(0), C.c_uint32(0)
    rc = capi.lib().prt_read_pfm(path.encode(), C.byref(p), C.byref(w), C.byref(h))
    if rc:
        raise PrtError(f"prt_read_pfm({path}) failed ({rc})")
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        capi.lib().prt_image_free(p)


def write_ppm(path: str, rgba8: np.ndarray):
    a = np.ascontiguousarray(rgba8, dtype=np.uint8)
    if capi.lib().prt_write_ppm(path.encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0]):
        raise PrtError(f"cannot write {path}")


def write_pfm(path: str, rgb: np.ndarray):
    a = _f32(rgb)
    if capi.lib().prt_write_pfm(path.encode(), a.ctypes.data_as(_fp), a.shape[1], a.shape[0]):
        raise PrtError(f"cannot write {path}")
