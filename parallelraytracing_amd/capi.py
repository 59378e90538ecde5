"""ctypes binding of include/prt.h (libprt.so).

The library is the product: there is no Python or CPU fallback.  If libprt.so is missing the import
fails loudly with the build command to run.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PRT_LIB_PATH: tuning hook (tools/ab_libs.py times alternative BUILDS of the same sources, e.g. other compiler flags)
LIB_PATH = os.environ.get("PRT_LIB_PATH") or os.path.join(_HERE, "csrc", "libprt.so")

PRT_MAX_DEPTH = 64

# shape / material / preset enums (include/prt.h)
SHAPE_CIRCLE, SHAPE_QUAD, SHAPE_TRIANGLE = 0, 1, 2
MAT_NONE, MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_EMISSIVE = 0, 1, 2, 3, 4
(PRESET_DEFAULT, PRESET_LIGHT_TEST, PRESET_MATERIAL_TEST, PRESET_CORNELL, PRESET_RANDOM_BALLS_SMALL,
 PRESET_RANDOM_BALLS_MEDIUM, PRESET_RANDOM_BALLS_LARGE) = range(7)
PRESET_NAMES = {
    "DEFAULT": PRESET_DEFAULT, "LIGHT_TEST": PRESET_LIGHT_TEST, "MATERIAL_TEST": PRESET_MATERIAL_TEST,
    "CORNELL": PRESET_CORNELL, "RANDOM_BALLS_SMALL": PRESET_RANDOM_BALLS_SMALL,
    "RANDOM_BALLS_MEDIUM": PRESET_RANDOM_BALLS_MEDIUM, "RANDOM_BALLS_LARGE": PRESET_RANDOM_BALLS_LARGE,
}


class PrtMaterial(C.Structure):
    _fields_ = [("type", C.c_uint32), ("rgb", C.c_float * 3), ("scalar", C.c_float)]


class PrtPrimitive(C.Structure):
    _fields_ = [("shape_type", C.c_uint32), ("shape_param", C.c_float * 2), ("material_id", C.c_uint32),
                ("mat", C.c_float * 16), ("inv", C.c_float * 16)]


class PrtMesh(C.Structure):
    _fields_ = [("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("indices", C.POINTER(C.c_uint32)), ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32),
                ("material_id", C.c_uint32)]


class PrtInstance(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("material_id", C.c_uint32), ("mat", C.c_float * 16), ("inv", C.c_float * 16)]


class PrtSceneDesc(C.Structure):
    _fields_ = [("materials", C.POINTER(PrtMaterial)), ("primitives", C.POINTER(PrtPrimitive)),
                ("meshes", C.POINTER(PrtMesh)), ("n_materials", C.c_uint32), ("n_primitives", C.c_uint32),
                ("n_meshes", C.c_uint32), ("sky", C.c_float * 3),
                ("instanced_meshes", C.POINTER(PrtMesh)), ("instances", C.POINTER(PrtInstance)),
                ("n_instanced_meshes", C.c_uint32), ("n_instances", C.c_uint32)]


class PrtCameraDesc(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("front", C.c_float * 3), ("width", C.c_float), ("height", C.c_float)]


class PrtHit(C.Structure):
    _fields_ = [("prim", C.c_int32), ("front_face", C.c_uint32), ("material_id", C.c_uint32), ("d2", C.c_float),
                ("position", C.c_float * 3), ("normal", C.c_float * 3)]


class PrtStats(C.Structure):
    _fields_ = [("rays_total", C.c_uint64), ("rays_per_depth", C.c_uint64 * PRT_MAX_DEPTH), ("samples", C.c_uint64),
                ("intersect_launches", C.c_uint64), ("intersect_ms", C.c_double), ("shade_ms", C.c_double),
                ("raygen_ms", C.c_double), ("accumulate_ms", C.c_double), ("bvh_node_visits", C.c_uint64),
                ("bvh_tri_tests", C.c_uint64), ("prim_tests", C.c_uint64), ("node_lane_slots", C.c_uint64),
                ("scan_ms", C.c_double), ("rays_traversed", C.c_uint64), ("tri_lane_slots", C.c_uint64), ("max_stack_used", C.c_uint64),
                ("wave_cycles_refill", C.c_uint64), ("wave_cycles_node", C.c_uint64), ("wave_cycles_tri", C.c_uint64)]


class PrtOccupancy(C.Structure):
    _fields_ = [("blocks_per_cu", C.c_uint32), ("waves_per_cu", C.c_uint32), ("max_waves_per_cu", C.c_uint32),
                ("vgprs", C.c_uint32), ("lds_bytes_per_block", C.c_uint32), ("compute_units", C.c_uint32),
                ("resident_grid_blocks", C.c_uint32)]


class PrtSampling(C.Structure):
    _fields_ = [("jitter", C.c_uint32), ("rr_depth", C.c_uint32), ("clamp", C.c_float)]


class PrtLens(C.Structure):
    _fields_ = [("fov_y", C.c_float), ("aperture", C.c_float), ("focus_distance", C.c_float)]


class PrtFeatureTrace(C.Structure):
    """Guide features through specular chains (include/prt.h): 0 = first hit only."""
    _fields_ = [("max_specular", C.c_uint32), ("roughness_max", C.c_float)]


class PrtFeatureSampling(C.Structure):
    """Sampled guide features (include/prt.h): samples = 0 = off; seed and first_sample of the prt_render calls meant."""
    _fields_ = [("samples", C.c_uint32), ("seed", C.c_uint32), ("first_sample", C.c_uint32)]


class PrtRadianceQuery(C.Structure):
    """Settings of prt_radiance (include/prt.h "Radiance query")."""
    _fields_ = [("max_depth", C.c_uint32), ("samples", C.c_uint32), ("seed", C.c_uint32), ("first_sample", C.c_uint32)]


RADIANCE_MAX_SAMPLES = 4096  # PRT_RADIANCE_MAX_SAMPLES


class PrtRadianceLitInfo(C.Structure):
    """What one prt_radiance_lit call cast (include/prt.h "Radiance query")."""
    _fields_ = [("shadow_rays", C.c_uint64), ("shadow_occluded", C.c_uint64)]


BAKE_MESH, BAKE_INSTANCE = 0, 1  # PRT_BAKE_MESH, PRT_BAKE_INSTANCE
BAKE_NONE = 0xFFFFFFFF            # owner of an uncovered texel


class PrtBakeTarget(C.Structure):
    """What a bake rasterises (include/prt.h "Surface baking")."""
    _fields_ = [("kind", C.c_uint32), ("index", C.c_uint32), ("uvs", C.POINTER(C.c_float)), ("width", C.c_uint32), ("height", C.c_uint32)]


class PrtBakeInfo(C.Structure):
    """The counts of one bake (include/prt.h "Surface baking")."""
    _fields_ = [("n_texels", C.c_uint64), ("n_covered", C.c_uint64), ("n_degenerate", C.c_uint64), ("n_faces_skipped", C.c_uint64),
                ("n_filled", C.c_uint64), ("rays", C.c_uint64), ("segments", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("shadow_occluded", C.c_uint64), ("device_ms", C.c_double)]


class PrtBakeOptions(C.Structure):
    """The options of prt_bake_irradiance_opt (include/prt.h "Surface baking"); reserved must be 0."""
    _fields_ = [("lighting", C.c_uint32), ("texel_light", C.c_uint32), ("dilate", C.c_uint32), ("reserved", C.c_uint32)]


class PrtBakeAdaptive(C.Structure):
    """Settings of prt_bake_irradiance_adaptive (include/prt.h "Bake statistics and adaptive sampling"); reserved must be 0."""
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("max_spp", C.c_uint32), ("threshold", C.c_float),
                ("noise_floor", C.c_float), ("reserved", C.c_uint32 * 3)]


class PrtBakeAdaptiveInfo(C.Structure):
    """What one prt_bake_irradiance_adaptive call did (include/prt.h "Bake statistics and adaptive sampling")."""
    _fields_ = [("passes", C.c_uint32), ("blocks", C.c_uint32), ("blocks_converged", C.c_uint32), ("blocks_capped", C.c_uint32),
                ("min_texel_spp", C.c_uint32), ("max_texel_spp", C.c_uint32), ("texel_samples", C.c_uint64)]


SH_MAX_ORDER = 2  # PRT_SH_MAX_ORDER


class PrtProbeShOptions(C.Structure):
    """The options of prt_probe_sh (include/prt.h "SH probes"); reserved must be 0."""
    _fields_ = [("order", C.c_uint32), ("lighting", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PrtProbeShInfo(C.Structure):
    """The counts of one prt_probe_sh call (include/prt.h "SH probes")."""
    _fields_ = [("n_probes", C.c_uint64), ("rays", C.c_uint64), ("segments", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("shadow_occluded", C.c_uint64), ("device_ms", C.c_double)]


class PrtAdaptive(C.Structure):
    """Settings of prt_render_adaptive (include/prt.h "Film statistics and adaptive sampling")."""
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("max_spp", C.c_uint32), ("threshold", C.c_float),
                ("noise_floor", C.c_float)]


class PrtAdaptiveInfo(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("tiles_local", C.c_uint32), ("tiles_converged", C.c_uint32),
                ("tiles_capped", C.c_uint32), ("min_tile_spp", C.c_uint32), ("max_tile_spp", C.c_uint32),
                ("pixel_samples", C.c_uint64)]


class PrtDenoise(C.Structure):
    """Settings of the film denoiser (include/prt.h "The filter contract"); prt_denoise_defaults fills the defaults."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_l", C.c_float), ("sigma_z", C.c_float),
                ("normal_power_log2", C.c_uint32), ("demodulate", C.c_uint32)]


DENOISE_MAX_PIXELS = 1 << 28  # PRT_DENOISE_MAX_PIXELS


class PrtTemporal(C.Structure):
    """Settings of the temporal reprojection (include/prt.h "Temporal reprojection"); prt_temporal_defaults fills the defaults."""
    _fields_ = [("max_history", C.c_float), ("normal_min", C.c_float), ("plane_tol", C.c_float)]


class PrtCameraBasis(C.Structure):
    """The camera as the kernels have it (prt_get_camera_basis)."""
    _fields_ = [("pos", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("front", C.c_float * 3),
                ("W", C.c_float), ("H", C.c_float), ("tan_fov_y", C.c_float)]


class PrtTemporalInfo(C.Structure):
    _fields_ = [("steps", C.c_uint32), ("resets", C.c_uint32), ("hit_pixels", C.c_uint32), ("reprojected", C.c_uint32),
                ("device_bytes", C.c_uint64)]


TEMPORAL_MAX_PIXELS = 1 << 28  # PRT_TEMPORAL_MAX_PIXELS


class PrtLighting(C.Structure):
    _fields_ = [("mode", C.c_uint32)]


class PrtLightStats(C.Structure):
    _fields_ = [("shadow_rays", C.c_uint64), ("shadow_occluded", C.c_uint64), ("n_lights", C.c_uint32),
                ("n_emitters_unsampled", C.c_uint32)]


class PrtEnvironment(C.Structure):
    _fields_ = [("rgb", C.POINTER(C.c_float)), ("width", C.c_uint32), ("height", C.c_uint32), ("light_share", C.c_float)]


class PrtEnvironmentInfo(C.Structure):
    _fields_ = [("is_set", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("n_sampled", C.c_uint32),
                ("t_env", C.c_uint64), ("light_share", C.c_float)]


class PrtTexture(C.Structure):
    _fields_ = [("rgb", C.POINTER(C.c_float)), ("width", C.c_uint32), ("height", C.c_uint32), ("filter", C.c_uint32),
                ("wrap", C.c_uint32)]


class PrtTextureSet(C.Structure):
    _fields_ = [("textures", C.POINTER(PrtTexture)), ("n_textures", C.c_uint32),
                ("material_texture", C.POINTER(C.c_uint32)), ("n_materials", C.c_uint32),
                ("mesh_uvs", C.POINTER(C.POINTER(C.c_float))), ("n_meshes", C.c_uint32),
                ("instanced_mesh_uvs", C.POINTER(C.POINTER(C.c_float))), ("n_instanced_meshes", C.c_uint32)]


class PrtTextureInfo(C.Structure):
    _fields_ = [("is_set", C.c_uint32), ("n_textures", C.c_uint32), ("n_textured_materials", C.c_uint32),
                ("n_uv_triangles", C.c_uint32), ("n_texels", C.c_uint64), ("device_bytes", C.c_uint64)]


# PrtTexture.filter / wrap (include/prt.h PRT_TEX_*)
TEX_FILTERS = {"nearest": 0, "bilinear": 1}
TEX_WRAPS = {"repeat": 0, "clamp": 1}
TEXTURE_NONE = 0xFFFFFFFF  # PRT_TEXTURE_NONE
TEX_MAX_SIZE = 16384       # PRT_TEX_MAX_SIZE

LIGHT_ENVIRONMENT = 0xFFFFFFFE  # PRT_LIGHT_ENVIRONMENT
ENV_RNG = 0x3C6EF372            # PRT_ENV_RNG

# PrtLighting.mode (include/prt.h)
LIGHTING_MODES = {"off": 0, "mis": 1, "nee": 2}
STAGES = {"raygen": 0, "shade0": 1, "shade": 2, "accumulate": 3}  # PRT_STAGE_* (prt_batch_instance, prt_instance_name)
# prt_set_light_sources masks (include/prt.h PRT_LIGHT_SOURCES_*)
LIGHT_SOURCES = {"analytic": 1, "all": 3}
# PrtLightSelection.mode (include/prt.h PRT_LIGHT_SELECTION_*)
LIGHT_SELECTIONS = {"power": 0, "clustered": 1}
LIGHT_MAX_CLUSTERS = 64


class PrtLightSelection(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("max_clusters", C.c_uint32)]


class PrtLightClusterInfo(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("active", C.c_uint32), ("n_clusters", C.c_uint32), ("max_clusters", C.c_uint32),
                ("n_empty_inner", C.c_uint32)]


class PrtBvhInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_triangles", C.c_uint32), ("max_depth", C.c_uint32),
                ("max_leaf_size", C.c_uint32), ("sah_cost", C.c_float), ("pad_abs", C.c_float),
                ("node_bytes", C.c_uint64), ("tri_bytes", C.c_uint64), ("n_nodes4", C.c_uint32), ("max_stack4", C.c_uint32),
                ("n_nodes8", C.c_uint32), ("depth8", C.c_uint32), ("build_ms", C.c_float),
                ("built_on_device", C.c_uint32), ("refit_ms", C.c_float), ("refits", C.c_uint32)]


class PrtMeshDeviceArrays(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p)]


class PrtRefitInfo(C.Structure):
    _fields_ = [("refits", C.c_uint32), ("last_form", C.c_uint32), ("normals_computed", C.c_uint32),
                ("host_copies_stale", C.c_uint32), ("device_ms", C.c_float), ("wall_ms", C.c_float),
                ("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64)]


class PrtInstanceUpdateInfo(C.Structure):
    _fields_ = [("updates", C.c_uint32), ("last_mode", C.c_uint32), ("top_nodes", C.c_uint32), ("top_depth", C.c_uint32),
                ("last_ms", C.c_float)]


# prt_set_instance_transforms modes (include/prt.h PRT_INSTANCES_*)
INSTANCE_MODES = {"refit": 0, "rebuild": 1}

# numpy dtype mirror of PrtHit (40 bytes)
HIT_DTYPE = [("prim", "<i4"), ("front_face", "<u4"), ("material_id", "<u4"), ("d2", "<f4"),
             ("position", "<f4", (3,)), ("normal", "<f4", (3,))]

_vp = C.c_void_p
_fp = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)

# name -> (restype, argtypes).  Every symbol include/prt.h declares is listed here; the CPU test-suite
# checks that each one is exported by the built library.
SIGNATURES = {
    "prt_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "prt_destroy": (None, [_vp]),
    "prt_last_error": (C.c_char_p, [_vp]),
    "prt_version": (C.c_int, []),
    "prt_device_memory_info": (None, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "prt_set_stream": (C.c_int, [_vp, _vp]),
    "prt_get_stream": (C.c_int, [_vp, C.POINTER(_vp)]),
    "prt_get_device": (C.c_int, [_vp]),
    "prt_clone_scene": (C.c_int, [_vp, _vp]),
    "prt_group_create": (C.c_int, [C.POINTER(C.c_int), C.c_uint32, C.POINTER(_vp)]),
    "prt_group_destroy": (None, [_vp]),
    "prt_group_last_error": (C.c_char_p, [_vp]),
    "prt_group_size": (C.c_uint32, [_vp]),
    "prt_group_transport": (C.c_char_p, [_vp]),
    "prt_group_context": (_vp, [_vp, C.c_uint32]),
    "prt_group_set_scene": (C.c_int, [_vp, C.POINTER(PrtSceneDesc)]),
    "prt_group_refit_meshes": (C.c_int, [_vp, C.POINTER(PrtMesh), C.c_uint32]),
    "prt_group_set_camera": (C.c_int, [_vp, C.POINTER(PrtCameraDesc)]),
    "prt_group_set_film": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "prt_group_film_clear": (C.c_int, [_vp]),
    "prt_group_set_sampling": (C.c_int, [_vp, C.POINTER(PrtSampling)]),
    "prt_group_set_samples_in_flight": (C.c_int, [_vp, C.c_uint32]),
    "prt_group_set_lens": (C.c_int, [_vp, C.POINTER(PrtLens)]),
    "prt_set_lens": (C.c_int, [_vp, C.POINTER(PrtLens)]),
    "prt_get_lens": (C.c_int, [_vp, C.POINTER(PrtLens)]),
    "prt_camera_rays_lens": (C.c_int, [_vp, C.c_uint32, _fp, _fp, _u32p, _fp, _fp]),
    "prt_group_set_param": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "prt_group_render": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "prt_group_film_read": (C.c_int, [_vp, _fp, _fp]),
    "prt_group_film_display": (C.c_int, [_vp, C.c_float, C.c_float, C.POINTER(C.c_uint8)]),
    "prt_group_get_stats": (C.c_int, [_vp, C.POINTER(PrtStats)]),
    "prt_group_set_lighting": (C.c_int, [_vp, C.POINTER(PrtLighting)]),
    "prt_group_get_light_stats": (C.c_int, [_vp, C.POINTER(PrtLightStats)]),
    "prt_group_set_light_sources": (C.c_int, [_vp, C.c_uint32]),
    "prt_set_light_sources": (C.c_int, [_vp, C.c_uint32]),
    "prt_set_light_selection": (C.c_int, [_vp, C.POINTER(PrtLightSelection)]),
    "prt_group_set_light_selection": (C.c_int, [_vp, C.POINTER(PrtLightSelection)]),
    "prt_light_cluster_info": (C.c_int, [_vp, C.POINTER(PrtLightClusterInfo)]),
    "prt_light_clusters": (C.c_int, [_vp, C.c_uint32, _u32p, _fp, _fp, _fp, _fp, C.POINTER(C.c_uint64), _u32p]),
    "prt_light_cluster_members": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, C.POINTER(C.c_uint64)]),
    "prt_light_cluster_pmf": (C.c_int, [_vp, C.c_uint32, _fp, _u32p]),
    "prt_light_intervals": (C.c_int, [_vp, C.c_uint32, _u32p, C.POINTER(C.c_uint64)]),
    "prt_set_environment": (C.c_int, [_vp, C.POINTER(PrtEnvironment)]),
    "prt_group_set_environment": (C.c_int, [_vp, C.POINTER(PrtEnvironment)]),
    "prt_environment_info": (C.c_int, [_vp, C.POINTER(PrtEnvironmentInfo)]),
    "prt_environment_intervals": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "prt_environment_eval": (C.c_int, [_vp, C.c_uint32, _fp, _fp, _u32p, _fp]),
    "prt_set_textures": (C.c_int, [_vp, C.POINTER(PrtTextureSet)]),
    "prt_group_set_textures": (C.c_int, [_vp, C.POINTER(PrtTextureSet)]),
    "prt_texture_info": (C.c_int, [_vp, C.POINTER(PrtTextureInfo)]),
    "prt_texture_eval": (C.c_int, [_vp, C.c_uint32, _u32p, _fp, _fp]),
    "prt_hit_uv": (C.c_int, [_vp, C.c_uint32, _fp, _fp, C.POINTER(PrtHit), _fp, _fp]),
    "prt_mesh_uvs": (_fp, [_vp]),
    "prt_mesh_had_uvs": (C.c_int, [_vp]),
    "prt_mesh_set_uvs": (C.c_int, [_vp, _fp]),
    "prt_read_pfm": (C.c_int, [C.c_char_p, C.POINTER(_fp), _u32p, _u32p]),
    "prt_image_free": (None, [_fp]),
    "prt_set_film_statistics": (C.c_int, [_vp, C.c_int]),
    "prt_get_film_statistics": (C.c_int, [_vp]),
    "prt_film_statistics_read": (C.c_int, [_vp, _fp, _fp]),
    "prt_film_noise_read": (C.c_int, [_vp, C.c_float, _fp]),
    "prt_adaptive_unconverged": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "prt_render_adaptive": (C.c_int, [_vp, C.POINTER(PrtAdaptive), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PrtAdaptiveInfo)]),
    "prt_tile_select": (C.c_int, [_vp, _fp, _fp, _fp, _u32p, C.c_uint32, C.c_float, C.c_float, _u32p, _u32p]),
    "prt_group_set_film_statistics": (C.c_int, [_vp, C.c_int]),
    "prt_group_render_adaptive": (C.c_int, [_vp, C.POINTER(PrtAdaptive), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PrtAdaptiveInfo)]),
    "prt_denoise_defaults": (None, [C.POINTER(PrtDenoise)]),
    "prt_denoise_variance": (C.c_float, [C.c_float, C.c_float, C.c_float]),
    "prt_render_features": (C.c_int, [_vp]),
    "prt_features_read": (C.c_int, [_vp, _fp, _fp, _fp, _fp, C.POINTER(C.c_int32)]),
    "prt_feature_trace_defaults": (None, [C.POINTER(PrtFeatureTrace)]),
    "prt_set_feature_trace": (C.c_int, [_vp, C.POINTER(PrtFeatureTrace)]),
    "prt_get_feature_trace": (C.c_int, [_vp, C.POINTER(PrtFeatureTrace)]),
    "prt_group_set_feature_trace": (C.c_int, [_vp, C.POINTER(PrtFeatureTrace)]),
    "prt_features_read_guide": (C.c_int, [_vp, _fp, _fp, _fp, _fp, C.POINTER(C.c_int32), _u32p]),
    "prt_feature_sampling_defaults": (None, [C.POINTER(PrtFeatureSampling)]),
    "prt_set_feature_sampling": (C.c_int, [_vp, C.POINTER(PrtFeatureSampling)]),
    "prt_get_feature_sampling": (C.c_int, [_vp, C.POINTER(PrtFeatureSampling)]),
    "prt_group_set_feature_sampling": (C.c_int, [_vp, C.POINTER(PrtFeatureSampling)]),
    "prt_features_read_sampled": (C.c_int, [_vp, _fp, _fp, _fp, _fp, C.POINTER(C.c_int32), _u32p]),
    "prt_denoise": (C.c_int, [_vp, C.POINTER(PrtDenoise), C.c_uint32, C.c_uint32, _fp, _fp, _fp, _fp, _fp, C.POINTER(C.c_int32), _fp, _fp]),
    "prt_denoise_device": (C.c_int, [_vp, C.POINTER(PrtDenoise), C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "prt_film_denoise": (C.c_int, [_vp, C.POINTER(PrtDenoise), _fp, _fp]),
    "prt_group_film_denoise": (C.c_int, [_vp, C.POINTER(PrtDenoise), _fp, _fp]),
    "prt_temporal_defaults": (None, [C.POINTER(PrtTemporal)]),
    "prt_get_camera_basis": (C.c_int, [_vp, C.POINTER(PrtCameraBasis)]),
    "prt_temporal_reproject": (C.c_int, [_vp, C.POINTER(PrtTemporal), C.c_uint32, C.c_uint32, C.POINTER(PrtCameraBasis),
                                         _fp, _fp, _fp, _fp, C.POINTER(C.c_int32), _fp, _fp,
                                         _fp, _fp, _fp, _fp, _fp, _fp, C.POINTER(C.c_int32),
                                         _fp, _fp, _fp, _fp, _fp, C.POINTER(C.c_uint8)]),
    "prt_temporal_reproject_device": (C.c_int, [_vp, C.POINTER(PrtTemporal), C.c_uint32, C.c_uint32, C.POINTER(PrtCameraBasis)] + [_vp] * 20),
    "prt_temporal_prev_surface": (C.c_int, [_vp, C.c_uint32, _fp, _fp, C.POINTER(C.c_int32), C.POINTER(PrtInstance), C.c_uint32, _fp, _fp]),
    "prt_film_temporal": (C.c_int, [_vp, C.POINTER(PrtTemporal), C.POINTER(PrtDenoise), _fp, _fp, _fp]),
    "prt_temporal_reset": (C.c_int, [_vp]),
    "prt_temporal_info": (C.c_int, [_vp, C.POINTER(PrtTemporalInfo)]),
    "prt_set_lighting": (C.c_int, [_vp, C.POINTER(PrtLighting)]),
    "prt_get_light_stats": (C.c_int, [_vp, C.POINTER(PrtLightStats)]),
    "prt_light_info": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, _fp]),
    "prt_sample_light": (C.c_int, [_vp, C.c_uint32, _fp, C.POINTER(PrtHit), _u32p, _fp, _fp, _u32p, _fp, _fp, _fp, _fp, _fp]),
    "prt_set_scene": (C.c_int, [_vp, C.POINTER(PrtSceneDesc)]),
    "prt_set_camera": (C.c_int, [_vp, C.POINTER(PrtCameraDesc)]),
    "prt_set_film": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "prt_film_clear": (C.c_int, [_vp]),
    "prt_render": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "prt_render_async": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "prt_synchronize": (C.c_int, [_vp]),
    "prt_set_samples_in_flight": (C.c_int, [_vp, C.c_uint32]),
    "prt_film_read": (C.c_int, [_vp, _fp, _fp]),
    "prt_film_local": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "prt_film_resolve": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp]),
    "prt_film_resolve_on": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp]),
    "prt_film_tonemap": (C.c_int, [_vp, _vp, _vp, C.c_float, C.c_float, _vp]),
    "prt_film_display": (C.c_int, [_vp, C.c_float, C.c_float, C.POINTER(C.c_uint8)]),
    "prt_camera_rays": (C.c_int, [_vp, C.c_uint32, _fp, _fp, _fp, _fp]),
    "prt_closest_hit": (C.c_int, [_vp, C.c_uint32, _fp, _fp, C.POINTER(PrtHit)]),
    "prt_closest_hit_device": (C.c_int, [_vp, C.c_uint32, _vp, _vp, _vp]),
    "prt_occluded": (C.c_int, [_vp, C.c_uint32, _fp, _fp, _fp, C.POINTER(C.c_uint8)]),
    "prt_occluded_device": (C.c_int, [_vp, C.c_uint32, _vp, _vp, _vp, _vp]),
    "prt_scatter": (C.c_int, [_vp, C.c_uint32, _fp, C.POINTER(PrtHit), _u32p, _u32p, _fp, _fp, _fp, _fp]),
    "prt_radiance": (C.c_int, [_vp, C.POINTER(PrtRadianceQuery), C.c_uint32, _fp, _fp, _u32p, _fp, _u32p]),
    "prt_radiance_device": (C.c_int, [_vp, C.POINTER(PrtRadianceQuery), C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "prt_radiance_lit": (C.c_int, [_vp, C.POINTER(PrtRadianceQuery), C.c_uint32, _fp, _fp, _u32p, _fp, _u32p, C.POINTER(PrtRadianceLitInfo)]),
    "prt_radiance_lit_device": (C.c_int, [_vp, C.POINTER(PrtRadianceQuery), C.c_uint32, _vp, _vp, _vp, _vp, _vp,
                                          C.POINTER(PrtRadianceLitInfo)]),
    "prt_radiance_lit_pb": (C.c_int, [_vp, C.POINTER(PrtRadianceQuery), C.c_uint32, _fp, _fp, _u32p, _fp, _fp, _u32p,
                                      C.POINTER(PrtRadianceLitInfo)]),
    "prt_radiance_lit_pb_device": (C.c_int, [_vp, C.POINTER(PrtRadianceQuery), C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp,
                                             C.POINTER(PrtRadianceLitInfo)]),
    "prt_bake_surface": (C.c_int, [_vp, C.POINTER(PrtBakeTarget), _u32p, _fp, _fp, _fp, C.POINTER(PrtBakeInfo)]),
    "prt_bake_rays": (C.c_int, [_vp, C.POINTER(PrtBakeTarget), C.c_uint32, C.c_uint32, _fp, _fp, _u32p]),
    "prt_bake_irradiance": (C.c_int, [_vp, C.POINTER(PrtBakeTarget), C.POINTER(PrtRadianceQuery), C.c_int, C.c_uint32, _fp,
                                      C.POINTER(C.c_uint8), C.POINTER(PrtBakeInfo)]),
    "prt_bake_irradiance_device": (C.c_int, [_vp, C.POINTER(PrtBakeTarget), C.POINTER(PrtRadianceQuery), C.c_int, C.c_uint32, _vp, _vp,
                                             C.POINTER(PrtBakeInfo)]),
    "prt_bake_irradiance_opt": (C.c_int, [_vp, C.POINTER(PrtBakeTarget), C.POINTER(PrtRadianceQuery), C.POINTER(PrtBakeOptions), _fp,
                                          C.POINTER(C.c_uint8), C.POINTER(PrtBakeInfo)]),
    "prt_bake_irradiance_opt_device": (C.c_int, [_vp, C.POINTER(PrtBakeTarget), C.POINTER(PrtRadianceQuery), C.POINTER(PrtBakeOptions),
                                                 _vp, _vp, C.POINTER(PrtBakeInfo)]),
    "prt_bake_light_samples": (C.c_int, [_vp, C.POINTER(PrtBakeTarget), C.c_uint32, C.c_uint32, _fp, _fp, _u32p, _fp, _fp]),
    "prt_bake_irradiance_adaptive": (C.c_int, [_vp, C.POINTER(PrtBakeTarget), C.POINTER(PrtRadianceQuery), C.POINTER(PrtBakeOptions),
                                               C.POINTER(PrtBakeAdaptive), _fp, _fp, _fp, _fp, _fp, C.POINTER(C.c_uint8),
                                               C.POINTER(PrtBakeInfo), C.POINTER(PrtBakeAdaptiveInfo)]),
    "prt_bake_irradiance_adaptive_device": (C.c_int, [_vp, C.POINTER(PrtBakeTarget), C.POINTER(PrtRadianceQuery), C.POINTER(PrtBakeOptions),
                                                      C.POINTER(PrtBakeAdaptive), _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(PrtBakeInfo),
                                                      C.POINTER(PrtBakeAdaptiveInfo)]),
    "prt_bake_block_select": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), _fp, _fp, _fp, _u32p, C.c_uint32, C.c_float,
                                        C.c_float, _u32p, _u32p, _u32p]),
    "prt_bake_noise": (C.c_int, [C.c_uint64, _fp, _fp, _fp, C.c_float, _fp]),
    "prt_probe_sh": (C.c_int, [_vp, C.POINTER(PrtProbeShOptions), C.POINTER(PrtRadianceQuery), C.c_uint32, _fp, _fp,
                               C.POINTER(PrtProbeShInfo)]),
    "prt_probe_sh_device": (C.c_int, [_vp, C.POINTER(PrtProbeShOptions), C.POINTER(PrtRadianceQuery), C.c_uint32, _vp, _vp,
                                      C.POINTER(PrtProbeShInfo)]),
    "prt_probe_sh_rays": (C.c_int, [_vp, C.c_uint32, _fp, C.c_uint32, C.c_uint32, _fp, _fp, _u32p]),
    "prt_sh_eval": (C.c_int, [C.c_uint32, _fp, C.c_uint32, _fp]),
    "prt_sh_irradiance": (C.c_int, [C.c_uint32, _fp, _fp, C.c_uint32, _fp]),
    "prt_enable_timing": (C.c_int, [_vp, C.c_int]),
    "prt_get_stats": (C.c_int, [_vp, C.POINTER(PrtStats)]),
    "prt_reset_stats": (C.c_int, [_vp]),
    "prt_measure_traversal": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PrtStats)]),
    "prt_bvh_info": (C.c_int, [_vp, C.POINTER(PrtBvhInfo)]),
    "prt_spill_rows": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "prt_kernel_occupancy": (C.c_int, [_vp, C.POINTER(PrtOccupancy)]),
    "prt_kernel_instance": (C.c_int, [_vp, C.c_char_p, C.c_uint32]),
    "prt_shade_instance": (C.c_int, [_vp, C.c_char_p, C.c_uint32]),
    "prt_batch_instance": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_uint32]),
    "prt_instance_name": (C.c_int, [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]),
    "prt_last_segment": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "prt_primary_reuse": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "prt_measure_shade_divergence": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "prt_refit_meshes": (C.c_int, [_vp, C.POINTER(PrtMesh), C.c_uint32]),
    "prt_refit_meshes_device": (C.c_int, [_vp, C.POINTER(PrtMeshDeviceArrays), C.c_uint32]),
    "prt_mesh_normals_device": (C.c_int, [_vp, C.c_uint32, _vp, _vp]),
    "prt_refit_info": (C.c_int, [_vp, C.POINTER(PrtRefitInfo)]),
    "prt_set_instance_transforms": (C.c_int, [_vp, C.POINTER(PrtInstance), C.c_uint32, C.c_uint32]),
    "prt_group_set_instance_transforms": (C.c_int, [_vp, C.POINTER(PrtInstance), C.c_uint32, C.c_uint32]),
    "prt_instance_update_info": (C.c_int, [_vp, C.POINTER(PrtInstanceUpdateInfo)]),
    "prt_instances_read": (C.c_int, [_vp, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _u32p]),
    "prt_bvh_read": (C.c_int, [_vp, _fp, _fp]),
    "prt_set_sampling": (C.c_int, [_vp, C.POINTER(PrtSampling)]),
    "prt_bvh_read4": (C.c_int, [_vp, _fp]),
    "prt_bvh_read8": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "prt_set_variant": (C.c_int, [_vp, C.c_int]),
    "prt_set_param": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "prt_mesh_load_ply": (C.c_int, [C.c_char_p, C.POINTER(_vp), C.c_char_p, C.c_size_t]),
    "prt_mesh_create": (C.c_int, [_fp, _fp, C.c_uint32, _u32p, C.c_uint32, C.POINTER(_vp)]),
    "prt_mesh_free": (None, [_vp]),
    "prt_mesh_vertex_count": (C.c_uint32, [_vp]),
    "prt_mesh_triangle_count": (C.c_uint32, [_vp]),
    "prt_mesh_positions": (_fp, [_vp]),
    "prt_mesh_normals": (_fp, [_vp]),
    "prt_mesh_indices": (_u32p, [_vp]),
    "prt_mesh_had_normals": (C.c_int, [_vp]),
    "prt_mesh_refine": (C.c_int, [_vp, C.c_uint32]),
    "prt_mesh_transform": (C.c_int, [_vp, _fp, _fp]),
    "prt_mesh_append": (C.c_int, [_vp, _vp]),
    "prt_scene_preset": (C.c_int, [C.c_int, C.POINTER(PrtMaterial), _u32p, C.POINTER(PrtPrimitive), _u32p]),
    "prt_make_transform": (None, [_fp, _fp, _fp, _fp, _fp]),
    "prt_write_ppm": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32]),
    "prt_write_pfm": (C.c_int, [C.c_char_p, _fp, C.c_uint32, C.c_uint32]),
}


def load(path: str = LIB_PATH) -> C.CDLL:
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP extension is the product and has no fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C parallelraytracing_amd/csrc`).")
    # torch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64; two HIP runtimes in one process do
    # not coexist, so when torch is importable it must load first (libprt.so then binds to the same runtime).
    try:
        import torch  # noqa: F401
    except Exception:  # torch is plumbing only: the library also runs without it (system ROCm runtime)
        pass
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = load()
    return _lib
