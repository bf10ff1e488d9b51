"""ctypes binding of ``libptamd.so`` (C ABI: ``include/pt_api.h``).

Python is plumbing here, not the product: every function below is a thin call into the HIP
library. There is NO CPU fallback — loading fails loudly if the library is missing, and every
render fails loudly without a HIP device.

Mirrors the reference's names where it has them: ``launch_unidirectional`` /
``launch_naive_unidirectional`` (deviceCode.cuh:8-12), ``init_render`` (main.cu:235),
``Camera.Pinhole`` / ``NotPinhole`` (objects.cuh:221-264).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PT_LIB_PATH selects another BUILD of the same HIP library (kernel A/B variants); it is never a fallback.
LIB_PATH = os.environ.get("PT_LIB_PATH") or os.path.join(_HERE, "csrc", "libptamd.so")

UNIDIRECTIONAL = 0
NAIVE_UNIDIRECTIONAL = 2
SEED = 103033  # deviceCode.cu:552
INFO_KEYS = ("width", "height", "spp", "max_depth", "integrator", "leaf_size", "n_tris", "n_lights", "n_nodes",
             "n_points", "n_normals", "n_uvs", "n_mats", "largest_leaf", "backup_count", "tree_depth")
COUNTER_KEYS = ("rays_closest", "rays_shadow", "node_pops", "box_tests", "tri_tests", "hits", "rng_draws", "iterations")


class _F4(C.Union):  # pt_float4: 16 bytes, 16-byte aligned (the long double member only forces the alignment)
    _fields_ = [("v", C.c_float * 4), ("_align", C.c_longdouble)]


class Camera(C.Structure):
    """pt_camera == the reference's Camera (objects.cuh:199-219), 112 bytes."""

    _fields_ = [("cameraOrigin", _F4), ("w", C.c_int32), ("h", C.c_int32), ("xRot", C.c_float), ("yRot", C.c_float),
                ("zRot", C.c_float), ("aperture", C.c_float), ("focalDist", C.c_float), ("fovScale", C.c_float),
                ("antiAliasJitterDist", C.c_float), ("_pad", C.c_float * 3), ("forward", _F4), ("right", _F4), ("up", _F4)]

    @staticmethod
    def Pinhole(pos, w, h, rot=(0.0, 0.0, 0.0), fov=60.0):
        return make_camera(True, pos, rot, fov, w, h)

    @staticmethod
    def NotPinhole(pos, w, h, rot, fov, aperture, focal_dist):
        return make_camera(False, pos, rot, fov, w, h, aperture, focal_dist)

    def tobytes(self):
        return bytes(memoryview(self))

    @staticmethod
    def frombytes(b):
        return Camera.from_buffer_copy(bytes(b))


assert C.sizeof(Camera) == 112 and C.alignment(Camera) == 16


class SceneDesc(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("n_positions", C.c_int32), ("normals", C.c_void_p), ("n_normals", C.c_int32),
                ("uvs", C.c_void_p), ("n_uvs", C.c_int32), ("triangles", C.c_void_p), ("n_triangles", C.c_int32),
                ("lights", C.c_void_p), ("n_lights", C.c_int32), ("bvh", C.c_void_p), ("n_nodes", C.c_int32),
                ("bvh_indices", C.c_void_p), ("materials", C.c_void_p), ("n_materials", C.c_int32),
                ("textures", C.c_void_p), ("n_texels", C.c_int32)]


class TileRange(C.Structure):
    _fields_ = [("first", C.c_int32), ("stride", C.c_int32), ("count", C.c_int32)]


class DenoiseParams(C.Structure):    # pt_denoise_params
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


class DenoiseVarParams(C.Structure):  # pt_denoise_var_params
    _fields_ = [("iterations", C.c_int32), ("sigma_var", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


class TemporalParams(C.Structure):   # pt_temporal_params
    _fields_ = [("max_history", C.c_int32), ("depth_tol", C.c_float), ("normal_tol", C.c_float)]


class RespondParams(C.Structure):    # pt_respond_params
    _fields_ = [("radius", C.c_int32), ("power", C.c_int32), ("threshold", C.c_float)]


class UpsampleParams(C.Structure):   # pt_upsample_params
    _fields_ = [("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


class ResolveParams(C.Structure):    # pt_resolve_params
    _fields_ = [("tonemap", C.c_int32), ("exposure", C.c_float)]


class SelectEntry(C.Structure):      # pt_select_entry
    _fields_ = [("component", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("colour", C.c_uint8 * 4), ("radius", C.c_int32),
                ("fill_alpha", C.c_int32)]


class Ray(C.Structure):              # pt_ray
    _fields_ = [("ox", C.c_float), ("oy", C.c_float), ("oz", C.c_float), ("max_t", C.c_float), ("dx", C.c_float), ("dy", C.c_float),
                ("dz", C.c_float), ("pad", C.c_uint32)]


class RayHit(C.Structure):           # pt_ray_hit
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("tri", C.c_int32)]


class RaySurface(C.Structure):       # pt_ray_surface
    _fields_ = [("px", C.c_float), ("py", C.c_float), ("pz", C.c_float), ("uvx", C.c_float), ("nx", C.c_float), ("ny", C.c_float),
                ("nz", C.c_float), ("uvy", C.c_float), ("material", C.c_int32), ("light", C.c_int32), ("backface", C.c_int32), ("pad", C.c_int32)]


def _record_dtype(struct):
    return np.dtype({"names": [f[0] for f in struct._fields_], "formats": [np.dtype(f[1]) for f in struct._fields_],
                     "offsets": [getattr(struct, f[0]).offset for f in struct._fields_], "itemsize": C.sizeof(struct)})


RAY_DTYPE, RAY_HIT_DTYPE, RAY_SURFACE_DTYPE = _record_dtype(Ray), _record_dtype(RayHit), _record_dtype(RaySurface)
_F4 = (4, np.float32)                # Scene._query's output of four floats per ray
QUERY_REORDER = 1                    # PT_QUERY_REORDER
QUERY_STREAM_PAD = 2                 # PT_QUERY_STREAM_PAD
QUERY_TEXEL_CENTRE = 4               # PT_QUERY_TEXEL_CENTRE
QUERY_MAX_T = 999999.0               # the max_t of the library's own closest-hit rays
PROBE_INSIDE = 1                     # PT_PROBE_INSIDE: the probe lies inside an object, lookups with states skip it
PROBE_IDLE = 2                       # PT_PROBE_IDLE: no surface within the maps' max_t


class GridDesc(C.Structure):         # pt_grid_desc
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("counts", C.c_int32 * 3), ("sh_samples", C.c_int32), ("map_res", C.c_int32),
                ("map_samples", C.c_int32), ("power", C.c_int32)]


class PreviewParams(C.Structure):    # pt_preview_params
    _fields_ = [("spp", C.c_int32), ("batches", C.c_int32), ("max_depth", C.c_int32), ("integrator", C.c_int32), ("use_mis", C.c_int32),
                ("aov_spp", C.c_int32), ("temporal", C.c_int32), ("filter", C.c_int32), ("temporal_params", TemporalParams),
                ("filter_params", DenoiseVarParams), ("resolve_params", ResolveParams)]


class PreviewStats(C.Structure):     # pt_preview_stats
    _fields_ = [("frames", C.c_int32), ("render_ms", C.c_float), ("aov_ms", C.c_float), ("accumulate_ms", C.c_float),
                ("filter_ms", C.c_float), ("resolve_ms", C.c_float), ("total_ms", C.c_float)]


class ConvergeParams(C.Structure):   # pt_converge_params
    _fields_ = [("threshold", C.c_float), ("min_history", C.c_int32)]


class AdaptiveParams(C.Structure):  # pt_adaptive_params
    _fields_ = [("min_spp", C.c_int32), ("max_spp", C.c_int32), ("chunk_spp", C.c_int32), ("threshold", C.c_float)]


class AdaptiveStats(C.Structure):   # pt_adaptive_stats
    _fields_ = [("rounds", C.c_int32), ("tiles_at_max", C.c_int32), ("pixel_samples", C.c_longlong)]


PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_int, C.c_void_p)      # pt_progress_fn


class PtError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libptamd.so; raise if it was not built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PtError("%s is missing: build it with `make -C cudapathtracer_amd/csrc` (or __graft_entry__.build()); "
                      "this package has no CPU fallback" % LIB_PATH)
    # One HIP runtime per process: torch ships its own libamdhip64 / libhsa-runtime64, and whichever of
    # two copies initialises second finds "no ROCm-capable device". With torch loaded first, libptamd's
    # DT_NEEDED libamdhip64.so.7 resolves to the copy already in the process. (A C/C++ host that does
    # not use torch links the system ROCm only and has no such issue.)
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, i32, u64, f32 = C.c_void_p, C.c_int, C.c_uint64, C.c_float
    L.pt_api_version.restype = i32
    L.pt_last_error.restype = C.c_char_p
    L.pt_device_count.restype = i32
    L.pt_scene_create.restype = vp; L.pt_scene_create.argtypes = [C.POINTER(SceneDesc)]
    L.pt_scene_create_from_mesh.restype = vp; L.pt_scene_create_from_mesh.argtypes = [C.POINTER(SceneDesc), i32, vp]
    L.pt_debug_packed.argtypes = [vp, i32, vp, C.c_size_t]
    L.pt_scene_update_mesh.argtypes = [vp, C.POINTER(SceneDesc), i32, vp]
    L.pt_scene_update_vertices.argtypes = [vp, vp, i32, vp, i32, vp]
    L.pt_scene_update_vertices_device.argtypes = [vp, vp, i32, vp, i32, vp]
    L.pt_scene_generation.argtypes = [vp]
    L.pt_scene_update_materials.argtypes = [vp, vp, i32]
    L.pt_scene_update_emission.argtypes = [vp, i32, vp, vp]
    L.pt_scene_has_motion.argtypes = [vp]
    L.pt_render_motion.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, vp, vp]
    L.pt_render_motion_device.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, vp, vp, vp]
    L.pt_render_motion_chain.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, vp, vp, vp, vp]
    L.pt_render_motion_chain_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, vp, vp, vp, vp, vp]
    L.pt_temporal_accumulate_motion.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp,
                                                C.POINTER(TemporalParams), vp, vp]
    L.pt_temporal_accumulate_motion_device.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp,
                                                       C.POINTER(TemporalParams), vp, vp, vp]
    L.pt_temporal_accumulate_cur_motion.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, vp, vp, vp, vp,
                                                    C.POINTER(TemporalParams), vp, vp]
    L.pt_temporal_accumulate_cur_motion_device.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, vp, vp, vp, vp,
                                                           C.POINTER(TemporalParams), vp, vp, vp]
    L.pt_respond_defaults.restype = None; L.pt_respond_defaults.argtypes = [C.POINTER(RespondParams)]
    L.pt_temporal_respond_workspace_bytes.restype = C.c_size_t; L.pt_temporal_respond_workspace_bytes.argtypes = [i32, i32]
    L.pt_temporal_accumulate_respond.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp,
                                                 C.POINTER(TemporalParams), C.POINTER(RespondParams), vp, vp, vp]
    L.pt_temporal_accumulate_respond_device.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp,
                                                        C.POINTER(TemporalParams), C.POINTER(RespondParams), vp, vp, vp, vp, vp]
    L.pt_preview_set_respond.argtypes = [vp, C.POINTER(RespondParams)]
    L.pt_preview_respond.argtypes = [vp, C.POINTER(RespondParams)]
    L.pt_preview_set_motion.argtypes = [vp, i32]
    L.pt_preview_motion.argtypes = [vp]
    L.pt_preview_set_motion_chain.argtypes = [vp, i32]
    L.pt_preview_motion_chain.argtypes = [vp]
    L.pt_render_ids.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, vp]
    L.pt_render_ids_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, vp, vp]
    L.pt_pick.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, vp, i32, vp, vp]
    L.pt_select_overlay.argtypes = [i32, i32, vp, i32, C.POINTER(SelectEntry), vp]
    L.pt_select_overlay_device.argtypes = [i32, i32, vp, i32, C.POINTER(SelectEntry), vp, vp]
    L.pt_preview_set_selection.argtypes = [vp, i32, C.POINTER(SelectEntry), i32]
    L.pt_preview_pick.argtypes = [vp, i32, i32, i32, vp, vp]
    L.pt_preview_read_ids.argtypes = [vp, vp]
    L.pt_preview_device_ids.restype = vp; L.pt_preview_device_ids.argtypes = [vp]
    L.pt_preview_id_passes.argtypes = [vp]
    L.pt_query_closest.argtypes = [vp, i32, vp, vp, vp, C.c_uint32]
    L.pt_query_closest_device.argtypes = [vp, i32, vp, vp, vp, C.c_uint32, vp]
    L.pt_query_shadow.argtypes = [vp, i32, vp, vp, C.c_uint32]
    L.pt_query_shadow_device.argtypes = [vp, i32, vp, vp, C.c_uint32, vp]
    L.pt_query_camera_rays_device.argtypes = [C.POINTER(Camera), i32, i32, f32, vp, vp]
    L.pt_query_radiance.argtypes = [vp, i32, vp, i32, i32, i32, i32, C.c_uint64, C.c_uint32, vp, C.c_uint32]
    L.pt_query_radiance_device.argtypes = [vp, i32, vp, i32, i32, i32, i32, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp]
    L.pt_query_radiance_moments.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32]
    L.pt_query_radiance_moments_device.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.pt_query_irradiance.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32]
    L.pt_query_irradiance_device.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.pt_query_irradiance_rays_device.argtypes = [vp, i32, vp, i32, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.pt_query_sh_workspace_bytes.restype = C.c_size_t; L.pt_query_sh_workspace_bytes.argtypes = [i32, i32]
    L.pt_query_sh.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, C.c_uint64, C.c_uint32, vp, C.c_uint32]
    L.pt_query_sh_device.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.pt_query_sh_rays_device.argtypes = [vp, i32, vp, i32, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.pt_query_distance.argtypes = [vp, i32, vp, i32, i32, C.c_uint64, C.c_uint32, vp, C.c_uint32]
    L.pt_query_distance_device.argtypes = [vp, i32, vp, i32, i32, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp]
    L.pt_query_distance_rays_device.argtypes = [vp, i32, vp, i32, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, vp]
    L.pt_grid_packed_bytes.restype = C.c_size_t; L.pt_grid_packed_bytes.argtypes = [C.POINTER(GridDesc)]
    L.pt_grid_pack.argtypes = [C.POINTER(GridDesc), vp, vp, vp]
    L.pt_grid_pack_device.argtypes = [C.POINTER(GridDesc), vp, vp, vp, vp]
    L.pt_grid_irradiance.argtypes = [C.POINTER(GridDesc), vp, i32, vp, vp]
    L.pt_grid_irradiance_device.argtypes = [C.POINTER(GridDesc), vp, i32, vp, vp, vp]
    L.pt_grid_classify.argtypes = [C.POINTER(GridDesc), i32, vp, vp, f32, vp]
    L.pt_grid_classify_device.argtypes = [C.POINTER(GridDesc), i32, vp, vp, f32, vp, vp]
    L.pt_grid_update.argtypes = [C.POINTER(GridDesc), i32, vp, vp, vp, f32, vp]
    L.pt_grid_update_device.argtypes = [C.POINTER(GridDesc), i32, vp, vp, vp, f32, vp, vp]
    L.pt_grid_irradiance_states.argtypes = [C.POINTER(GridDesc), vp, vp, i32, vp, vp]
    L.pt_grid_irradiance_states_device.argtypes = [C.POINTER(GridDesc), vp, vp, i32, vp, vp, vp]
    L.pt_grid_relocate.argtypes = [C.POINTER(GridDesc), i32, vp, vp, f32, f32, vp, vp]
    L.pt_grid_relocate_device.argtypes = [C.POINTER(GridDesc), i32, vp, vp, f32, f32, vp, vp, vp]
    L.pt_grid_irradiance_offsets.argtypes = [C.POINTER(GridDesc), vp, vp, vp, i32, vp, vp]
    L.pt_grid_irradiance_offsets_device.argtypes = [C.POINTER(GridDesc), vp, vp, vp, i32, vp, vp, vp]
    L.pt_query_guides.argtypes = [vp, i32, vp, i32, vp, vp, vp, C.c_uint32]
    L.pt_query_guides_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, C.c_uint32, vp]
    L.pt_debug_update_ms.argtypes = [vp, vp]
    L.pt_light_triangles.argtypes = [C.POINTER(SceneDesc), vp]
    L.pt_scene_destroy.argtypes = [vp]
    L.pt_render.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, u64, C.POINTER(TileRange), vp]
    L.pt_render_counted.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, u64, C.POINTER(TileRange), vp, vp]
    L.pt_render_tiles_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, u64, C.POINTER(TileRange), vp, i32, vp]
    L.pt_untile_device.argtypes = [i32, i32, C.POINTER(TileRange), vp, vp, vp]
    L.pt_tile_device.argtypes = [i32, i32, C.POINTER(TileRange), vp, vp, vp]
    L.pt_launch_unidirectional.argtypes = [i32, Camera, vp, i32, i32, i32, i32, vp]
    L.pt_launch_naive_unidirectional.argtypes = [i32, Camera, vp, i32, i32, i32, i32, vp]
    L.pt_set_variant.argtypes = [vp, i32]
    L.pt_has_experimental.restype = i32
    L.pt_get_counters.argtypes = [vp, vp]
    L.pt_reset_counters.argtypes = [vp]
    L.pt_last_kernel_ms.restype = f32; L.pt_last_kernel_ms.argtypes = [vp]
    L.pt_scene_flags.argtypes = [vp]
    L.pt_last_tile_handovers.argtypes = [vp]
    L.pt_last_moments_launches.argtypes = [vp]
    L.pt_queue_stalls.argtypes = [vp]
    L.pt_debug_queue_header.argtypes = [vp, C.POINTER(C.c_int)]
    L.pt_set_culling.argtypes = [vp, i32]
    L.pt_set_option.argtypes = [vp, C.c_char_p, i32]
    L.pt_get_option.argtypes = [vp, C.c_char_p, vp]
    L.pt_debug_stamps.argtypes = [vp, vp]
    L.pt_rank_tiles.argtypes = [i32, i32, i32, i32, C.POINTER(TileRange)]
    L.pt_multi_create.restype = vp; L.pt_multi_create.argtypes = [C.POINTER(SceneDesc), i32, vp]
    L.pt_multi_destroy.argtypes = [vp]
    L.pt_multi_set_option.argtypes = [vp, C.c_char_p, i32]
    L.pt_multi_set_variant.argtypes = [vp, i32]
    L.pt_multi_render.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, u64, vp, vp]
    L.pt_render_multi.argtypes = [C.POINTER(SceneDesc), i32, vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, u64, vp, vp]
    L.pt_probe_rng.argtypes = [u64, i32, vp, i32, vp, vp, vp]
    L.pt_probe_math.argtypes = [i32, vp, vp, vp, vp, vp, vp]
    L.pt_probe_rcp_exhaustive.argtypes = [vp, vp]
    L.pt_probe_camera_rays.argtypes = [C.POINTER(Camera), u64, i32, vp, vp]
    L.pt_probe_trace_closest.argtypes = [vp, i32, vp, vp, vp, vp]
    L.pt_probe_trace_shadow.argtypes = [vp, i32, vp, vp, vp, vp]
    L.pt_probe_bsdf_sample.argtypes = [vp, i32, vp, vp, vp, f32, f32, u64, vp, vp]
    L.pt_probe_bsdf_eval.argtypes = [vp, i32, vp, vp, vp, f32, f32, vp]
    L.novum_scene_load.restype = vp; L.novum_scene_load.argtypes = [C.c_char_p, C.c_char_p, i32]
    L.novum_scene_load_ex.restype = vp; L.novum_scene_load_ex.argtypes = [C.c_char_p, C.c_char_p, i32, i32]
    L.pt_bvh_build_device.argtypes = [vp, i32, vp, i32, i32, i32, vp, i32, vp, vp]
    L.novum_bvh_build_host.argtypes = [vp, i32, vp, i32, i32, vp, i32, vp, vp]
    L.novum_scene_free.argtypes = [vp]
    L.novum_scene_info.argtypes = [vp, vp]
    L.novum_scene_desc.argtypes = [vp, C.POINTER(SceneDesc)]
    L.novum_scene_camera.argtypes = [vp, C.POINTER(Camera)]
    L.novum_make_camera.argtypes = [i32, vp, vp, f32, f32, f32, i32, i32, C.POINTER(Camera)]
    L.novum_finalise.argtypes = [vp, i32, i32]
    L.novum_init_render.argtypes = [C.c_char_p, C.c_char_p, i32, vp, C.c_char_p]
    L.novum_init_render_progressive.argtypes = [C.c_char_p, C.c_char_p, i32, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_double, i32]
    L.novum_save_csv_mono.argtypes = [C.c_char_p, vp, i32, i32, i32]
    L.pt_launch_progressive.argtypes = [i32, i32, Camera, vp, i32, i32, i32, i32, vp, i32, PROGRESS_FN, vp]
    L.novum_save_bmp.argtypes = [C.c_char_p, vp, i32, i32, i32]
    L.pt_render_aovs.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, u64, vp, vp]
    L.pt_render_aovs_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, u64, vp, vp, vp]
    L.pt_render_aovs_chain.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, u64, vp, vp, vp]
    L.pt_render_aovs_chain_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, u64, vp, vp, vp, vp]
    L.pt_render_aovs_centre.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, vp, vp, vp]
    L.pt_render_aovs_centre_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, vp, vp, vp, vp]
    L.pt_probe_centre_rays.argtypes = [C.POINTER(Camera), i32, vp, vp]
    L.pt_denoise_defaults.restype = None; L.pt_denoise_defaults.argtypes = [C.POINTER(DenoiseParams)]
    L.pt_denoise_workspace_bytes.restype = C.c_size_t; L.pt_denoise_workspace_bytes.argtypes = [i32, i32]
    L.pt_denoise.argtypes = [i32, i32, vp, i32, vp, vp, C.POINTER(DenoiseParams), vp]
    L.pt_denoise_device.argtypes = [i32, i32, vp, i32, vp, vp, C.POINTER(DenoiseParams), vp, vp, vp]
    L.pt_render_adaptive.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, u64, C.POINTER(AdaptiveParams), vp, vp, vp,
                                     C.POINTER(AdaptiveStats)]
    L.pt_render_adaptive_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, u64, C.POINTER(AdaptiveParams), vp, vp, vp,
                                            C.POINTER(AdaptiveStats), vp]
    L.pt_render_moments.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, u64, vp, vp]
    L.pt_render_moments_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, u64, vp, vp, vp]
    L.pt_denoise_var_defaults.restype = None; L.pt_denoise_var_defaults.argtypes = [C.POINTER(DenoiseVarParams)]
    L.pt_denoise_var_workspace_bytes.restype = C.c_size_t; L.pt_denoise_var_workspace_bytes.argtypes = [i32, i32]
    L.pt_denoise_var.argtypes = [i32, i32, vp, vp, i32, i32, vp, vp, C.POINTER(DenoiseVarParams), vp]
    L.pt_denoise_var_device.argtypes = [i32, i32, vp, vp, i32, i32, vp, vp, C.POINTER(DenoiseVarParams), vp, vp, vp]
    L.pt_temporal_defaults.restype = None; L.pt_temporal_defaults.argtypes = [C.POINTER(TemporalParams)]
    L.pt_temporal_accumulate.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, i32, i32, vp, vp, vp, vp, vp,
                                         C.POINTER(TemporalParams), vp, vp]
    L.pt_temporal_accumulate_device.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, i32, i32, vp, vp, vp, vp, vp,
                                                C.POINTER(TemporalParams), vp, vp, vp]
    L.pt_denoise_hist_workspace_bytes.restype = C.c_size_t; L.pt_denoise_hist_workspace_bytes.argtypes = [i32, i32]
    L.pt_denoise_hist.argtypes = [i32, i32, vp, vp, vp, C.POINTER(DenoiseVarParams), vp]
    L.pt_denoise_hist_device.argtypes = [i32, i32, vp, vp, vp, C.POINTER(DenoiseVarParams), vp, vp, vp]
    L.pt_upsample_defaults.restype = None; L.pt_upsample_defaults.argtypes = [C.POINTER(UpsampleParams)]
    L.pt_camera_scaled.argtypes = [C.POINTER(Camera), i32, C.POINTER(Camera)]
    L.pt_upsample.argtypes = [i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, C.POINTER(UpsampleParams), vp]
    L.pt_upsample_device.argtypes = [i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, C.POINTER(UpsampleParams), vp, vp]
    L.pt_guide_subsample.argtypes = [i32, i32, i32, vp, vp, vp, vp]
    L.pt_guide_subsample_device.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
    L.pt_temporal_accumulate_cur.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, vp, vp, vp, C.POINTER(TemporalParams), vp, vp]
    L.pt_temporal_accumulate_cur_device.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, vp, vp, vp, C.POINTER(TemporalParams),
                                                    vp, vp, vp]
    L.pt_resolve_defaults.restype = None; L.pt_resolve_defaults.argtypes = [C.POINTER(ResolveParams)]
    L.pt_resolve.argtypes = [i32, i32, vp, i32, vp, C.POINTER(ResolveParams), vp, vp]
    L.pt_resolve_device.argtypes = [i32, i32, vp, i32, vp, C.POINTER(ResolveParams), vp, vp, vp]
    L.pt_preview_defaults.restype = None; L.pt_preview_defaults.argtypes = [C.POINTER(PreviewParams)]
    L.pt_preview_create.restype = vp; L.pt_preview_create.argtypes = [vp, i32, i32, C.POINTER(PreviewParams)]
    L.pt_preview_frame.argtypes = [vp, C.POINTER(Camera), u64]
    L.pt_preview_reset.argtypes = [vp]
    L.pt_preview_scene_changed.argtypes = [vp, i32]
    L.pt_preview_set_scale.argtypes = [vp, i32]
    L.pt_preview_scale.argtypes = [vp]
    L.pt_preview_set_guide_chain.argtypes = [vp, i32]
    L.pt_preview_guide_chain.argtypes = [vp]
    L.pt_preview_set_guide_centre.argtypes = [vp, i32]
    L.pt_preview_guide_centre.argtypes = [vp]
    L.pt_preview_guide_passes.argtypes = [vp]
    L.pt_preview_read.argtypes = [vp, vp, vp, vp, vp]
    L.pt_preview_device_rgba8.restype = vp; L.pt_preview_device_rgba8.argtypes = [vp]
    L.pt_preview_device_mean.restype = vp; L.pt_preview_device_mean.argtypes = [vp]
    L.pt_preview_last_stats.argtypes = [vp, C.POINTER(PreviewStats)]
    L.pt_preview_destroy.restype = None; L.pt_preview_destroy.argtypes = [vp]
    L.pt_converge_defaults.restype = None; L.pt_converge_defaults.argtypes = [C.POINTER(ConvergeParams)]
    L.pt_temporal_select.argtypes = [i32, i32, vp, vp, C.POINTER(ConvergeParams), vp, vp, vp, vp]
    L.pt_temporal_select_device.argtypes = [i32, i32, vp, vp, C.POINTER(ConvergeParams), vp, vp, vp, vp, vp]
    L.pt_render_moments_tiles.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, u64, vp, i32, vp, vp]
    L.pt_render_moments_tiles_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, i32, i32, u64, vp, i32, vp, vp, vp]
    L.pt_temporal_accumulate_live.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp,
                                              C.POINTER(TemporalParams), vp, vp]
    L.pt_temporal_accumulate_live_device.argtypes = [i32, i32, C.POINTER(Camera), C.POINTER(Camera), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp,
                                                     C.POINTER(TemporalParams), vp, vp, vp]
    L.pt_preview_set_converge.argtypes = [vp, C.POINTER(ConvergeParams)]
    L.pt_preview_last_live.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pt_preview_read_tiles.argtypes = [vp, vp, vp]
    L.pt_render_adaptive_moments.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, u64, C.POINTER(AdaptiveParams), vp, vp, vp, vp,
                                             C.POINTER(AdaptiveStats)]
    L.pt_render_adaptive_moments_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, u64, C.POINTER(AdaptiveParams), vp, vp, vp,
                                                    vp, C.POINTER(AdaptiveStats), vp]
    L.pt_probe_adaptive_moments.argtypes = [i32, i32, i32, i32, vp]
    L.pt_denoise_var_tiles_workspace_bytes.restype = C.c_size_t; L.pt_denoise_var_tiles_workspace_bytes.argtypes = [i32, i32]
    L.pt_denoise_var_tiles.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp, C.POINTER(DenoiseVarParams), vp]
    L.pt_denoise_var_tiles_device.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp, C.POINTER(DenoiseVarParams), vp, vp, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _check(rc, what):
    if rc != 0:
        raise PtError("%s failed (%d): %s" % (what, rc, lib().pt_last_error().decode(errors="replace")))


def has_experimental():
    """Always False: the A/B variants of DESIGN.md §6 (options wide, compact, spec, defer_shadow, xcd_bands, refill = 2) were
    removed, and the library refuses those options with -3. Kept for callers that ask."""
    return bool(lib().pt_has_experimental())


def device_count():
    return lib().pt_device_count()


def make_camera(pinhole, pos, rot, fov, w, h, aperture=0.0, focal_dist=0.0):
    cam = Camera()
    pos = np.ascontiguousarray(pos, np.float32); rot = np.ascontiguousarray(rot, np.float32)
    lib().novum_make_camera(int(pinhole), _p(pos), _p(rot), fov, aperture, focal_dist, w, h, C.byref(cam))
    return cam


def finalise(rgba_sum, spp):
    """main.cu:860-870: divide by spp, NaN -> (1,0,1), Inf -> (0,1,0)."""
    out = np.ascontiguousarray(rgba_sum, np.float32).copy()
    lib().novum_finalise(_p(out), out.size // 4, spp)
    return out


def save_bmp(path, rgba, post_process=True):
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    if lib().novum_save_bmp(path.encode(), _p(rgba), w, h, int(post_process)) != 0:
        raise PtError("could not write " + path)


def save_csv_mono(path, rgba, channel=0):
    """Image::saveImageCSV_MONO(channel) (imageUtil.cu:123-142)."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    if lib().novum_save_csv_mono(path.encode(), _p(rgba), w, h, int(channel)) != 0:
        raise PtError("could not write " + path)


def init_render(config_path, render_number=0, base_dir=None, bmp_path=None, preview_bmp=None, preview_csv=None,
                interval_seconds=5.0, chunk_spp=0):
    """initRender (main.cu:235-923) for the unidirectional integrators; returns finalised [h,w,4].
    With chunk_spp > 0 and a preview path it also writes the reference's progressive preview
    (render.bmp / renderCSV.csv every interval_seconds, deviceCode.cu:574-604)."""
    hs = HostScene(config_path, base_dir, render_number)
    w, h = hs.info["width"], hs.info["height"]
    hs.close()
    out = np.zeros((h, w, 4), np.float32)
    enc = lambda s: s.encode() if s else None
    rc = lib().novum_init_render_progressive(config_path.encode(), enc(base_dir), render_number, _p(out), enc(bmp_path),
                                             enc(preview_bmp), enc(preview_csv), float(interval_seconds), int(chunk_spp))
    _check(rc, "novum_init_render")
    return out


BUILD_STATS = np.dtype([("n_nodes", "i4"), ("largest_leaf", "i4"), ("backups", "i4"), ("depth", "i4"), ("sort_fallbacks", "i4"),
                        ("levels", "i4"), ("device_ms", "f4"), ("total_ms", "f4")])


def build_bvh(points, mesh, max_leaf_size, where="device"):
    """buildBVH (main.cu:20-233) on raw arrays in the reference's layouts: `points` float4[n] bytes,
    `mesh` Triangle (80 B)[n] bytes. where="device": pt_bvh_build_device (reference-tree
    mode); where="host": the kept host builder. Returns (nodes uint8[48*n_nodes], indices int32[n], stats dict)."""
    pts = np.ascontiguousarray(points).view(np.uint8).reshape(-1)
    m = np.ascontiguousarray(mesh).view(np.uint8).reshape(-1)
    n = m.size // 80
    cap = max(2 * n - 1, 1)
    nodes = np.zeros(cap * 48, np.uint8)
    idx = np.zeros(max(n, 1), np.int32)
    st = np.zeros(1, BUILD_STATS)
    if where == "device":
        k = lib().pt_bvh_build_device(_p(pts), pts.size // 16, _p(m), n, int(max_leaf_size), 0, _p(nodes), cap, _p(idx), _p(st))
        if k <= 0:
            raise PtError("pt_bvh_build_device failed (%d): %s" % (k, lib().pt_last_error().decode(errors="replace")))
    else:
        k = lib().novum_bvh_build_host(_p(pts), pts.size // 16, _p(m), n, int(max_leaf_size), _p(nodes), cap, _p(idx), _p(st))
        if k <= 0:
            raise PtError("novum_bvh_build_host failed (%d)" % k)
    return nodes[:k * 48].copy(), idx[:n], {f: st[0][f].item() for f in BUILD_STATS.names}


class HostScene:
    """What the kept scene loader produces (novum_scene_load): host arrays in the reference's data model."""

    _ARRAYS = {"points": ("positions", "n_positions", 16), "normals": ("normals", "n_normals", 16), "uvs": ("uvs", "n_uvs", 8),
               "mesh": ("triangles", "n_triangles", 80), "lights": ("lights", "n_lights", 80), "bvh": ("bvh", "n_nodes", 48),
               "indices": ("bvh_indices", "n_triangles", 4), "materials": ("materials", "n_materials", 176),
               "textures": ("textures", "n_texels", 16)}

    def __init__(self, config_path, base_dir=None, render_number=0, bvh_builder="host"):
        """bvh_builder: "host" (the reference's buildBVH on the CPU) or "device" (pt_bvh_build_device; same arrays)."""
        self.h = lib().novum_scene_load_ex(config_path.encode(), base_dir.encode() if base_dir else None, render_number,
                                           {"host": 0, "device": 1}[bvh_builder])
        if not self.h:
            raise PtError("novum_scene_load failed for %s: %s" % (config_path, lib().pt_last_error().decode(errors="replace")))
        info = np.zeros(16, np.int32)
        lib().novum_scene_info(self.h, _p(info))
        self.info = dict(zip(INFO_KEYS, (int(v) for v in info)))
        self.desc = SceneDesc()
        lib().novum_scene_desc(self.h, C.byref(self.desc))

    def camera(self):
        cam = Camera()
        lib().novum_scene_camera(self.h, C.byref(cam))
        return cam

    def array(self, what):
        field, count, size = self._ARRAYS[what]
        n = getattr(self.desc, count) * size
        ptr = getattr(self.desc, field)
        if not ptr or n == 0:
            return np.zeros(0, np.uint8)
        return np.frombuffer((C.c_uint8 * n).from_address(ptr), np.uint8).copy()

    def close(self):
        if self.h:
            lib().novum_scene_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _desc_from_arrays(arrays):
    """SceneDesc over arrays in the reference's layouts; the second value keeps the buffers it points into alive."""
    a = {k: np.ascontiguousarray(v).view(np.uint8) for k, v in arrays.items()}
    d = SceneDesc()
    d.positions, d.n_positions = a["points"].ctypes.data, a["points"].size // 16
    d.normals, d.n_normals = a["normals"].ctypes.data, a["normals"].size // 16
    d.uvs, d.n_uvs = a["uvs"].ctypes.data, a["uvs"].size // 8
    d.triangles, d.n_triangles = a["mesh"].ctypes.data, a["mesh"].size // 80
    d.lights, d.n_lights = (a["lights"].ctypes.data if a["lights"].size else None), a["lights"].size // 80
    if "bvh" in a:                    # (the device builder reads neither: from_mesh / update_mesh take arrays without a tree)
        d.bvh, d.n_nodes = a["bvh"].ctypes.data, a["bvh"].size // 48
        d.bvh_indices = a["indices"].ctypes.data
    d.materials, d.n_materials = a["materials"].ctypes.data, a["materials"].size // 176
    t = a.get("textures")
    d.textures, d.n_texels = (t.ctypes.data if t is not None and t.size else None), (t.size // 16 if t is not None else 0)
    return d, a


def light_triangles(host=None, arrays=None):
    """pt_light_triangles (host only): per light the packed (leaf-order) triangle it was made from, or -1."""
    if host is not None:
        d, keep = host.desc, host
    else:
        d, keep = _desc_from_arrays(arrays)
    out = np.full(max(d.n_lights, 1), -1, np.int32)
    _check(lib().pt_light_triangles(C.byref(d), _p(out)), "pt_light_triangles")
    del keep
    return out[:d.n_lights]


class Scene:
    """Device-resident, re-packed scene (pt_scene). Created on the CURRENT HIP device."""

    def __init__(self, host: HostScene | None = None, desc: SceneDesc | None = None, options: dict | None = None):
        d = host.desc if host is not None else desc
        self.h = lib().pt_scene_create(C.byref(d))
        if not self.h:
            raise PtError("pt_scene_create failed: " + lib().pt_last_error().decode(errors="replace"))
        self.set_options(options)

    def set_option(self, name, value):
        """pt_set_option: kernel-selection / scheduling options by name (include/pt_api.h lists them)."""
        _check(lib().pt_set_option(self.h, name.encode(), int(value)), "pt_set_option(%s)" % name)
        return self

    def set_options(self, options):
        for k, v in (options or {}).items():
            self.set_option(k, v)
        return self

    def get_option(self, name):
        out = np.zeros(1, np.int32)
        _check(lib().pt_get_option(self.h, name.encode(), _p(out)), "pt_get_option(%s)" % name)
        return int(out[0])

    @staticmethod
    def _mesh_desc(host_or_desc, max_leaf_size):
        """(SceneDesc, what keeps its arrays alive, leaf size) of a HostScene, a SceneDesc or a dict of arrays in the reference's
        layouts (points, normals, uvs, mesh, lights, materials[, textures]; a tree is not needed). A HostScene brings its config's
        leaf size; the other two need max_leaf_size."""
        if isinstance(host_or_desc, HostScene):
            return host_or_desc.desc, host_or_desc, host_or_desc.info["leaf_size"] if max_leaf_size is None else int(max_leaf_size)
        if max_leaf_size is None:
            raise PtError("max_leaf_size is needed with a SceneDesc or a dict of arrays (only a HostScene knows its config's)")
        if isinstance(host_or_desc, SceneDesc):
            return host_or_desc, host_or_desc, int(max_leaf_size)
        d, keep = _desc_from_arrays(host_or_desc)
        return d, keep, int(max_leaf_size)

    @staticmethod
    def from_mesh(host: "HostScene", max_leaf_size=None, options=None):
        """pt_scene_create_from_mesh: BVH build (reference tree) and re-layout on the device from the host scene's
        geometry; its host-built tree is not used. `host` may also be a SceneDesc or a dict of arrays (then with
        max_leaf_size). Returns the scene; `.build_stats` has the builder's numbers."""
        st = np.zeros(1, BUILD_STATS)
        d, keep, leaf = Scene._mesh_desc(host, max_leaf_size)
        h = lib().pt_scene_create_from_mesh(C.byref(d), leaf, _p(st))
        if not h:
            raise PtError("pt_scene_create_from_mesh failed: " + lib().pt_last_error().decode(errors="replace"))
        sc = Scene.__new__(Scene)
        sc.h = h; sc._keep = host
        sc.set_options(options)
        sc.build_stats = {f: st[0][f].item() for f in BUILD_STATS.names}
        del keep
        return sc

    def update_mesh(self, host_or_desc, max_leaf_size=None):
        """pt_scene_update_mesh: replace mesh, materials, lights and textures in place and rebuild the reference tree on the
        device, as from_mesh would; options, variant, culling, counters and work buffers stay. host_or_desc: a HostScene, a
        SceneDesc, or a dict of arrays (the last two with max_leaf_size). `.build_stats` has the builder's numbers."""
        st = np.zeros(1, BUILD_STATS)
        d, keep, leaf = Scene._mesh_desc(host_or_desc, max_leaf_size)
        _check(lib().pt_scene_update_mesh(self.h, C.byref(d), leaf, _p(st)), "pt_scene_update_mesh")
        del keep
        self.build_stats = {f: st[0][f].item() for f in BUILD_STATS.names}
        return self

    def update_vertices(self, points, normals=None, n_points=None, n_normals=None):
        """pt_scene_update_vertices[_device]: new vertex positions (float4 each) and, optionally, new normals for a scene that
        went through the device builder; topology, materials, lights' triangles and textures stay, and the tree is rebuilt on the
        device. Host arrays (anything numpy can view as bytes) go to the host form. A device buffer goes to the _device form: an
        object with data_ptr() (a tensor on the scene's device, 16 bytes per element row), or a raw device pointer as an int with
        its count in n_points / n_normals, as the other *_device wrappers take pointers. `.build_stats` has the builder's numbers."""
        def dev(x, n):
            if isinstance(x, int):
                if n is None:
                    raise PtError("update_vertices: a raw device pointer needs its count (n_points / n_normals)")
                return x, int(n)
            return x.data_ptr(), (x.numel() * x.element_size()) // 16 if n is None else int(n)
        st = np.zeros(1, BUILD_STATS)
        on_device = isinstance(points, int) or hasattr(points, "data_ptr")
        if on_device:
            if normals is not None and not (isinstance(normals, int) or hasattr(normals, "data_ptr")):
                raise PtError("update_vertices: points are on the device, normals must be too")
            pp, np_ = dev(points, n_points)
            nn, nn_ = dev(normals, n_normals) if normals is not None else (None, 0)
            _check(lib().pt_scene_update_vertices_device(self.h, pp, np_, nn, nn_, _p(st)), "pt_scene_update_vertices_device")
        else:
            pts = np.ascontiguousarray(points).view(np.uint8).reshape(-1)
            nrm = np.ascontiguousarray(normals).view(np.uint8).reshape(-1) if normals is not None else None
            _check(lib().pt_scene_update_vertices(self.h, _p(pts), pts.size // 16, _p(nrm), nrm.size // 16 if nrm is not None else 0, _p(st)),
                   "pt_scene_update_vertices")
        self.build_stats = {f: st[0][f].item() for f in BUILD_STATS.names}
        return self

    def update_materials(self, materials):
        """pt_scene_update_materials: replace the material table in place; nothing is rebuilt. materials: the scene's number of
        176-byte pt_material records, as an array of them or anything numpy can view as bytes (HostScene.array("materials") gives
        one). Works on any scene; the scene then renders as a fresh one of the edited description, and has_motion drops to 0."""
        m = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
        if m.size % 176:
            raise PtError("update_materials: %d bytes are no whole number of 176-byte material records" % m.size)
        _check(lib().pt_scene_update_materials(self.h, _p(m), m.size // 176), "pt_scene_update_materials")
        return self

    def update_emission(self, light_indices, emission):
        """pt_scene_update_emission: lights[light_indices[k]] and every triangle of that light emit emission[k] (float4 each; rows
        of three floats get w = 0). The set of lights stays; a repeated index takes its last entry."""
        idx = np.ascontiguousarray(light_indices, np.int32).reshape(-1)
        e = np.ascontiguousarray(emission, np.float32).reshape(len(idx), -1)
        if e.shape[1] == 3:
            e = np.ascontiguousarray(np.concatenate([e, np.zeros((len(idx), 1), np.float32)], axis=1))
        if e.shape[1] != 4:
            raise PtError("update_emission: one float3 or float4 per light index is needed")
        _check(lib().pt_scene_update_emission(self.h, len(idx), _p(idx), _p(e)), "pt_scene_update_emission")
        return self

    @property
    def generation(self):
        """pt_scene_generation: 0 after create, +1 per successful update_mesh / update_vertices / update_materials /
        update_emission."""
        return lib().pt_scene_generation(self.h)

    def packed(self, what):
        """Test hook (pt_debug_packed): the records as uint8 [count, record size]; what = nodes / tris / attrs / lights / mats."""
        code, rec = {"nodes": (0, 64), "tris": (1, 48), "attrs": (2, 80), "lights": (3, 64), "mats": (4, 96)}[what]
        n = lib().pt_debug_packed(self.h, code, None, 0)
        if n < 0:
            raise PtError("pt_debug_packed failed")
        buf = np.zeros((max(n, 0), rec), np.uint8)
        if n:
            lib().pt_debug_packed(self.h, code, _p(buf), buf.nbytes)
        return buf

    @staticmethod
    def from_arrays(arrays, options=None):
        """pt_scene_create straight from arrays in the reference's layouts (dict of buffers: points,
        normals, uvs, mesh, lights, bvh, indices, materials[, textures])."""
        d, _keep = _desc_from_arrays(arrays)
        return Scene(desc=d, options=options)

    @staticmethod
    def from_config(config_path, base_dir=None, render_number=0):
        hs = HostScene(config_path, base_dir, render_number)
        return Scene(hs), hs

    def close(self):
        if self.h:
            lib().pt_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- launchers ------------------------------------------------------------------------------
    def render(self, camera, w, h, spp, max_depth, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, tiles=None,
               counters=False, out=None):
        """Host-buffer launcher: returns (sum-of-samples [h,w,4] float32, per-pixel counters [h,w,8] or None)."""
        col = np.zeros((h, w, 4), np.float32) if out is None else out
        cnt = np.zeros((h, w, 8), np.uint32) if counters else None
        tr = C.byref(tiles) if tiles is not None else None
        if counters:
            rc = lib().pt_render_counted(self.h, C.byref(camera), w, h, spp, max_depth, integrator, int(use_mis), seed, tr, _p(col), _p(cnt))
        else:                                               # the timed kernels (time slices, REFILL / FLAT instantiations)
            rc = lib().pt_render(self.h, C.byref(camera), w, h, spp, max_depth, integrator, int(use_mis), seed, tr, _p(col))
        _check(rc, "pt_render")
        return col, cnt

    def render_tiles_device(self, camera, w, h, spp, max_depth, d_tile_ptr, integrator=UNIDIRECTIONAL, use_mis=True,
                            seed=SEED, tiles=None, count_work=False, stream=0):
        tr = C.byref(tiles) if tiles is not None else None
        rc = lib().pt_render_tiles_device(self.h, C.byref(camera), w, h, spp, max_depth, integrator, int(use_mis), seed, tr,
                                          d_tile_ptr, int(count_work), stream or None)
        _check(rc, "pt_render_tiles_device")

    def render_aovs(self, camera, w, h, aov_spp=1, seed=SEED):
        """pt_render_aovs: first-hit feature buffers, returns (albedo, normal_depth) as [h,w,4] float32 (y = 0 the bottom row).
        albedo.w is the coverage (hits / aov_spp), normal_depth.w the mean hit distance."""
        alb = np.zeros((h, w, 4), np.float32)
        nd = np.zeros((h, w, 4), np.float32)
        _check(lib().pt_render_aovs(self.h, C.byref(camera), w, h, aov_spp, seed, _p(alb), _p(nd)), "pt_render_aovs")
        return alb, nd

    def render_aovs_device(self, camera, w, h, d_albedo_ptr, d_normal_depth_ptr, aov_spp=1, seed=SEED, stream=0):
        """pt_render_aovs_device: the same into device buffers of w*h float4 each, asynchronous on `stream`."""
        _check(lib().pt_render_aovs_device(self.h, C.byref(camera), w, h, aov_spp, seed, d_albedo_ptr, d_normal_depth_ptr, stream or None),
               "pt_render_aovs_device")

    def render_aovs_chain(self, camera, w, h, max_links, aov_spp=1, seed=SEED, links=False):
        """pt_render_aovs_chain: feature buffers that follow mirrors and glass (at most max_links specular links, 0..16) to the first
        non-specular surface: its albedo and normal, the summed path length as depth. Returns (albedo, normal_depth) as render_aovs
        does, and with links=True also the mean link count per pixel, [h,w] float32."""
        alb = np.zeros((h, w, 4), np.float32)
        nd = np.zeros((h, w, 4), np.float32)
        ln = np.zeros((h, w), np.float32) if links else None
        _check(lib().pt_render_aovs_chain(self.h, C.byref(camera), w, h, aov_spp, max_links, seed, _p(alb), _p(nd), _p(ln) if links else None),
               "pt_render_aovs_chain")
        return (alb, nd, ln) if links else (alb, nd)

    def render_aovs_chain_device(self, camera, w, h, max_links, d_albedo_ptr, d_normal_depth_ptr, d_links_ptr=None, aov_spp=1, seed=SEED, stream=0):
        """pt_render_aovs_chain_device: the same into device buffers (w*h float4 twice, and w*h floats or None), asynchronous on `stream`."""
        _check(lib().pt_render_aovs_chain_device(self.h, C.byref(camera), w, h, aov_spp, max_links, seed, d_albedo_ptr, d_normal_depth_ptr,
                                                 d_links_ptr or None, stream or None), "pt_render_aovs_chain_device")

    def render_aovs_centre(self, camera, w, h, max_links=0, links=False):
        """pt_render_aovs_centre: feature buffers through pixel centres: one ray per pixel that no random draw reaches (the camera's
        jitter and aperture play no part), so there is no aov_spp and no seed. Equals render_aovs_chain(cam0, w, h, max_links,
        aov_spp=1) bit for bit, cam0 being the camera with antiAliasJitterDist = aperture = 0. Returns (albedo, normal_depth), and
        the link count [h,w] float32 as a third item with links=True."""
        alb = np.zeros((h, w, 4), np.float32); nd = np.zeros((h, w, 4), np.float32)
        ln = np.zeros((h, w), np.float32) if links else None
        _check(lib().pt_render_aovs_centre(self.h, C.byref(camera), w, h, max_links, _p(alb), _p(nd), _p(ln) if links else None),
               "pt_render_aovs_centre")
        return (alb, nd, ln) if links else (alb, nd)

    def render_aovs_centre_device(self, camera, w, h, max_links, d_albedo_ptr, d_normal_depth_ptr, d_links_ptr=0, stream=0):
        """pt_render_aovs_centre_device: the same into device buffers (w*h float4 twice, and w*h floats or None), asynchronous on `stream`."""
        _check(lib().pt_render_aovs_centre_device(self.h, C.byref(camera), w, h, max_links, d_albedo_ptr, d_normal_depth_ptr, d_links_ptr or None,
                                                  stream or None), "pt_render_aovs_centre_device")

    def render_motion(self, camera, w, h, guides=False):
        """pt_render_motion: per pixel centre, where the surface point it shows was before the scene's most recent update_vertices:
        [h,w,4] float32, (P'.x, P'.y, P'.z, 1) for a surface that moved, all zeros for a static one or no hit. First hit only.
        guides=True returns (albedo, normal_depth, motion), the first two being render_aovs_centre(camera, w, h, 0) bit for bit
        from the same trace."""
        mv = np.zeros((h, w, 4), np.float32)
        alb = np.zeros((h, w, 4), np.float32) if guides else None
        nd = np.zeros((h, w, 4), np.float32) if guides else None
        _check(lib().pt_render_motion(self.h, C.byref(camera), w, h, _p(alb), _p(nd), _p(mv)), "pt_render_motion")
        return (alb, nd, mv) if guides else mv

    def render_motion_device(self, camera, w, h, d_albedo_ptr, d_normal_depth_ptr, d_motion_ptr, stream=0):
        """pt_render_motion_device: the same into device buffers (w*h float4 each; the two guide pointers both 0 / None or both set),
        asynchronous on `stream`."""
        _check(lib().pt_render_motion_device(self.h, C.byref(camera), w, h, d_albedo_ptr or None, d_normal_depth_ptr or None, d_motion_ptr or None,
                                             stream or None), "pt_render_motion_device")

    def render_motion_chain(self, camera, w, h, max_links, guides=False, links=False):
        """pt_render_motion_chain: render_motion along render_aovs_centre's chain of at most max_links mirror and glass links: for a
        moved surface seen behind static mirrors or panes, (V'.x, V'.y, V'.z, 1) with V' the virtual image of where it was; zeros
        where a mirror on the way moved. max_links 0 is render_motion. guides=True returns (albedo, normal_depth, motion), the first
        two being render_aovs_centre(camera, w, h, max_links) bit for bit from the same trace; links=True (with guides) appends the
        link count [h,w] float32."""
        mv = np.zeros((h, w, 4), np.float32)
        alb = np.zeros((h, w, 4), np.float32) if guides else None
        nd = np.zeros((h, w, 4), np.float32) if guides else None
        ln = np.zeros((h, w), np.float32) if links else None
        _check(lib().pt_render_motion_chain(self.h, C.byref(camera), w, h, max_links, _p(alb), _p(nd), _p(ln), _p(mv)), "pt_render_motion_chain")
        out = ((alb, nd, mv) if guides else (mv,)) + ((ln,) if links else ())
        return out if len(out) > 1 else mv

    def render_motion_chain_device(self, camera, w, h, max_links, d_albedo_ptr, d_normal_depth_ptr, d_links_ptr, d_motion_ptr, stream=0):
        """pt_render_motion_chain_device: the same into device buffers (w*h float4 each, w*h floats for the links; the two guide
        pointers both 0 / None or both set, the links pointer only with them), asynchronous on `stream`."""
        _check(lib().pt_render_motion_chain_device(self.h, C.byref(camera), w, h, max_links, d_albedo_ptr or None, d_normal_depth_ptr or None,
                                                   d_links_ptr or None, d_motion_ptr or None, stream or None), "pt_render_motion_chain_device")

    def render_ids(self, camera, w, h, max_links=0):
        """pt_render_ids: [h,w,4] int32 per pixel centre: (tri, material, light or -1, info), info = backface bit | links << 8, of
        the surface render_aovs_centre(camera, w, h, max_links) shows there; (-1, -1, -1, 0) where the ray hits nothing. tri indexes
        the description's triangles, material is update_materials' row, light is update_emission's index."""
        ids = np.zeros((h, w, 4), np.int32)
        _check(lib().pt_render_ids(self.h, C.byref(camera), w, h, max_links, _p(ids)), "pt_render_ids")
        return ids

    def render_ids_device(self, camera, w, h, max_links, d_ids_ptr, stream=0):
        """pt_render_ids_device: the same into a device buffer of w*h int32x4, asynchronous on `stream`."""
        _check(lib().pt_render_ids_device(self.h, C.byref(camera), w, h, max_links, d_ids_ptr or None, stream or None), "pt_render_ids_device")

    def pick(self, camera, w, h, xy, max_links=0):
        """pt_pick: render_ids at the pixels xy ([n,2] int32, (x, y) each): (ids [n,4] int32, hit [n,4] float32), hit being the
        surface's point and the chain's summed path length (render_aovs_centre's depth there); zeros for a miss. Blocking."""
        q = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        ids, hit = np.zeros((len(q), 4), np.int32), np.zeros((len(q), 4), np.float32)
        _check(lib().pt_pick(self.h, C.byref(camera), w, h, len(q), _p(q), max_links, _p(ids), _p(hit)), "pt_pick")
        return ids, hit

    # -- ray queries ----------------------------------------------------------------------------
    @staticmethod
    def _query_rays(what, rays):
        """(is_torch, rays, n): an [n, 8] float32 numpy array (ox, oy, oz, max_t, dx, dy, dz, pad; a RAY_DTYPE array is viewed as one),
        or a contiguous float32 torch tensor of that shape on the current HIP device, which is used where it lies."""
        if isinstance(rays, np.ndarray) or not hasattr(rays, "data_ptr"):
            a = np.asarray(rays)
            if a.dtype == RAY_DTYPE:
                a = np.ascontiguousarray(a).view(np.float32)
            a = np.ascontiguousarray(a, np.float32).reshape(-1, 8)
            return False, a, len(a)
        import torch
        if not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() or rays.dim() != 2 or rays.shape[1] != 8:
            raise PtError("%s: a torch tensor of rays must be a contiguous [n, 8] float32 tensor on the scene's device" % what)
        if rays.device.index != torch.cuda.current_device():
            raise PtError("%s: the rays are on %s but the current device is %d" % (what, rays.device, torch.cuda.current_device()))
        return True, rays, int(rays.shape[0])

    def _query(self, name, rays, outs, args, empty=(False, False)):
        """The form of every query_* method above query_camera_rays: pt_<name>_device on torch's current stream with data_ptr()s for
        a torch tensor of rays, the host entry pt_<name> for numpy. outs: per output (columns, numpy dtype), or None for one the
        caller left out: float32 tensors [n, columns] ([n] for 0 columns) on the rays' device, or numpy zeros of that shape (a
        record dtype: [n] records). args(rays, outs) gives the C arguments between n and the stream from the pointers. empty:
        whether the (torch, numpy) form makes the call at n == 0; an empty tensor has no data pointer to hand over and passes NULL.
        Returns the outputs."""
        is_torch, r, n = self._query_rays(name, rays)
        if is_torch:
            import torch
            out = [o and torch.empty((n, o[0]) if o[0] else (n,), dtype=torch.float32, device=r.device) for o in outs]
            ptr = lambda t: t.data_ptr() if t is not None and n else None
            fn, tail = "pt_%s_device" % name, (torch.cuda.current_stream(r.device).cuda_stream or None,)
        else:
            out = [o and np.zeros((n, o[0]) if o[0] and not np.dtype(o[1]).names else n, o[1]) for o in outs]
            ptr, fn, tail = _p, "pt_" + name, ()
        if n or empty[0 if is_torch else 1]:
            _check(getattr(lib(), fn)(self.h, n, *args(ptr(r), [ptr(o) for o in out]), *tail), fn)
        return out

    def query_closest(self, rays, surfaces=False, reorder=False):
        """pt_query_closest: the closest hit of each of the caller's rays ([n, 8] float32: o, max_t, d, pad; d is not normalised).
        numpy in: the host form, hits as a RAY_HIT_DTYPE array (t, u, v, tri; tri -1 for a miss) and, with surfaces, a
        RAY_SURFACE_DTYPE array. A torch tensor on the scene's device in: pt_query_closest_device on torch's current stream, no host
        copy, hits as an [n, 4] float32 tensor whose column 3 holds tri's bits (hits.view(torch.int32)[:, 3]) and surfaces as
        [n, 12] float32 (words 8..10 material, light, backface as int32 bits). Returns hits, or (hits, surfaces)."""
        flags = QUERY_REORDER if reorder else 0
        hits, surf = self._query("query_closest", rays, [(4, RAY_HIT_DTYPE), (12, RAY_SURFACE_DTYPE) if surfaces else None],
                                 lambda r, o: (r, o[0], o[1], flags))
        return (hits, surf) if surfaces else hits

    def query_shadow(self, rays, reorder=False):
        """pt_query_shadow: the shadow ray's throughput along each ray below its max_t, [n, 4] float32 (rgb, 0): zeros when occluded.
        numpy in, numpy out (host form); a torch tensor on the scene's device in, a torch tensor out, on torch's current stream."""
        flags = QUERY_REORDER if reorder else 0
        return self._query("query_shadow", rays, [_F4], lambda r, o: (r, o[0], flags))[0]

    def query_radiance(self, rays, spp, max_depth, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, first_stream=0, stream_pad=False):
        """pt_query_radiance: the path-traced light along each of the caller's rays ([n, 8] float32: o, max_t, d, pad; d must be unit),
        summed over spp samples: [n, 4] float32 (rgb sums, 0). Ray i draws from stream first_stream + i of `seed`, or, with stream_pad,
        first_stream + its pad word (uint32). numpy in, numpy out (host form); a torch tensor on the scene's device in, a torch tensor
        out, on torch's current stream with no host copy. The centre rays of a camera without jitter and aperture give render()'s sums."""
        flags = QUERY_STREAM_PAD if stream_pad else 0
        return self._query("query_radiance", rays, [_F4], lambda r, o: (r, spp, max_depth, integrator, 1 if use_mis else 0, seed, first_stream, o[0], flags),
                           empty=(True, True))[0]

    def query_radiance_moments(self, rays, spp, batch_spp, max_depth, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, first_stream=0,
                               stream_pad=False):
        """pt_query_radiance_moments: query_radiance in spp / batch_spp batches of batch_spp samples. Returns (S, Q), both [n, 4]
        float32: S is query_radiance's output bit for bit, Q per rgb channel the sum of the ray's squared batch sums and Q.w the
        number of batches, as render_moments defines them. numpy in, numpy out (host form); a torch tensor on the scene's device in,
        tensors out, on torch's current stream with no host copy. denoise_var(S.reshape(h, w, 4), Q.reshape(h, w, 4), spp,
        spp // batch_spp, ...) reads the pair."""
        flags = QUERY_STREAM_PAD if stream_pad else 0
        return tuple(self._query("query_radiance_moments", rays, [_F4, _F4], lambda r, o: (
            r, spp, batch_spp, max_depth, integrator, 1 if use_mis else 0, seed, first_stream, o[0], o[1], flags), empty=(True, True)))

    def query_irradiance(self, records, lanes, spp_lane, max_depth, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, first_stream=0,
                         moments=False, flags=0):
        """pt_query_irradiance: cosine-sampled light at surface points. records is [n, 8] float32 (point, max_t, unit normal, pad:
        rays.irradiance_records, rays.records_from_surfaces); each record runs on `lanes` (1, 2, 4 .. 64) lanes of a wave, lane l of
        record i on stream first_stream + i * lanes + l of `seed` (with flags = QUERY_STREAM_PAD: the record's pad word for i), spp_lane
        samples per lane. Returns S, [n, 4] float32 (the rgb sums of the record's lanes * spp_lane samples, 0), or with moments (S, Q),
        Q the sum of the squared lane sums and Q.w = lanes: denoise_var(S.reshape(h, w, 4), Q.reshape(h, w, 4), lanes * spp_lane, lanes,
        ...) reads the pair. Irradiance is pi * S / (lanes * spp_lane). numpy in, numpy out (host form); a torch tensor on the scene's
        device in, tensors out, on torch's current stream with no host copy."""
        s, q = self._query("query_irradiance", records, [_F4, _F4 if moments else None], lambda r, o: (
            r, lanes, spp_lane, max_depth, integrator, 1 if use_mis else 0, seed, first_stream, o[0], o[1], flags), empty=(True, True))
        return (s, q) if moments else s

    def query_irradiance_rays(self, records, lanes, seed=SEED, first_stream=0, draw_offset=None, flags=0):
        """pt_query_irradiance_rays_device: the rays query_irradiance's samples start from, [n * lanes, 8] float32: ray i * lanes + l is
        lane l of record i, made of draws draw_offset[i * lanes + l] and the next of that lane's stream ([n * lanes] uint32 or int32;
        None: the lane's first sample), with the record's max_t and, in its pad word, what the lane adds to first_stream:
        query_radiance(rays, 1, ..., first_stream=first_stream, stream_pad=True) is such a sample's radiance. A torch tensor of records
        on the scene's device gives a tensor, on torch's current stream; numpy records are copied up and the rays come back as numpy."""
        return self._lane_rays("query_irradiance_rays", records, lanes, seed, first_stream, draw_offset, flags)

    def _lane_rays(self, name, records, lanes, seed, first_stream, draw_offset, flags, per_record=None):
        """query_irradiance_rays, query_sh_rays and query_distance_rays: pt_<name>_device on [n, 8] records, n * per_record rays out.
        `lanes` is the argument handed to C; per_record, the lanes a record has, is that number unless given (query_distance_rays
        hands over res and has res * res)."""
        import torch
        is_torch, r, n = self._query_rays(name, records)
        dev = r.device if is_torch else torch.device("cuda", torch.cuda.current_device())
        d = r if is_torch else torch.from_numpy(r if r.flags.writeable else r.copy()).to(dev)
        per_record = lanes if per_record is None else per_record
        m = n * per_record if per_record > 0 else 0
        off = None
        if draw_offset is not None:
            off = draw_offset if hasattr(draw_offset, "data_ptr") else torch.from_numpy(np.ascontiguousarray(draw_offset).astype(np.int32).reshape(-1))
            off = off.to(device=dev, dtype=torch.int32).contiguous()
            if off.numel() != m:
                raise PtError("%s: draw_offset has %d entries for %d rays" % (name, off.numel(), m))
        out = torch.empty((m, 8), dtype=torch.float32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None and n else None
        fn = "pt_%s_device" % name
        _check(getattr(lib(), fn)(self.h, n, ptr(d), lanes, seed, first_stream, ptr(off), ptr(out), flags, torch.cuda.current_stream(dev).cuda_stream or None), fn)
        return out if is_torch else out.cpu().numpy()

    def query_sh(self, records, lanes, spp_lane, max_depth, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, first_stream=0, flags=0):
        """pt_query_sh: a light probe's SH coefficients. records is [n, 8] float32 (probe position, max_t, three words that are not
        read, pad: rays.sh_records, rays.sh_grid); each record runs on `lanes` (a power of two in 1..4096) lanes, lane l of record i
        on stream first_stream + i * lanes + l of `seed` (with flags = QUERY_STREAM_PAD: the record's pad word for i), spp_lane
        samples per lane, each in a uniformly distributed direction. Returns [n, 9, 4] float32: per SH term of bands 0..2 the rgb
        sums of Li * Y_k over the record's lanes * spp_lane samples, and 0. The radiance coefficients are 4 pi / (lanes * spp_lane)
        times the sums (rays.sh_irradiance evaluates them). numpy in, numpy out (host form); a torch tensor on the scene's device in,
        a tensor out, on torch's current stream with no host copy, the workspace of lanes > 64 a torch tensor."""
        work = None
        if hasattr(records, "data_ptr") and not isinstance(records, np.ndarray):
            import torch
            nbytes = lib().pt_query_sh_workspace_bytes(int(records.shape[0]) if records.dim() else 0, lanes)
            work = torch.empty(nbytes, dtype=torch.uint8, device=records.device) if nbytes else None
            tail = lambda o: (o[0], work.data_ptr() if work is not None else None, flags)
        else:
            tail = lambda o: (o[0], flags)
        out = self._query("query_sh", records, [(36, np.float32)], lambda r, o: (
            r, lanes, spp_lane, max_depth, integrator, 1 if use_mis else 0, seed, first_stream) + tail(o), empty=(True, True))[0]
        return out.reshape(-1, 9, 4)

    def query_sh_rays(self, records, lanes, seed=SEED, first_stream=0, draw_offset=None, flags=0):
        """pt_query_sh_rays_device: the rays query_sh's samples start from, [n * lanes, 8] float32, as query_irradiance_rays gives
        them for query_irradiance: ray i * lanes + l is lane l of record i, made of draws draw_offset[i * lanes + l] and the next of
        that lane's stream, with the record's max_t and, in its pad word, what the lane adds to first_stream."""
        return self._lane_rays("query_sh_rays", records, lanes, seed, first_stream, draw_offset, flags)

    def query_distance(self, records, res, spp_lane=1, seed=SEED, first_stream=0, flags=0):
        """pt_query_distance: a probe's octahedral map of hit-distance moments. records is [n, 8] float32 (probe position, max_t, three
        words that are not read, pad: rays.distance_records, rays.sh_grid); each record runs on res * res lanes (res 4, 8, 16 or 32),
        lane ty * res + tx being texel (tx, ty) on stream first_stream + i * res * res + ty * res + tx of `seed` (with flags =
        QUERY_STREAM_PAD: the record's pad word for i), spp_lane samples per lane, each in a direction of its texel. With flags =
        QUERY_TEXEL_CENTRE: one sample at the texel's centre, no random number. Returns [n, res, res, 4] float32, indexed [i, ty, tx]:
        the sum of the samples' distances to the nearest surface (max_t where there is none), the sum of their squares, the number
        that hit, and the number of those hits seen from behind (rays.distance_visibility and rays.grid_irradiance read the first
        two). numpy in, numpy out (host form); a torch tensor on the scene's device in, a tensor out, on torch's current stream with
        no host copy."""
        cols = res * res * 4 if res in (4, 8, 16, 32) else 4          # (any other res is refused before anything is written)
        out = self._query("query_distance", records, [(cols, np.float32)], lambda r, o: (r, res, spp_lane, seed, first_stream, o[0], flags),
                          empty=(True, True))[0]
        return out.reshape(out.shape[0], res, res, 4)

    def query_distance_rays(self, records, res, seed=SEED, first_stream=0, draw_offset=None, flags=0):
        """pt_query_distance_rays_device: the rays query_distance's samples start from, [n * res * res, 8] float32, as query_sh_rays
        gives them for query_sh: ray i * res * res + l is lane l of record i, made of draws draw_offset[i * res * res + l] and the
        next of that lane's stream (with QUERY_TEXEL_CENTRE: the texel's centre), with the record's max_t and, in its pad word, what
        the lane adds to first_stream: query_closest on them is what a sample of query_distance sees."""
        return self._lane_rays("query_distance_rays", records, res, seed, first_stream, draw_offset, flags,
                               per_record=res * res if res in (4, 8, 16, 32) else 0)

    def query_guides(self, rays, max_links=0, links=False):
        """pt_query_guides: render_aovs_centre's guides for each of the caller's rays ([n, 8] float32: o, max_t, d, pad; d must be
        unit): (albedo, normal_depth), both [n, 4] float32: (albedo, 1) and (normal, summed path length) of the first non-specular
        surface behind at most max_links mirror and glass links, zeros for a ray that hits nothing below its max_t; links=True appends
        the link count [n] float32. numpy in, numpy out (host form); a torch tensor on the scene's device in, tensors out, on torch's
        current stream with no host copy."""
        alb, nd, ln = self._query("query_guides", rays, [_F4, _F4, (0, np.float32) if links else None], lambda r, o: (r, max_links, o[0], o[1], o[2], 0),
                                  empty=(False, True))
        return (alb, nd, ln) if links else (alb, nd)

    def query_camera_rays(self, camera, w, h, max_t=QUERY_MAX_T):
        """pt_query_camera_rays_device: the centre rays of render_aovs_centre / render_ids as an [h*w, 8] float32 torch tensor on the
        current device (ray y*w + x), made on torch's current stream."""
        return query_camera_rays(camera, w, h, max_t)

    @property
    def has_motion(self):
        """pt_scene_has_motion: 1 if the scene keeps the positions from before its last update (it was an update_vertices), else 0."""
        return lib().pt_scene_has_motion(self.h)

    def render_adaptive(self, camera, w, h, max_depth, min_spp, max_spp, chunk_spp, threshold, integrator=UNIDIRECTIONAL, use_mis=True,
                        seed=SEED):
        """pt_render_adaptive: tiles stop when their error estimate falls below `threshold` (the schedule: include/pt_api.h).
        Returns (colors [h,w,4] float32: each pixel the SUM of its own tile's samples, tile_spp [tilesY,tilesX] int32,
        tile_err [tilesY,tilesX] float32, stats dict). adaptive_mean(colors, tile_spp) gives the per-pixel mean."""
        ty, tx = (h + 7) // 8, (w + 7) // 8
        col = np.zeros((h, w, 4), np.float32)
        spp = np.zeros((ty, tx), np.int32)
        err = np.zeros((ty, tx), np.float32)
        st = AdaptiveStats()
        p = adaptive_params(min_spp, max_spp, chunk_spp, threshold)
        _check(lib().pt_render_adaptive(self.h, C.byref(camera), w, h, max_depth, integrator, int(use_mis), seed, C.byref(p), _p(col),
                                        _p(spp), _p(err), C.byref(st)), "pt_render_adaptive")
        return col, spp, err, {f: getattr(st, f) for f, _ in AdaptiveStats._fields_}

    def render_adaptive_device(self, camera, w, h, max_depth, min_spp, max_spp, chunk_spp, threshold, d_rgba_sum_ptr, d_tile_spp_ptr,
                               d_tile_err_ptr=None, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, stream=0):
        """pt_render_adaptive_device: the same into device buffers (w*h float4, one int32 / float32 per tile; the error buffer may be
        None). Blocks; the work is enqueued on `stream`. Returns the stats dict."""
        st = AdaptiveStats()
        p = adaptive_params(min_spp, max_spp, chunk_spp, threshold)
        _check(lib().pt_render_adaptive_device(self.h, C.byref(camera), w, h, max_depth, integrator, int(use_mis), seed, C.byref(p),
                                               d_rgba_sum_ptr, d_tile_spp_ptr, d_tile_err_ptr or None, C.byref(st), stream or None),
               "pt_render_adaptive_device")
        return {f: getattr(st, f) for f, _ in AdaptiveStats._fields_}

    def render_adaptive_moments(self, camera, w, h, max_depth, min_spp, max_spp, chunk_spp, threshold, integrator=UNIDIRECTIONAL,
                                use_mis=True, seed=SEED):
        """pt_render_adaptive_moments: render_adaptive plus the sum of squared batch sums (a batch = a half-round of chunk_spp
        samples; max_spp must be a multiple of 2 * chunk_spp). Returns (colors, sq, tile_spp, tile_err, stats): sq [h,w,4] float32 as
        render_moments' Q at each tile's own count, the rest as render_adaptive. denoise_var_tiles(colors, sq, tile_spp, chunk_spp,
        ...) reads them."""
        ty, tx = (h + 7) // 8, (w + 7) // 8
        col = np.zeros((h, w, 4), np.float32)
        sq = np.zeros((h, w, 4), np.float32)
        spp = np.zeros((ty, tx), np.int32)
        err = np.zeros((ty, tx), np.float32)
        st = AdaptiveStats()
        p = adaptive_params(min_spp, max_spp, chunk_spp, threshold)
        _check(lib().pt_render_adaptive_moments(self.h, C.byref(camera), w, h, max_depth, integrator, int(use_mis), seed, C.byref(p), _p(col),
                                                _p(sq), _p(spp), _p(err), C.byref(st)), "pt_render_adaptive_moments")
        return col, sq, spp, err, {f: getattr(st, f) for f, _ in AdaptiveStats._fields_}

    def render_adaptive_moments_device(self, camera, w, h, max_depth, min_spp, max_spp, chunk_spp, threshold, d_rgba_sum_ptr, d_sq_sum_ptr,
                                       d_tile_spp_ptr, d_tile_err_ptr=None, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, stream=0):
        """pt_render_adaptive_moments_device: the same into device buffers (two of w*h float4, one int32 / float32 per tile; the
        error buffer may be None). Blocks; the work is enqueued on `stream`. Returns the stats dict."""
        st = AdaptiveStats()
        p = adaptive_params(min_spp, max_spp, chunk_spp, threshold)
        _check(lib().pt_render_adaptive_moments_device(self.h, C.byref(camera), w, h, max_depth, integrator, int(use_mis), seed, C.byref(p),
                                                       d_rgba_sum_ptr, d_sq_sum_ptr, d_tile_spp_ptr, d_tile_err_ptr or None, C.byref(st),
                                                       stream or None), "pt_render_adaptive_moments_device")
        return {f: getattr(st, f) for f, _ in AdaptiveStats._fields_}

    def render_moments(self, camera, w, h, spp, batch_spp, max_depth, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED):
        """pt_render_moments: `spp` samples per pixel in spp / batch_spp batches. Returns (S, Q), both [h,w,4] float32: S the
        sum of the samples (render(spp) into zeros, bit for bit), Q per rgb channel the sum of the squared batch sums, Q.w
        the number of batches. denoise_var(S, Q, spp, spp // batch_spp, ...) reads the pair."""
        S = np.zeros((h, w, 4), np.float32)
        Q = np.zeros((h, w, 4), np.float32)
        _check(lib().pt_render_moments(self.h, C.byref(camera), w, h, spp, batch_spp, max_depth, integrator, int(use_mis), seed, _p(S), _p(Q)),
               "pt_render_moments")
        return S, Q

    def render_moments_device(self, camera, w, h, spp, batch_spp, max_depth, d_rgba_sum_ptr, d_sq_sum_ptr, integrator=UNIDIRECTIONAL,
                              use_mis=True, seed=SEED, stream=0):
        """pt_render_moments_device: the same into device buffers of w*h float4 each. Blocks; the work is enqueued on `stream`."""
        _check(lib().pt_render_moments_device(self.h, C.byref(camera), w, h, spp, batch_spp, max_depth, integrator, int(use_mis), seed,
                                              d_rgba_sum_ptr, d_sq_sum_ptr, stream or None), "pt_render_moments_device")

    def render_moments_tiles(self, camera, w, h, spp, batch_spp, max_depth, tile_list, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED):
        """pt_render_moments_tiles: render_moments on the 8x8 tiles of `tile_list` (int32 [count], strictly ascending tile numbers,
        row-major over the tile grid). Returns (S, Q) as render_moments does: its values on the listed tiles, S = 0 and Q.rgb = 0
        elsewhere, Q.w the number of batches everywhere."""
        if not isinstance(tile_list, np.ndarray) or tile_list.dtype != np.int32 or tile_list.ndim != 1:
            raise PtError("render_moments_tiles: tile_list must be a one-dimensional int32 array")
        lst = np.ascontiguousarray(tile_list)
        S = np.zeros((h, w, 4), np.float32)
        Q = np.zeros((h, w, 4), np.float32)
        _check(lib().pt_render_moments_tiles(self.h, C.byref(camera), w, h, spp, batch_spp, max_depth, integrator, int(use_mis), seed,
                                             _p(lst) if lst.size else None, int(lst.size), _p(S), _p(Q)), "pt_render_moments_tiles")
        return S, Q

    def render_moments_tiles_device(self, camera, w, h, spp, batch_spp, max_depth, d_tile_list_ptr, count, d_rgba_sum_ptr, d_sq_sum_ptr,
                                    integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, stream=0):
        """pt_render_moments_tiles_device: the same from a device list of `count` tiles (trusted) into device buffers of w*h float4
        each. Blocks; the work is enqueued on `stream`."""
        _check(lib().pt_render_moments_tiles_device(self.h, C.byref(camera), w, h, spp, batch_spp, max_depth, integrator, int(use_mis), seed,
                                                    d_tile_list_ptr or None, int(count), d_rgba_sum_ptr, d_sq_sum_ptr, stream or None),
               "pt_render_moments_tiles_device")

    def launch_unidirectional(self, max_depth, camera, num_sample, use_mis, w, h, d_colors_ptr):
        _check(lib().pt_launch_unidirectional(max_depth, camera, self.h, num_sample, int(use_mis), w, h, d_colors_ptr), "pt_launch_unidirectional")

    def launch_progressive(self, integrator, max_depth, camera, num_sample, use_mis, w, h, d_colors_ptr, chunk_spp, progress=None):
        """pt_launch_progressive: progress(samples_done) -> truthy to stop early."""
        cb = PROGRESS_FN((lambda done, _u: int(bool(progress(done)))) if progress else (lambda done, _u: 0))
        _check(lib().pt_launch_progressive(integrator, max_depth, camera, self.h, num_sample, int(use_mis), w, h, d_colors_ptr, chunk_spp, cb, None),
               "pt_launch_progressive")

    def launch_naive_unidirectional(self, max_depth, camera, num_sample, use_mis, w, h, d_colors_ptr):
        _check(lib().pt_launch_naive_unidirectional(max_depth, camera, self.h, num_sample, int(use_mis), w, h, d_colors_ptr), "pt_launch_naive_unidirectional")

    def set_variant(self, variant):
        """0 / "megakernel" (default) or 1 / "wavefront" (stream-compacted A/B variant; same results)."""
        v = {"megakernel": 0, "wavefront": 1}.get(variant, variant)
        _check(lib().pt_set_variant(self.h, int(v)), "pt_set_variant")
        return self

    def counters(self):
        out = np.zeros(8, np.uint64)
        _check(lib().pt_get_counters(self.h, _p(out)), "pt_get_counters")
        return dict(zip(COUNTER_KEYS, (int(v) for v in out)))

    def reset_counters(self):
        _check(lib().pt_reset_counters(self.h), "pt_reset_counters")

    def debug_stamps(self):
        out = np.zeros(8, np.uint64)
        _check(lib().pt_debug_stamps(self.h, _p(out)), "pt_debug_stamps")
        return dict(zip(("regen", "closest", "bounce_logic", "wave_lifetimes", "not_earliest_start", "latest_end", "shadow_in_bounce", "slot7"), (int(v) for v in out)))

    def global_node_fetches(self):
        """Counting launches since reset_counters: internal-node fetches that missed the LDS scene cache (normal builds)."""
        out = np.zeros(8, np.uint64)
        _check(lib().pt_debug_stamps(self.h, _p(out)), "pt_debug_stamps")
        return int(out[0])

    def debug_lane_util(self):
        """-DPT_UTIL builds, after a counting render: lanes carried per trip through the traversal loops."""
        out = np.zeros(8, np.uint64)
        _check(lib().pt_debug_stamps(self.h, _p(out)), "pt_debug_stamps")
        v = [int(x) for x in out]
        names = ("closest_nodes", "closest_tris", "shadow_nodes", "shadow_tris")
        return {n: {"wave_trips": v[2 * k], "lane_trips": v[2 * k + 1], "lanes_per_trip": (v[2 * k + 1] / v[2 * k]) if v[2 * k] else 0.0}
                for k, n in enumerate(names)}

    def set_culling(self, on=True):
        """pt_set_culling: opt-in box culling (not the reference's visiting set; see pt_api.h)."""
        _check(lib().pt_set_culling(self.h, int(bool(on))), "pt_set_culling")
        return self

    def flags(self):
        f = lib().pt_scene_flags(self.h)
        return {"onchip": bool(f & 1), "persistent": bool(f & 2), "time_slices": bool(f & 4), "hbm_kernel": bool(f & 8), "culling": bool(f & 16), "refill": bool(f & 32), "flat": bool(f & 64), "simple": bool(f & 128), "flat_pair": bool(f & 256), "leaf_table": bool(f & 512), "lean": bool(f & 1024)}

    def tile_handovers(self):
        """pt_last_tile_handovers: tiles that changed hands between waves in the last (completed) megakernel launch."""
        n = lib().pt_last_tile_handovers(self.h)
        _check(min(n, 0), "pt_last_tile_handovers")
        return n

    def last_moments_launches(self):
        """pt_last_moments_launches: render launches of the last render_moments* call on this scene — 1 if it ran fused (option
        "moments_fused"), spp / batch_spp in batches, 0 for an empty tile list, -1 before any such call."""
        return int(lib().pt_last_moments_launches(self.h))

    def queue_header(self):
        """pt_debug_queue_header: the tile queue's 16 header words after the last queued launch (None: that launch used no queue)."""
        out = (C.c_int * 16)()
        rc = lib().pt_debug_queue_header(self.h, out)
        if rc < 0:
            _check(rc, "pt_debug_queue_header")
        return list(out) if rc == 1 else None

    def queue_stalls(self):
        """pt_queue_stalls: launches whose queue waiters gave up although the frame was complete (not an error)."""
        return int(lib().pt_queue_stalls(self.h))

    def last_kernel_ms(self):
        """Device time of the last launch; raises if that launch did not finish its frame (tile-queue timeout).
        Callers of render_tiles_device (asynchronous) learn about an incomplete frame here."""
        ms = float(lib().pt_last_kernel_ms(self.h))
        if ms < 0.0:
            raise PtError("pt_last_kernel_ms: " + (lib().pt_last_error().decode(errors="replace") or "the last launch failed"))
        return ms

    # -- probes ---------------------------------------------------------------------------------
    def trace_closest(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = len(rays)
        oi = np.zeros((n, 4), np.int32); of = np.zeros((n, 12), np.float32); cnt = np.zeros(8, np.uint64)
        _check(lib().pt_probe_trace_closest(self.h, n, _p(rays), _p(oi), _p(of), _p(cnt)), "pt_probe_trace_closest")
        return oi, of, dict(zip(COUNTER_KEYS, (int(v) for v in cnt)))

    def trace_shadow(self, rays, max_t):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        max_t = np.ascontiguousarray(max_t, np.float32)
        n = len(rays)
        of = np.zeros((n, 3), np.float32); cnt = np.zeros(8, np.uint64)
        _check(lib().pt_probe_trace_shadow(self.h, n, _p(rays), _p(max_t), _p(of), _p(cnt)), "pt_probe_trace_shadow")
        return of, dict(zip(COUNTER_KEYS, (int(v) for v in cnt)))

    def bsdf_sample(self, material, wi, backface, subseq, eta_i=1.0, eta_t=1.0, seed=SEED):
        material = np.ascontiguousarray(material, np.int32); wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        backface = np.ascontiguousarray(backface, np.int32); subseq = np.ascontiguousarray(subseq, np.uint32)
        n = len(material)
        out = np.zeros((n, 8), np.float32)
        _check(lib().pt_probe_bsdf_sample(self.h, n, _p(material), _p(wi), _p(backface), eta_i, eta_t, seed, _p(subseq), _p(out)), "pt_probe_bsdf_sample")
        return out

    def bsdf_eval(self, material, wi, wo, eta_i=1.0, eta_t=1.0):
        material = np.ascontiguousarray(material, np.int32)
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3); wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        n = len(material)
        out = np.zeros((n, 4), np.float32)
        _check(lib().pt_probe_bsdf_eval(self.h, n, _p(material), _p(wi), _p(wo), eta_i, eta_t, _p(out)), "pt_probe_bsdf_eval")
        return out


MULTI_STATS = np.dtype([("n_devices", "i4"), ("gather", "i4"), ("kernel_ms", "f4", (16,)), ("render_ms", "f4"), ("gather_ms", "f4"), ("total_ms", "f4")])


class MultiScene:
    """pt_multi: one replica of the scene per HIP device, frame sharded by interleaved 8x8 tiles, one gather to device 0
    (include/pt_api.h, "multi-GPU"). device_ids=None means devices 0 .. n_devices-1."""

    def __init__(self, host: "HostScene", n_devices, device_ids=None, options=None):
        ids = np.ascontiguousarray(device_ids, np.int32) if device_ids is not None else None
        self._keep = host
        self.h = lib().pt_multi_create(C.byref(host.desc), int(n_devices), _p(ids))
        if not self.h:
            raise PtError("pt_multi_create failed: " + lib().pt_last_error().decode(errors="replace"))
        for k, v in (options or {}).items():
            self.set_option(k, v)
        self.stats = None

    def set_option(self, name, value):
        _check(lib().pt_multi_set_option(self.h, name.encode(), int(value)), "pt_multi_set_option(%s)" % name)
        return self

    def set_variant(self, variant):
        _check(lib().pt_multi_set_variant(self.h, int({"megakernel": 0, "wavefront": 1}.get(variant, variant))), "pt_multi_set_variant")
        return self

    def render(self, camera, w, h, spp, max_depth, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, out=None):
        col = np.zeros((h, w, 4), np.float32) if out is None else out
        st = np.zeros(1, MULTI_STATS)
        _check(lib().pt_multi_render(self.h, C.byref(camera), w, h, spp, max_depth, integrator, int(use_mis), seed, _p(col), _p(st)), "pt_multi_render")
        self.stats = {"n_devices": int(st[0]["n_devices"]), "gather": {0: "none", 1: "rccl", 2: "peer_copy"}[int(st[0]["gather"])],
                      "kernel_ms": [float(v) for v in st[0]["kernel_ms"][:int(st[0]["n_devices"])]],
                      "render_ms": float(st[0]["render_ms"]), "gather_ms": float(st[0]["gather_ms"]), "total_ms": float(st[0]["total_ms"])}
        return col

    def close(self):
        if self.h:
            lib().pt_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_multi(host, n_devices, camera, w, h, spp, max_depth, integrator=UNIDIRECTIONAL, use_mis=True, seed=SEED, device_ids=None):
    """pt_render_multi: the one-shot form."""
    ids = np.ascontiguousarray(device_ids, np.int32) if device_ids is not None else None
    col = np.zeros((h, w, 4), np.float32)
    _check(lib().pt_render_multi(C.byref(host.desc), int(n_devices), _p(ids), C.byref(camera), w, h, spp, max_depth, integrator, int(use_mis), seed, _p(col), None),
           "pt_render_multi")
    return col


def parse_options(pairs):
    """["flat=0", "waves_hbm=2"] -> {"flat": 0, "waves_hbm": 2} for the --opt flag of bench.py and tools/."""
    out = {}
    for p in pairs or []:
        for item in p.split(","):
            if item:
                k, _, v = item.partition("=")
                out[k.strip()] = int(v)
    return out


def denoise_defaults():
    """pt_denoise_defaults as a dict: iterations, sigma_color, sigma_normal, sigma_depth."""
    p = DenoiseParams()
    lib().pt_denoise_defaults(C.byref(p))
    return {f: getattr(p, f) for f, _ in DenoiseParams._fields_}


def _filter_params(struct, defaults, **given):
    """A pt_denoise_params or pt_denoise_var_params: the library's defaults, then every parameter that is not None."""
    p = struct()
    defaults(C.byref(p))
    for f, v in given.items():
        if v is not None:
            setattr(p, f, v)
    return p


def _denoise_params(iterations, sigma_color, sigma_normal, sigma_depth):
    return _filter_params(DenoiseParams, lib().pt_denoise_defaults, iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal,
                          sigma_depth=sigma_depth)


def _denoise_call(what, frame, out, call):
    """What the host form pt_<what> of a filter does once its arrays are checked: `out`, or a new array like `frame` (the input it
    may alias), checked; then call(w, h, out pointer), which returns the library's status."""
    h, w = frame.shape[:2]
    res = np.empty_like(frame) if out is None else out
    if not (isinstance(res, np.ndarray) and res.dtype == np.float32 and res.shape == frame.shape and res.flags.c_contiguous):
        raise PtError("%s: out must be a C-contiguous float32 array of shape %s" % (what, frame.shape))
    _check(call(w, h, _p(res)), "pt_" + what)
    return res


def denoise_workspace_bytes(w, h):
    return int(lib().pt_denoise_workspace_bytes(w, h))


def denoise(rgba_sum, spp, albedo, normal_depth, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, out=None):
    """pt_denoise (host, blocking): the a-trous filter guided by render_aovs' buffers. rgba_sum is the radiance SUM of
    `spp` samples as pt_render leaves it ([h,w,4] float32); returns the same units. A None parameter takes the library
    default (denoise_defaults()). `out` may be rgba_sum itself."""
    S, A, N = _f4_frames("denoise", (("rgba_sum", rgba_sum), ("albedo", albedo), ("normal_depth", normal_depth)))
    return _denoise_call("denoise", S, out, lambda w, h, res: lib().pt_denoise(
        w, h, _p(S), int(spp), _p(A), _p(N), C.byref(_denoise_params(iterations, sigma_color, sigma_normal, sigma_depth)), res))


def denoise_device(w, h, d_rgba_sum_ptr, spp, d_albedo_ptr, d_normal_depth_ptr, d_workspace_ptr, d_out_ptr, iterations=None,
                   sigma_color=None, sigma_normal=None, sigma_depth=None, stream=0):
    """pt_denoise_device: device buffers of w*h float4 (e.g. tensor.data_ptr()) and a workspace of
    denoise_workspace_bytes(w, h) bytes; asynchronous on `stream`. d_out_ptr may equal d_rgba_sum_ptr."""
    p = _denoise_params(iterations, sigma_color, sigma_normal, sigma_depth)
    _check(lib().pt_denoise_device(w, h, d_rgba_sum_ptr, int(spp), d_albedo_ptr, d_normal_depth_ptr, C.byref(p), d_workspace_ptr, d_out_ptr,
                                   stream or None), "pt_denoise_device")


def denoise_var_defaults():
    """pt_denoise_var_defaults as a dict: iterations, sigma_var, sigma_normal, sigma_depth."""
    p = DenoiseVarParams()
    lib().pt_denoise_var_defaults(C.byref(p))
    return {f: getattr(p, f) for f, _ in DenoiseVarParams._fields_}


def _denoise_var_params(iterations, sigma_var, sigma_normal, sigma_depth):
    return _filter_params(DenoiseVarParams, lib().pt_denoise_var_defaults, iterations=iterations, sigma_var=sigma_var, sigma_normal=sigma_normal,
                          sigma_depth=sigma_depth)


def denoise_var_workspace_bytes(w, h):
    return int(lib().pt_denoise_var_workspace_bytes(w, h))


def denoise_var(rgba_sum, sq_sum, spp, batches, albedo, normal_depth, iterations=None, sigma_var=None, sigma_normal=None, sigma_depth=None,
                out=None):
    """pt_denoise_var (host, blocking): the a-trous filter with a variance-guided colour weight. rgba_sum and sq_sum are
    what Scene.render_moments returned for `spp` samples in `batches` batches ([h,w,4] float32); albedo and normal_depth come
    from render_aovs. Returns the filtered radiance sum. A None parameter takes the library default
    (denoise_var_defaults()). `out` may be rgba_sum itself."""
    S, Q, A, N = _f4_frames("denoise_var", tuple(zip(_SUMS, (rgba_sum, sq_sum, albedo, normal_depth))))
    return _denoise_call("denoise_var", S, out, lambda w, h, res: lib().pt_denoise_var(
        w, h, _p(S), _p(Q), int(spp), int(batches), _p(A), _p(N), C.byref(_denoise_var_params(iterations, sigma_var, sigma_normal, sigma_depth)), res))


def denoise_var_device(w, h, d_rgba_sum_ptr, d_sq_sum_ptr, spp, batches, d_albedo_ptr, d_normal_depth_ptr, d_workspace_ptr, d_out_ptr,
                       iterations=None, sigma_var=None, sigma_normal=None, sigma_depth=None, stream=0):
    """pt_denoise_var_device: device buffers of w*h float4 and a workspace of denoise_var_workspace_bytes(w, h) bytes;
    asynchronous on `stream`. d_out_ptr may equal d_rgba_sum_ptr."""
    p = _denoise_var_params(iterations, sigma_var, sigma_normal, sigma_depth)
    _check(lib().pt_denoise_var_device(w, h, d_rgba_sum_ptr, d_sq_sum_ptr, int(spp), int(batches), d_albedo_ptr, d_normal_depth_ptr,
                                       C.byref(p), d_workspace_ptr, d_out_ptr, stream or None), "pt_denoise_var_device")


def denoise_var_tiles_workspace_bytes(w, h):
    return int(lib().pt_denoise_var_tiles_workspace_bytes(w, h))


def denoise_var_tiles(rgba_sum, sq_sum, tile_spp, batch_spp, albedo, normal_depth, iterations=None, sigma_var=None, sigma_normal=None,
                      sigma_depth=None, out=None):
    """pt_denoise_var_tiles (host, blocking): denoise_var on an adaptive frame. rgba_sum, sq_sum and tile_spp (int32
    [ceil(h/8), ceil(w/8)]) are what Scene.render_adaptive_moments returned with chunk_spp = batch_spp; albedo and normal_depth come
    from render_aovs*. Returns the filtered radiance sum in the units of rgba_sum: adaptive_mean(result, tile_spp) and
    resolve(result, tile_spp=tile_spp) apply as to the raw frame. `out` may be rgba_sum itself."""
    S, Q, A, N = _f4_frames("denoise_var_tiles", tuple(zip(_SUMS, (rgba_sum, sq_sum, albedo, normal_depth))))
    h, w = S.shape[:2]
    if not isinstance(tile_spp, np.ndarray) or tile_spp.dtype != np.int32 or tile_spp.shape != ((h + 7) // 8, (w + 7) // 8):
        raise PtError("denoise_var_tiles: tile_spp must be an int32 [%d, %d] array for a %d x %d frame" % ((h + 7) // 8, (w + 7) // 8, w, h))
    return _denoise_call("denoise_var_tiles", S, out, lambda w, h, res: lib().pt_denoise_var_tiles(
        w, h, _p(S), _p(Q), _p(np.ascontiguousarray(tile_spp)), int(batch_spp), _p(A), _p(N),
        C.byref(_denoise_var_params(iterations, sigma_var, sigma_normal, sigma_depth)), res))


def denoise_var_tiles_device(w, h, d_rgba_sum_ptr, d_sq_sum_ptr, d_tile_spp_ptr, batch_spp, d_albedo_ptr, d_normal_depth_ptr, d_workspace_ptr,
                             d_out_ptr, iterations=None, sigma_var=None, sigma_normal=None, sigma_depth=None, stream=0):
    """pt_denoise_var_tiles_device: device buffers of w*h float4, the tile map (one int32 per tile, trusted) and a workspace of
    denoise_var_tiles_workspace_bytes(w, h) bytes; asynchronous on `stream`. d_out_ptr may equal d_rgba_sum_ptr."""
    p = _denoise_var_params(iterations, sigma_var, sigma_normal, sigma_depth)
    _check(lib().pt_denoise_var_tiles_device(w, h, d_rgba_sum_ptr, d_sq_sum_ptr, d_tile_spp_ptr, int(batch_spp), d_albedo_ptr,
                                             d_normal_depth_ptr, C.byref(p), d_workspace_ptr, d_out_ptr, stream or None),
           "pt_denoise_var_tiles_device")


def temporal_defaults():
    """pt_temporal_defaults as a dict: max_history, depth_tol, normal_tol."""
    p = TemporalParams()
    lib().pt_temporal_defaults(C.byref(p))
    return {f: getattr(p, f) for f, _ in TemporalParams._fields_}


def _temporal_params(max_history, depth_tol, normal_tol):
    p = TemporalParams()
    lib().pt_temporal_defaults(C.byref(p))
    for f, v in (("max_history", max_history), ("depth_tol", depth_tol), ("normal_tol", normal_tol)):
        if v is not None:
            setattr(p, f, v)
    return p


def _f4_frames(what, named, shape=None):
    """The float32 [h, w, 4] checks of denoise_var, for a list of (name, array); returns the contiguous arrays."""
    arrs = []
    for name, a in named:
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 3 or a.shape[2] != 4:
            raise PtError("%s: %s must be a float32 [h, w, 4] array" % (what, name))
        arrs.append(np.ascontiguousarray(a))
    shape = arrs[0].shape if shape is None else shape
    if any(a.shape != shape for a in arrs):
        raise PtError("%s: shapes differ: %s" % (what, ", ".join(str(a.shape) for a in arrs)))
    return arrs


def _history_arrays(what, shape, prev_normal_depth, hist, hist_len):
    """The three history arrays of temporal_accumulate*: all None, or checked against the frame's shape and made contiguous."""
    given = [x is not None for x in (prev_normal_depth, hist, hist_len)]
    if any(given) != all(given):
        raise PtError("%s: prev_normal_depth, hist and hist_len must be all None or all given" % what)
    if not all(given):
        return None, None, None
    PN, H = _f4_frames(what, (("prev_normal_depth", prev_normal_depth), ("hist", hist)), shape)
    if not isinstance(hist_len, np.ndarray) or hist_len.dtype != np.float32 or hist_len.shape != shape[:2]:
        raise PtError("%s: hist_len must be a float32 [%d, %d] array" % (what, shape[0], shape[1]))
    return PN, H, np.ascontiguousarray(hist_len)


_SUMS = ("rgba_sum", "sq_sum", "albedo", "normal_depth")
_CUR = ("cur", "normal_depth")


def _temporal_host(what, camera, camera_prev, names, frames, sums, history, params, motion=None, tile_live=None):
    """The host form pt_<what>: `frames` are its [h, w, 4] arrays in the order of the C arguments, called `names` in the messages; the
    (spp, batches) of `sums` follow the first two of them. `motion` and `tile_live` are (array or None,) for an entry that takes one."""
    arrs = _f4_frames(what, tuple(zip(names, frames)))
    h, w = arrs[0].shape[:2]
    extra = list(_history_arrays(what, arrs[0].shape, *history))
    if motion is not None:
        extra.append(None if motion[0] is None else _f4_frames(what, (("motion", motion[0]),), arrs[0].shape)[0])
    if tile_live is not None:
        extra.append(None if tile_live[0] is None else _tile_map(what, tile_live[0], h, w))
    out, out_len = np.empty_like(arrs[0]), np.empty((h, w), np.float32)
    p = _temporal_params(*params)
    args = [_p(a) for a in arrs[:2]] + [int(v) for v in sums] + [_p(a) for a in arrs[2:] + extra]
    _check(getattr(lib(), "pt_" + what)(w, h, C.byref(camera), C.byref(camera_prev) if camera_prev is not None else None, *args, C.byref(p),
                                        _p(out), _p(out_len)), "pt_" + what)
    return out, out_len


def _temporal_device(what, w, h, camera, camera_prev, frame, optional, outputs, params, stream):
    """The device form pt_<what>_device: `frame` are this frame's arguments in C order, `optional` the pointers that may be 0 / None
    (the history triple, then the motion buffer or the tile map)."""
    p = _temporal_params(*params)
    _check(getattr(lib(), "pt_%s_device" % what)(w, h, C.byref(camera), C.byref(camera_prev) if camera_prev is not None else None, *frame,
                                                 *(x or None for x in optional), C.byref(p), *outputs, stream or None), "pt_%s_device" % what)


def temporal_accumulate(camera, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, camera_prev=None, prev_normal_depth=None, hist=None,
                        hist_len=None, max_history=None, depth_tol=None, normal_tol=None):
    """pt_temporal_accumulate (host, blocking): blend this frame (render_moments' sums, render_aovs' buffers) into the history
    reprojected from the previous camera. prev_normal_depth, hist ([h,w,4] float32) and hist_len ([h,w] float32) are all None on
    the first frame. camera_prev None = the camera did not move. Returns new (hist, hist_len); the inputs are left untouched.
    A None parameter takes the library default (temporal_defaults())."""
    return _temporal_host("temporal_accumulate", camera, camera_prev, _SUMS, (rgba_sum, sq_sum, albedo, normal_depth), (spp, batches),
                          (prev_normal_depth, hist, hist_len), (max_history, depth_tol, normal_tol))


def temporal_accumulate_device(w, h, camera, camera_prev, d_rgba_sum_ptr, d_sq_sum_ptr, spp, batches, d_albedo_ptr, d_normal_depth_ptr,
                               d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr, d_out_hist_ptr, d_out_hist_len_ptr, max_history=None,
                               depth_tol=None, normal_tol=None, stream=0):
    """pt_temporal_accumulate_device: device buffers (w*h float4; the two lengths w*h float), asynchronous on `stream`, no
    workspace. The three history pointers are 0 / None on the first frame; the outputs must not alias the input history."""
    _temporal_device("temporal_accumulate", w, h, camera, camera_prev,
                     (d_rgba_sum_ptr, d_sq_sum_ptr, int(spp), int(batches), d_albedo_ptr, d_normal_depth_ptr),
                     (d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr), (d_out_hist_ptr, d_out_hist_len_ptr),
                     (max_history, depth_tol, normal_tol), stream)


def temporal_accumulate_motion(camera, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, camera_prev=None, prev_normal_depth=None, hist=None,
                               hist_len=None, motion=None, max_history=None, depth_tol=None, normal_tol=None):
    """pt_temporal_accumulate_motion (host, blocking): temporal_accumulate with Scene.render_motion's buffer for this camera: a pixel
    whose motion.w is 1 reprojects motion.xyz, where its surface point was, and never takes the identity path. motion None is
    temporal_accumulate bit for bit. Returns new (hist, hist_len)."""
    return _temporal_host("temporal_accumulate_motion", camera, camera_prev, _SUMS, (rgba_sum, sq_sum, albedo, normal_depth), (spp, batches),
                          (prev_normal_depth, hist, hist_len), (max_history, depth_tol, normal_tol), motion=(motion,))


def temporal_accumulate_motion_device(w, h, camera, camera_prev, d_rgba_sum_ptr, d_sq_sum_ptr, spp, batches, d_albedo_ptr, d_normal_depth_ptr,
                                      d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr, d_motion_ptr, d_out_hist_ptr, d_out_hist_len_ptr,
                                      max_history=None, depth_tol=None, normal_tol=None, stream=0):
    """pt_temporal_accumulate_motion_device: temporal_accumulate_device plus the device motion buffer (0 / None: none)."""
    _temporal_device("temporal_accumulate_motion", w, h, camera, camera_prev,
                     (d_rgba_sum_ptr, d_sq_sum_ptr, int(spp), int(batches), d_albedo_ptr, d_normal_depth_ptr),
                     (d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr, d_motion_ptr), (d_out_hist_ptr, d_out_hist_len_ptr),
                     (max_history, depth_tol, normal_tol), stream)


def temporal_accumulate_cur_motion(camera, cur, normal_depth, camera_prev=None, prev_normal_depth=None, hist=None, hist_len=None, motion=None,
                                   max_history=None, depth_tol=None, normal_tol=None):
    """pt_temporal_accumulate_cur_motion (host, blocking): temporal_accumulate_cur with a motion buffer, as temporal_accumulate_motion."""
    return _temporal_host("temporal_accumulate_cur_motion", camera, camera_prev, _CUR, (cur, normal_depth), (),
                          (prev_normal_depth, hist, hist_len), (max_history, depth_tol, normal_tol), motion=(motion,))


def temporal_accumulate_cur_motion_device(w, h, camera, camera_prev, d_cur_ptr, d_normal_depth_ptr, d_prev_normal_depth_ptr, d_hist_ptr,
                                          d_hist_len_ptr, d_motion_ptr, d_out_hist_ptr, d_out_hist_len_ptr, max_history=None, depth_tol=None,
                                          normal_tol=None, stream=0):
    """pt_temporal_accumulate_cur_motion_device: temporal_accumulate_cur_device plus the device motion buffer (0 / None: none)."""
    _temporal_device("temporal_accumulate_cur_motion", w, h, camera, camera_prev, (d_cur_ptr, d_normal_depth_ptr),
                     (d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr, d_motion_ptr), (d_out_hist_ptr, d_out_hist_len_ptr),
                     (max_history, depth_tol, normal_tol), stream)


def respond_defaults():
    """pt_respond_defaults as a dict: radius, power, threshold."""
    p = RespondParams()
    lib().pt_respond_defaults(C.byref(p))
    return {f: getattr(p, f) for f, _ in RespondParams._fields_}


def _respond_params(threshold=None, radius=None, power=None):
    p = RespondParams()
    lib().pt_respond_defaults(C.byref(p))
    for f, v in (("threshold", threshold), ("radius", radius), ("power", power)):
        if v is not None:
            setattr(p, f, v if f == "threshold" else int(v))
    return p


def temporal_respond_workspace_bytes(w, h):
    """pt_temporal_respond_workspace_bytes: the device form's workspace, 36 bytes per pixel."""
    return int(lib().pt_temporal_respond_workspace_bytes(w, h))


def temporal_accumulate_respond(camera, normal_depth, rgba_sum=None, sq_sum=None, spp=0, batches=0, albedo=None, cur=None, camera_prev=None,
                                prev_normal_depth=None, hist=None, hist_len=None, motion=None, max_history=None, depth_tol=None, normal_tol=None,
                                threshold=None, radius=None, power=None, scale=True):
    """pt_temporal_accumulate_respond (host, blocking): temporal_accumulate (the frame as rgba_sum, sq_sum, spp, batches, albedo) or
    temporal_accumulate_cur (the frame as `cur`), with or without `motion`, and a per-pixel change test that scales the gathered
    history length by lambda in [0, 1] where the frame and the history disagree by more than `threshold` standard deviations over a
    (2 radius + 1)^2 window. threshold inf is the base function bit for bit. Returns (hist, hist_len, lambda [h,w] float32 or None
    with scale False). A None parameter takes the library default (temporal_defaults(), respond_defaults())."""
    what = "temporal_accumulate_respond"
    named = [(n, a) for n, a in (("rgba_sum", rgba_sum), ("sq_sum", sq_sum), ("albedo", albedo), ("cur", cur)) if a is not None]
    arrs = dict(zip([n for n, _ in named] + ["normal_depth"], _f4_frames(what, tuple(named) + (("normal_depth", normal_depth),))))
    nd = arrs["normal_depth"]
    h, w = nd.shape[:2]
    PN, H, HL = _history_arrays(what, nd.shape, prev_normal_depth, hist, hist_len)
    M = None if motion is None else _f4_frames(what, (("motion", motion),), nd.shape)[0]
    out, out_len = np.empty_like(nd), np.empty((h, w), np.float32)
    lam = np.empty((h, w), np.float32) if scale else None
    tp, rp = _temporal_params(max_history, depth_tol, normal_tol), _respond_params(threshold, radius, power)
    _check(lib().pt_temporal_accumulate_respond(w, h, C.byref(camera), C.byref(camera_prev) if camera_prev is not None else None,
                                                _p(arrs.get("rgba_sum")), _p(arrs.get("sq_sum")), int(spp), int(batches), _p(arrs.get("albedo")),
                                                _p(arrs.get("cur")), _p(nd), _p(PN), _p(H), _p(HL), _p(M), C.byref(tp), C.byref(rp), _p(out),
                                                _p(out_len), _p(lam)), "pt_" + what)
    return out, out_len, lam


def temporal_accumulate_respond_device(w, h, camera, camera_prev, d_rgba_sum_ptr, d_sq_sum_ptr, spp, batches, d_albedo_ptr, d_cur_ptr,
                                       d_normal_depth_ptr, d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr, d_motion_ptr, d_workspace_ptr,
                                       d_out_hist_ptr, d_out_hist_len_ptr, d_out_scale_ptr=0, max_history=None, depth_tol=None, normal_tol=None,
                                       threshold=None, radius=None, power=None, stream=0):
    """pt_temporal_accumulate_respond_device: device buffers, asynchronous on `stream` (two launches). Exactly one of the sums
    (d_rgba_sum_ptr, d_sq_sum_ptr, d_albedo_ptr) and d_cur_ptr is given, the other 0 / None; d_workspace_ptr holds
    temporal_respond_workspace_bytes(w, h) bytes; d_motion_ptr and d_out_scale_ptr may be 0 / None."""
    tp, rp = _temporal_params(max_history, depth_tol, normal_tol), _respond_params(threshold, radius, power)
    o = lambda x: x or None
    _check(lib().pt_temporal_accumulate_respond_device(w, h, C.byref(camera), C.byref(camera_prev) if camera_prev is not None else None,
                                                       o(d_rgba_sum_ptr), o(d_sq_sum_ptr), int(spp), int(batches), o(d_albedo_ptr), o(d_cur_ptr),
                                                       d_normal_depth_ptr, o(d_prev_normal_depth_ptr), o(d_hist_ptr), o(d_hist_len_ptr),
                                                       o(d_motion_ptr), C.byref(tp), C.byref(rp), o(d_workspace_ptr), d_out_hist_ptr,
                                                       d_out_hist_len_ptr, o(d_out_scale_ptr), stream or None),
           "pt_temporal_accumulate_respond_device")


def _tile_map(what, tile_live, h, w):
    shape = ((h + 7) // 8, (w + 7) // 8)
    if not isinstance(tile_live, np.ndarray) or tile_live.dtype != np.int32 or tile_live.shape != shape:
        raise PtError("%s: tile_live must be an int32 [%d, %d] array for a %d x %d frame" % (what, shape[0], shape[1], w, h))
    return np.ascontiguousarray(tile_live)


def temporal_accumulate_live(camera, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth, hist, hist_len, tile_live,
                             camera_prev=None, max_history=None, depth_tol=None, normal_tol=None):
    """pt_temporal_accumulate_live (host, blocking): temporal_accumulate for a resting camera with a map of live tiles (int32
    [ceil(h/8), ceil(w/8)], as temporal_select returns it; None = every tile live). A tile whose entry is 0 keeps its history and
    length bit for bit; the others blend this frame in. camera_prev must be None or equal to camera. Returns new (hist, hist_len)."""
    return _temporal_host("temporal_accumulate_live", camera, camera_prev, _SUMS, (rgba_sum, sq_sum, albedo, normal_depth), (spp, batches),
                          (prev_normal_depth, hist, hist_len), (max_history, depth_tol, normal_tol), tile_live=(tile_live,))


def temporal_accumulate_live_device(w, h, camera, camera_prev, d_rgba_sum_ptr, d_sq_sum_ptr, spp, batches, d_albedo_ptr, d_normal_depth_ptr,
                                    d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr, d_tile_live_ptr, d_out_hist_ptr, d_out_hist_len_ptr,
                                    max_history=None, depth_tol=None, normal_tol=None, stream=0):
    """pt_temporal_accumulate_live_device: temporal_accumulate_device plus the device map of live tiles (0 / None: every tile)."""
    _temporal_device("temporal_accumulate_live", w, h, camera, camera_prev,
                     (d_rgba_sum_ptr, d_sq_sum_ptr, int(spp), int(batches), d_albedo_ptr, d_normal_depth_ptr),
                     (d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr, d_tile_live_ptr), (d_out_hist_ptr, d_out_hist_len_ptr),
                     (max_history, depth_tol, normal_tol), stream)


def converge_defaults():
    """pt_converge_defaults as a dict: threshold, min_history."""
    p = ConvergeParams()
    lib().pt_converge_defaults(C.byref(p))
    return {f: getattr(p, f) for f, _ in ConvergeParams._fields_}


def _converge_params(threshold, min_history):
    p = ConvergeParams()
    lib().pt_converge_defaults(C.byref(p))
    if threshold is not None:
        p.threshold = threshold
    if min_history is not None:
        p.min_history = int(min_history)
    return p


def temporal_select(hist, hist_len, threshold=None, min_history=None):
    """pt_temporal_select (host, blocking): which 8x8 tiles of a history still need samples. hist is [h,w,4] float32, hist_len
    [h,w] float32. Returns (tile_err float32 [ceil(h/8), ceil(w/8)], tile_live int32 of the same shape, live_list: the live
    tiles' numbers, ascending int32). A None parameter takes the library default (converge_defaults())."""
    H, = _f4_frames("temporal_select", (("hist", hist),))
    h, w = H.shape[:2]
    if not isinstance(hist_len, np.ndarray) or hist_len.dtype != np.float32 or hist_len.shape != (h, w):
        raise PtError("temporal_select: hist_len must be a float32 [%d, %d] array" % (h, w))
    HL = np.ascontiguousarray(hist_len)
    ty, tx = (h + 7) // 8, (w + 7) // 8
    err, live, lst, cnt = np.empty((ty, tx), np.float32), np.empty((ty, tx), np.int32), np.empty(ty * tx, np.int32), np.zeros(1, np.int32)
    p = _converge_params(threshold, min_history)
    _check(lib().pt_temporal_select(w, h, _p(H), _p(HL), C.byref(p), _p(err), _p(live), _p(lst), _p(cnt)), "pt_temporal_select")
    return err, live, lst[:int(cnt[0])].copy()


def temporal_select_device(w, h, d_hist_ptr, d_hist_len_ptr, d_tile_err_ptr, d_tile_live_ptr, d_list_ptr, d_count_ptr, threshold=None,
                           min_history=None, stream=0):
    """pt_temporal_select_device: device buffers (one float, one int32 and one list slot per 8x8 tile, one int32 count),
    asynchronous on `stream`."""
    p = _converge_params(threshold, min_history)
    _check(lib().pt_temporal_select_device(w, h, d_hist_ptr, d_hist_len_ptr, C.byref(p), d_tile_err_ptr, d_tile_live_ptr, d_list_ptr,
                                           d_count_ptr, stream or None), "pt_temporal_select_device")


def temporal_accumulate_cur(camera, cur, normal_depth, camera_prev=None, prev_normal_depth=None, hist=None, hist_len=None, max_history=None,
                            depth_tol=None, normal_tol=None):
    """pt_temporal_accumulate_cur (host, blocking): temporal_accumulate with this frame's working pixels given in `cur` ([h,w,4]
    float32: e and V, V = -1 for a pass-through pixel), as upsample returns them. Returns new (hist, hist_len)."""
    return _temporal_host("temporal_accumulate_cur", camera, camera_prev, _CUR, (cur, normal_depth), (),
                          (prev_normal_depth, hist, hist_len), (max_history, depth_tol, normal_tol))


def temporal_accumulate_cur_device(w, h, camera, camera_prev, d_cur_ptr, d_normal_depth_ptr, d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr,
                                   d_out_hist_ptr, d_out_hist_len_ptr, max_history=None, depth_tol=None, normal_tol=None, stream=0):
    """pt_temporal_accumulate_cur_device: temporal_accumulate_device with the frame's (e, V) buffer in place of its sums."""
    _temporal_device("temporal_accumulate_cur", w, h, camera, camera_prev, (d_cur_ptr, d_normal_depth_ptr),
                     (d_prev_normal_depth_ptr, d_hist_ptr, d_hist_len_ptr), (d_out_hist_ptr, d_out_hist_len_ptr),
                     (max_history, depth_tol, normal_tol), stream)


def upsample_defaults():
    """pt_upsample_defaults as a dict: sigma_normal, sigma_depth."""
    p = UpsampleParams()
    lib().pt_upsample_defaults(C.byref(p))
    return {f: getattr(p, f) for f, _ in UpsampleParams._fields_}


def _upsample_params(sigma_normal, sigma_depth):
    p = UpsampleParams()
    lib().pt_upsample_defaults(C.byref(p))
    for f, v in (("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth)):
        if v is not None:
            setattr(p, f, v)
    return p


def scaled_camera(camera, scale):
    """pt_camera_scaled: the camera of the low-res frame of render scale `scale` (w and h divided, nothing else changed)."""
    out = Camera()
    _check(lib().pt_camera_scaled(C.byref(camera), int(scale), C.byref(out)), "pt_camera_scaled")
    return out


def upsample(scale, rgba_sum_lo, sq_sum_lo, spp, batches, albedo_lo, normal_depth_lo, albedo, normal_depth, sigma_normal=None, sigma_depth=None):
    """pt_upsample (host, blocking): a frame rendered with scaled_camera(cam, scale) (render_moments' sums of `spp` samples in
    `batches` batches and render_aovs' buffers, [h / scale, w / scale, 4] float32) brought to the display size of albedo and
    normal_depth ([h, w, 4], render_aovs with cam). Returns cur [h, w, 4]: e and V in denoise_var's working format, V = -1 for a
    pass-through pixel; temporal_accumulate_cur and denoise_hist read it."""
    A, N = _f4_frames("upsample", (("albedo", albedo), ("normal_depth", normal_depth)))
    h, w = A.shape[:2]
    scale = int(scale)
    lo_shape = (h // scale, w // scale, 4) if scale > 0 else None
    S, Q, Al, Nl = _f4_frames("upsample", (("rgba_sum_lo", rgba_sum_lo), ("sq_sum_lo", sq_sum_lo), ("albedo_lo", albedo_lo),
                                           ("normal_depth_lo", normal_depth_lo)), lo_shape)
    out = np.empty_like(A)
    p = _upsample_params(sigma_normal, sigma_depth)
    _check(lib().pt_upsample(w, h, scale, _p(S), _p(Q), int(spp), int(batches), _p(Al), _p(Nl), _p(A), _p(N), C.byref(p), _p(out)), "pt_upsample")
    return out


def upsample_device(w, h, scale, d_rgba_sum_lo_ptr, d_sq_sum_lo_ptr, spp, batches, d_albedo_lo_ptr, d_normal_depth_lo_ptr, d_albedo_ptr,
                    d_normal_depth_ptr, d_out_cur_ptr, sigma_normal=None, sigma_depth=None, stream=0):
    """pt_upsample_device: device buffers ((w / scale) * (h / scale) float4 for the four low-res ones, w*h float4 for the guides
    and the output), asynchronous on `stream`, no workspace. The output must not alias an input."""
    p = _upsample_params(sigma_normal, sigma_depth)
    _check(lib().pt_upsample_device(w, h, int(scale), d_rgba_sum_lo_ptr, d_sq_sum_lo_ptr, int(spp), int(batches), d_albedo_lo_ptr,
                                    d_normal_depth_lo_ptr, d_albedo_ptr, d_normal_depth_ptr, C.byref(p), d_out_cur_ptr, stream or None),
           "pt_upsample_device")


def guide_subsample(scale, albedo, normal_depth):
    """pt_guide_subsample (host, blocking): the low-res guide of CENTRE feature buffers ([h, w, 4] float32, render_aovs_centre) at
    render scale `scale`: (albedo_lo, normal_depth_lo) = the inputs' [::scale, ::scale], which is render_aovs_centre with
    scaled_camera(cam, scale) bit for bit."""
    A, N = _f4_frames("guide_subsample", (("albedo", albedo), ("normal_depth", normal_depth)))
    h, w = A.shape[:2]
    scale = int(scale)
    lo = (h // scale, w // scale, 4) if scale > 0 else (0, 0, 4)
    Al, Nl = np.empty(lo, np.float32), np.empty(lo, np.float32)
    _check(lib().pt_guide_subsample(w, h, scale, _p(A), _p(N), _p(Al), _p(Nl)), "pt_guide_subsample")
    return Al, Nl


def guide_subsample_device(w, h, scale, d_albedo_ptr, d_normal_depth_ptr, d_out_albedo_lo_ptr, d_out_normal_depth_lo_ptr, stream=0):
    """pt_guide_subsample_device: device buffers (w*h float4 in, (w / scale) * (h / scale) float4 out), asynchronous on `stream`."""
    _check(lib().pt_guide_subsample_device(w, h, int(scale), d_albedo_ptr, d_normal_depth_ptr, d_out_albedo_lo_ptr, d_out_normal_depth_lo_ptr,
                                           stream or None), "pt_guide_subsample_device")


def denoise_hist_workspace_bytes(w, h):
    return int(lib().pt_denoise_hist_workspace_bytes(w, h))


def denoise_hist(hist, albedo, normal_depth, iterations=None, sigma_var=None, sigma_normal=None, sigma_depth=None, out=None):
    """pt_denoise_hist (host, blocking): denoise_var's filter on a history buffer of temporal_accumulate, guided by the current
    frame's albedo and normal_depth. Returns the per-pixel radiance MEAN ([h,w,4] float32, w = 0): finalise(..., 1) applies.
    `out` may be hist itself."""
    H, A, N = _f4_frames("denoise_hist", (("hist", hist), ("albedo", albedo), ("normal_depth", normal_depth)))
    return _denoise_call("denoise_hist", H, out, lambda w, h, res: lib().pt_denoise_hist(
        w, h, _p(H), _p(A), _p(N), C.byref(_denoise_var_params(iterations, sigma_var, sigma_normal, sigma_depth)), res))


def denoise_hist_device(w, h, d_hist_ptr, d_albedo_ptr, d_normal_depth_ptr, d_workspace_ptr, d_out_ptr, iterations=None, sigma_var=None,
                        sigma_normal=None, sigma_depth=None, stream=0):
    """pt_denoise_hist_device: device buffers of w*h float4 and a workspace of denoise_hist_workspace_bytes(w, h) bytes;
    asynchronous on `stream`. d_out_ptr may equal d_hist_ptr."""
    p = _denoise_var_params(iterations, sigma_var, sigma_normal, sigma_depth)
    _check(lib().pt_denoise_hist_device(w, h, d_hist_ptr, d_albedo_ptr, d_normal_depth_ptr, C.byref(p), d_workspace_ptr, d_out_ptr, stream or None),
           "pt_denoise_hist_device")


class TemporalHistory:
    """Host-side history of a w x h viewer: push() one frame after the other, each with the camera it was rendered with."""

    def __init__(self, w, h, max_history=None, depth_tol=None, normal_tol=None, respond=None):
        """respond: None (off), True (the library's respond_defaults()) or a dict of threshold / radius / power: the frames that have
        a history are blended by temporal_accumulate_respond, and self.scale holds the last frame's lambda."""
        self.w, self.h = w, h
        self.params = dict(max_history=max_history, depth_tol=depth_tol, normal_tol=normal_tol)
        self.respond = None if respond is None or respond is False else ({} if respond is True else dict(respond))
        self.reset()

    def reset(self):
        self.camera = self.normal_depth = self.hist = self.hist_len = self.scale = None

    def push(self, camera, rgba_sum, sq_sum, spp, batches, albedo, normal_depth):
        """Blend the frame into the history; returns the current hist (pass it to denoise_hist with this frame's buffers)."""
        if rgba_sum.shape != (self.h, self.w, 4):
            raise PtError("TemporalHistory: frame is %s, the history %d x %d" % (rgba_sum.shape, self.w, self.h))
        if self.respond is not None and self.hist is not None:
            self.hist, self.hist_len, self.scale = temporal_accumulate_respond(
                camera, normal_depth, rgba_sum, sq_sum, spp, batches, albedo, camera_prev=self.camera, prev_normal_depth=self.normal_depth,
                hist=self.hist, hist_len=self.hist_len, **self.params, **self.respond)
        else:
            self.hist, self.hist_len = temporal_accumulate(camera, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, self.camera,
                                                           self.normal_depth, self.hist, self.hist_len, **self.params)
        self.camera = Camera.frombytes(camera.tobytes())
        self.normal_depth = normal_depth.copy()
        return self.hist

    def push_cur(self, camera, cur, normal_depth):
        """push() for a frame given as (e, V) working pixels (upsample's output): frames of any render scale share the history."""
        if cur.shape != (self.h, self.w, 4):
            raise PtError("TemporalHistory: frame is %s, the history %d x %d" % (cur.shape, self.w, self.h))
        if self.respond is not None and self.hist is not None:
            self.hist, self.hist_len, self.scale = temporal_accumulate_respond(
                camera, normal_depth, cur=cur, camera_prev=self.camera, prev_normal_depth=self.normal_depth, hist=self.hist,
                hist_len=self.hist_len, **self.params, **self.respond)
        else:
            self.hist, self.hist_len = temporal_accumulate_cur(camera, cur, normal_depth, self.camera, self.normal_depth, self.hist,
                                                               self.hist_len, **self.params)
        self.camera = Camera.frombytes(camera.tobytes())
        self.normal_depth = normal_depth.copy()
        return self.hist


def resolve_defaults():
    """pt_resolve_defaults as a dict: tonemap, exposure."""
    p = ResolveParams()
    lib().pt_resolve_defaults(C.byref(p))
    return {f: getattr(p, f) for f, _ in ResolveParams._fields_}


def _resolve_params(tonemap, exposure):
    p = ResolveParams()
    lib().pt_resolve_defaults(C.byref(p))
    if tonemap is not None:
        p.tonemap = int(tonemap)
    if exposure is not None:
        p.exposure = exposure
    return p


def resolve(rgba, spp=0, tile_spp=None, tonemap=None, exposure=None):
    """pt_resolve (host, blocking): display bytes of a frame of radiance sums. rgba is [h,w,4] float32; it is divided by `spp`,
    or per 8x8 tile by tile_spp (int32 [ceil(h/8), ceil(w/8)], as render_adaptive returns it), painted as finalise paints NaN /
    Inf, scaled by `exposure`, tone-mapped and gamma-corrected as save_bmp does (tonemap False: clamped only) and converted to
    bytes. Returns (rgba8 [h,w,4] uint8 with alpha 255, mean [h,w,4] float32 = finalise(rgba, spp)); y = 0 stays the bottom row."""
    S, = _f4_frames("resolve", (("rgba", rgba),))
    h, w = S.shape[:2]
    T = None
    if tile_spp is not None:
        if not isinstance(tile_spp, np.ndarray) or tile_spp.dtype != np.int32 or tile_spp.shape != ((h + 7) // 8, (w + 7) // 8):
            raise PtError("resolve: tile_spp must be an int32 [%d, %d] array for a %d x %d frame" % ((h + 7) // 8, (w + 7) // 8, w, h))
        T = np.ascontiguousarray(tile_spp)
    out8, mean = np.empty((h, w, 4), np.uint8), np.empty_like(S)
    p = _resolve_params(tonemap, exposure)
    _check(lib().pt_resolve(w, h, _p(S), int(spp), _p(T), C.byref(p), _p(out8), _p(mean)), "pt_resolve")
    return out8, mean


def resolve_device(w, h, d_rgba_ptr, spp, d_rgba8_ptr, d_mean_ptr=0, d_tile_spp_ptr=0, tonemap=None, exposure=None, stream=0):
    """pt_resolve_device: device buffers (w*h float4 in, w*h*4 bytes out, optionally the w*h float4 mean and one int32 per 8x8
    tile), asynchronous on `stream`. The outputs must not alias the inputs."""
    p = _resolve_params(tonemap, exposure)
    _check(lib().pt_resolve_device(w, h, d_rgba_ptr, int(spp), d_tile_spp_ptr or None, C.byref(p), d_rgba8_ptr, d_mean_ptr or None,
                                   stream or None), "pt_resolve_device")


def select_entries(entries):
    """A pt_select_entry array from SelectEntry objects or dicts / tuples (component, lo, hi, colour (r, g, b, outline alpha), radius,
    fill_alpha); component may be "tri", "material" or "light". Returns (n, array or None)."""
    entries = list(entries or ())
    if not entries:
        return 0, None
    arr = (SelectEntry * len(entries))()
    for i, e in enumerate(entries):
        if isinstance(e, SelectEntry):
            e = (e.component, e.lo, e.hi, tuple(e.colour), e.radius, e.fill_alpha)
        elif isinstance(e, dict):
            e = tuple(e[k] for k in ("component", "lo", "hi", "colour", "radius", "fill_alpha"))
        comp, lo, hi, colour, radius, fill = e
        comp = {"tri": 0, "material": 1, "light": 2}.get(comp, comp)
        arr[i] = SelectEntry(int(comp), int(lo), int(hi), (C.c_uint8 * 4)(*[int(c) for c in colour]), int(radius), int(fill))
    return len(entries), arr


def select_overlay(ids, rgba8, entries):
    """pt_select_overlay (host, blocking): a copy of rgba8 ([h,w,4] uint8) with the selections `entries` (at most four, see
    select_entries) drawn from ids ([h,w,4] int32, render_ids' output): outline pixels blended with the entry's colour at its outline
    alpha, fill pixels at fill_alpha, the alpha byte and unselected pixels untouched."""
    if not (isinstance(ids, np.ndarray) and ids.dtype == np.int32 and ids.ndim == 3 and ids.shape[2] == 4):
        raise PtError("select_overlay: ids must be an int32 [h, w, 4] array")
    if not (isinstance(rgba8, np.ndarray) and rgba8.dtype == np.uint8 and rgba8.shape == ids.shape):
        raise PtError("select_overlay: rgba8 must be a uint8 array of ids' shape")
    h, w = ids.shape[:2]
    out = np.ascontiguousarray(rgba8).copy()
    n, arr = select_entries(entries)
    _check(lib().pt_select_overlay(w, h, _p(np.ascontiguousarray(ids)), n, arr, _p(out)), "pt_select_overlay")
    return out


def select_overlay_device(w, h, d_ids_ptr, entries, d_rgba8_ptr, stream=0):
    """pt_select_overlay_device: in place on device buffers (w*h int32x4 in, w*h*4 bytes in and out), asynchronous on `stream`."""
    n, arr = select_entries(entries)
    _check(lib().pt_select_overlay_device(w, h, d_ids_ptr or None, n, arr, d_rgba8_ptr or None, stream or None), "pt_select_overlay_device")


def preview_defaults():
    """pt_preview_defaults as a dict; temporal_params, filter_params and resolve_params are dicts themselves."""
    p = PreviewParams()
    lib().pt_preview_defaults(C.byref(p))
    sub = lambda s: {f: getattr(s, f) for f, _ in s._fields_}
    return {f: (sub(getattr(p, f)) if f.endswith("_params") else getattr(p, f)) for f, _ in PreviewParams._fields_}


class Preview:
    """pt_preview: the device buffers of one w x h viewer of `scene` (which must outlive it) and one call per frame:
    render_moments -> render_aovs -> temporal_accumulate -> denoise_hist -> resolve on the device, history and guide ping-ponged
    there (set_scale: the beauty pass at a fraction of the resolution, upsampled by the guides). Keyword arguments are pt_preview_params' fields (spp, batches, max_depth, integrator, use_mis, aov_spp, temporal,
    filter) and those of the three stages (max_history, depth_tol, normal_tol; iterations, sigma_var, sigma_normal, sigma_depth;
    tonemap, exposure); what is left out takes the library's default."""

    def __init__(self, scene, w, h, **params):
        p = PreviewParams()
        lib().pt_preview_defaults(C.byref(p))
        for k, v in params.items():
            for s in (p, p.temporal_params, p.filter_params, p.resolve_params):
                if any(k == f for f, _ in s._fields_) and not k.endswith("_params"):
                    setattr(s, k, int(v) if isinstance(v, bool) else v)
                    break
            else:
                raise PtError("Preview: unknown parameter %r" % k)
        self.w, self.h, self.temporal = w, h, bool(p.temporal)
        self._scene = scene
        self.handle = lib().pt_preview_create(scene.h if scene is not None else None, w, h, C.byref(p))
        if not self.handle:
            raise PtError("pt_preview_create failed: " + lib().pt_last_error().decode(errors="replace"))

    def frame(self, camera, seed=SEED):
        """pt_preview_frame: render and post-process one frame; blocks. The image stays on the device (read(), device_rgba8())."""
        _check(lib().pt_preview_frame(self.handle, C.byref(camera), seed), "pt_preview_frame")
        return self

    def reset(self):
        """Drop the history: the next frame is a first frame."""
        _check(lib().pt_preview_reset(self.handle), "pt_preview_reset")
        return self

    def scene_changed(self, keep_history=False):
        """pt_preview_scene_changed: the scene was updated (Scene.update_mesh / update_vertices) since the last frame. The next
        frame renders every tile and traces its guide again; keep_history False also drops the history (as reset does), True
        blends into it where depth and normal still validate. Without this call a session that finds the scene's generation
        changed behaves as with keep_history False."""
        _check(lib().pt_preview_scene_changed(self.handle, 1 if keep_history else 0), "pt_preview_scene_changed")
        return self

    def set_scale(self, scale):
        """pt_preview_set_scale: the frames that follow render their beauty pass at 1 / scale of the size in each axis (1..8, a
        divisor of w and h) and upsample it with the full-resolution guides; 1 is the full-resolution frame. History carries over."""
        _check(lib().pt_preview_set_scale(self.handle, int(scale)), "pt_preview_set_scale")
        return self

    @property
    def scale(self):
        return lib().pt_preview_scale(self.handle)

    def set_guide_chain(self, max_links):
        """pt_preview_set_guide_chain: the frames that follow take their guides from render_aovs_chain(max_links) (1..16) in place of
        render_aovs (0, the default). A call that changes the value drops the history, as reset() does."""
        _check(lib().pt_preview_set_guide_chain(self.handle, int(max_links)), "pt_preview_set_guide_chain")
        return self

    @property
    def guide_chain(self):
        return lib().pt_preview_guide_chain(self.handle)

    def set_guide_centre(self, on):
        """pt_preview_set_guide_centre: the frames that follow trace their guides through pixel centres (render_aovs_centre with the
        guide chain's max_links), take a scaled frame's low-res guide by guide_subsample, and launch no feature pass while the camera
        rests. A call that changes the value drops the history, as reset() does."""
        _check(lib().pt_preview_set_guide_centre(self.handle, int(on)), "pt_preview_set_guide_centre")
        return self

    @property
    def guide_centre(self):
        return lib().pt_preview_guide_centre(self.handle)

    def set_motion(self, on):
        """pt_preview_set_motion: with 1, the frame after one announced update_vertices that keeps its history (scene_changed(True))
        also traces Scene.render_motion and accumulates through temporal_accumulate[_cur]_motion, so surfaces that moved keep their
        history. Off by default; changing it does not reset the session."""
        _check(lib().pt_preview_set_motion(self.handle, int(on)), "pt_preview_set_motion")
        return self

    @property
    def motion(self):
        return lib().pt_preview_motion(self.handle)

    def set_motion_chain(self, on):
        """pt_preview_set_motion_chain: with 1, a motion frame (set_motion(1)) of a session with a guide chain traces
        Scene.render_motion_chain along that chain in place of render_motion, so a moved object seen in a mirror or through glass
        keeps its history too; with centre guides that one pass also writes the frame's guide. Off by default; changing it does not
        reset the session."""
        _check(lib().pt_preview_set_motion_chain(self.handle, int(on)), "pt_preview_set_motion_chain")
        return self

    @property
    def motion_chain(self):
        return lib().pt_preview_motion_chain(self.handle)

    def set_respond(self, threshold=None, radius=None, power=None):
        """pt_preview_set_respond: the frames that follow and have a history (converging frames excepted) accumulate through
        temporal_accumulate_respond, so a static surface whose lighting changed shortens its own history. A None parameter takes the
        library default (respond_defaults()); set_respond(False) turns it off, which is a session's initial state. Changing it does
        not reset the session."""
        if threshold is False:
            _check(lib().pt_preview_set_respond(self.handle, None), "pt_preview_set_respond")
            return self
        p = _respond_params(threshold, radius, power)
        _check(lib().pt_preview_set_respond(self.handle, C.byref(p)), "pt_preview_set_respond")
        return self

    def respond(self):
        """pt_preview_respond: the option's parameters as a dict (radius, power, threshold), or None while it is off."""
        p = RespondParams()
        r = lib().pt_preview_respond(self.handle, C.byref(p))
        _check(min(r, 0), "pt_preview_respond")
        return {f: getattr(p, f) for f, _ in RespondParams._fields_} if r == 1 else None

    @property
    def guide_passes(self):
        """pt_preview_guide_passes: feature-pass launches of all good frames since the session was created."""
        return lib().pt_preview_guide_passes(self.handle)

    def set_selection(self, entries=(), max_links=0):
        """pt_preview_set_selection: the frames that follow end with select_overlay(entries) on their rgba8, drawn from the session's
        own ID buffer (render_ids(the frame's camera, max_links) at display size, traced again only when the camera, the scene or
        max_links changed). No entries turns it off, which is a session's initial state. Nothing but rgba8 changes, and the session
        is not reset."""
        n, arr = select_entries(entries)
        _check(lib().pt_preview_set_selection(self.handle, n, arr, int(max_links)), "pt_preview_set_selection")
        return self

    def pick(self, x, y, max_links=0):
        """pt_preview_pick: Scene.pick of one pixel with the last good frame's camera at display size: (ids [4] int32, hit [4] float32)."""
        ids, hit = np.zeros(4, np.int32), np.zeros(4, np.float32)
        _check(lib().pt_preview_pick(self.handle, int(x), int(y), int(max_links), _p(ids), _p(hit)), "pt_preview_pick")
        return ids, hit

    def read_ids(self):
        """pt_preview_read_ids: the session's ID buffer, [h,w,4] int32."""
        ids = np.empty((self.h, self.w, 4), np.int32)
        _check(lib().pt_preview_read_ids(self.handle, _p(ids)), "pt_preview_read_ids")
        return ids

    def device_ids(self):
        """Device address of the w*h int32x4 ID buffer (None before the first selection; valid until close())."""
        return lib().pt_preview_device_ids(self.handle)

    @property
    def id_passes(self):
        """pt_preview_id_passes: ID-pass launches of all good frames since the session was created."""
        return lib().pt_preview_id_passes(self.handle)

    def set_converge(self, threshold=None, min_history=None):
        """pt_preview_set_converge: while the camera rests, the frames that follow render only the 8x8 tiles whose history has
        not converged (temporal_select's rule) and carry the others forward. threshold 0 (or False) turns it off, None takes the
        library default; off is a session's initial state."""
        if threshold is False:
            _check(lib().pt_preview_set_converge(self.handle, None), "pt_preview_set_converge")
            return self
        p = _converge_params(threshold, min_history)
        _check(lib().pt_preview_set_converge(self.handle, C.byref(p)), "pt_preview_set_converge")
        return self

    def last_live(self):
        """pt_preview_last_live: (live tiles, all tiles) of the last good frame; they are equal on a frame that did not converge."""
        live, total = C.c_int(-1), C.c_int(-1)
        _check(lib().pt_preview_last_live(self.handle, C.byref(live), C.byref(total)), "pt_preview_last_live")
        return live.value, total.value

    def read_tiles(self):
        """pt_preview_read_tiles: (tile_err float32, tile_live int32), both [ceil(h/8), ceil(w/8)], of the last converging frame."""
        ty, tx = (self.h + 7) // 8, (self.w + 7) // 8
        err, live = np.empty((ty, tx), np.float32), np.empty((ty, tx), np.int32)
        _check(lib().pt_preview_read_tiles(self.handle, _p(err), _p(live)), "pt_preview_read_tiles")
        return err, live

    def read(self, rgba8=True, mean=True, hist=None, hist_len=None):
        """pt_preview_read: the last good frame's outputs as a dict of the requested arrays: rgba8 [h,w,4] uint8, mean [h,w,4]
        float32, hist [h,w,4] float32 and hist_len [h,w] float32 (the last two by default exactly when the session is temporal)."""
        want = {"rgba8": rgba8, "mean": mean, "hist": self.temporal if hist is None else hist,
                "hist_len": self.temporal if hist_len is None else hist_len}
        shapes = {"rgba8": ((self.h, self.w, 4), np.uint8), "mean": ((self.h, self.w, 4), np.float32),
                  "hist": ((self.h, self.w, 4), np.float32), "hist_len": ((self.h, self.w), np.float32)}
        out = {k: np.empty(*shapes[k]) for k, v in want.items() if v}
        _check(lib().pt_preview_read(self.handle, *[_p(out.get(k)) for k in ("rgba8", "mean", "hist", "hist_len")]), "pt_preview_read")
        return out

    def device_rgba8(self):
        """Device address of the w*h*4 display bytes (valid until close(); holds the last good frame)."""
        return lib().pt_preview_device_rgba8(self.handle)

    def device_mean(self):
        return lib().pt_preview_device_mean(self.handle)

    def stats(self):
        """pt_preview_last_stats: good frames since creation and the last one's stage times in milliseconds."""
        st = PreviewStats()
        _check(lib().pt_preview_last_stats(self.handle, C.byref(st)), "pt_preview_last_stats")
        return {f: getattr(st, f) for f, _ in PreviewStats._fields_}

    def close(self):
        if self.handle:
            lib().pt_preview_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grid_desc(lo, hi, counts, sh_samples, map_res=0, map_samples=1, power=3):
    """A pt_grid_desc: the grid of rays.sh_grid(lo, hi, counts), the samples Scene.query_sh spent on a probe (lanes * spp_lane), and,
    for a grid with distance maps, Scene.query_distance's res and spp_lane and the exponent of the Chebyshev test."""
    d = GridDesc()
    d.lo[:], d.hi[:], d.counts[:] = [float(v) for v in lo], [float(v) for v in hi], [int(v) for v in counts]
    d.sh_samples, d.map_res, d.map_samples, d.power = int(sh_samples), int(map_res), int(map_samples), int(power)
    return d


def grid_packed_bytes(desc):
    """pt_grid_packed_bytes: the size of the packed buffer of a grid, or PtError for a desc the library refuses."""
    n = int(lib().pt_grid_packed_bytes(C.byref(desc)))
    if not n:
        _check(-1, "pt_grid_packed_bytes")
    return n


def _is_tensor(a):
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def _grid_input(what, name, a, words, like=None):
    """A float32 input of `words` words: a C-contiguous numpy array for the host form, or, with `like` a tensor, a contiguous tensor
    on its device for the device form."""
    if like is not None:
        import torch
        if not (_is_tensor(a) and a.is_cuda and a.device == like.device and a.dtype == torch.float32 and a.is_contiguous()):
            raise PtError("%s: %s must be a contiguous float32 tensor on %s" % (what, name, like.device))
        if a.device.index != torch.cuda.current_device():
            raise PtError("%s: %s is on %s but the current device is %d" % (what, name, a.device, torch.cuda.current_device()))
        got = a.numel()
    else:
        if _is_tensor(a):
            raise PtError("%s: %s is a tensor but the call's other arrays are numpy" % (what, name))
        a = np.ascontiguousarray(a, np.float32)
        got = a.size
    if got != words:
        raise PtError("%s: %s holds %d float32 words, the grid needs %d" % (what, name, got, words))
    return a


def grid_pack(desc, coeff_sums, maps=None):
    """pt_grid_pack: Scene.query_sh's sums [n, 9, 4] and, for a grid with maps (desc.map_res = R), Scene.query_distance's maps
    [n, R, R, 4] of the n probes of rays.sh_grid, as the packed buffer grid_irradiance reads: a 1-D float32 array of
    grid_packed_bytes(desc) / 4 words. numpy in, numpy out (host form); torch tensors on the current HIP device in, a tensor out, on
    torch's current stream with no host copy."""
    words = grid_packed_bytes(desc) // 4
    n, r = desc.counts[0] * desc.counts[1] * desc.counts[2], desc.map_res
    if (maps is None) != (r == 0):
        raise PtError("grid_pack: maps are %s but desc.map_res is %d" % ("missing" if maps is None else "given", r))
    like = coeff_sums if _is_tensor(coeff_sums) else None
    s = _grid_input("grid_pack", "coeff_sums", coeff_sums, n * 36, like)
    m = None if maps is None else _grid_input("grid_pack", "maps", maps, n * r * r * 4, like)
    if like is not None:
        import torch
        packed = torch.empty(words, dtype=torch.float32, device=s.device)
        _check(lib().pt_grid_pack_device(C.byref(desc), s.data_ptr(), m.data_ptr() if m is not None else None, packed.data_ptr(),
                                         torch.cuda.current_stream(s.device).cuda_stream or None), "pt_grid_pack_device")
    else:
        packed = np.zeros(words, np.float32)
        _check(lib().pt_grid_pack(C.byref(desc), _p(s), _p(m), _p(packed)), "pt_grid_pack")
    return packed


def _grid_words(what, name, a, count, like=None, writable=False):
    """`count` 32-bit integer words (probe numbers, state words): for the host form a C-contiguous int32 or uint32 numpy array (one
    that is written must be the caller's own array, not a copy), or, with `like` a tensor, a contiguous int32 tensor on its device
    (torch's 32-bit integer type; a state word's bits are the same)."""
    if like is not None:
        import torch
        if not (_is_tensor(a) and a.is_cuda and a.device == like.device and a.dtype == torch.int32 and a.is_contiguous()):
            raise PtError("%s: %s must be a contiguous int32 tensor on %s" % (what, name, like.device))
        got = a.numel()
    else:
        if _is_tensor(a):
            raise PtError("%s: %s is a tensor but the call's other arrays are numpy" % (what, name))
        if writable:
            if not (isinstance(a, np.ndarray) and a.dtype in (np.uint32, np.int32) and a.flags.c_contiguous and a.flags.writeable):
                raise PtError("%s: %s must be a writable C-contiguous uint32 array" % (what, name))
        else:
            a = np.asarray(a)
            a = np.ascontiguousarray(a if a.dtype in (np.uint32, np.int32) else a.astype(np.int32))
        got = a.size
    if got != count:
        raise PtError("%s: %s holds %d words, the call needs %d" % (what, name, got, count))
    return a


def _grid_list(what, desc, indices, like):
    """(k, indices or None) of a probe list: None is the identity over the grid's n probes."""
    n = desc.counts[0] * desc.counts[1] * desc.counts[2]
    if indices is None:
        return n, None
    k = int(indices.numel()) if _is_tensor(indices) else int(np.asarray(indices).size)
    return k, _grid_words(what, "indices", indices, k, like)


def _ptr(a):
    return None if a is None else (a.data_ptr() if _is_tensor(a) else _p(a))


def grid_classify(desc, maps, back_fraction=0.25, indices=None, states=None):
    """pt_grid_classify: a state word per probe from Scene.query_distance's maps [k, R, R, 4] of the probes `indices` [k] (None: all n,
    in the grid's order). PROBE_INSIDE where the hits seen from behind pass back_fraction of the hits, PROBE_IDLE where nothing was
    hit. Writes the listed probes' words of `states` [n] (a zeroed array when None; uint32 numpy for the host form, an int32 tensor
    for the device form) and returns it. numpy in, numpy out; tensors on the current HIP device in, a tensor out, on torch's current
    stream."""
    like = maps if _is_tensor(maps) else None
    n, r = desc.counts[0] * desc.counts[1] * desc.counts[2], desc.map_res
    k, idx = _grid_list("grid_classify", desc, indices, like)
    mp = _grid_input("grid_classify", "maps", maps, k * r * r * 4, like)
    if like is not None:
        import torch
        if states is None:
            states = torch.zeros(n, dtype=torch.int32, device=mp.device)
        st = _grid_words("grid_classify", "states", states, n, like)
        _check(lib().pt_grid_classify_device(C.byref(desc), k, _ptr(idx), _ptr(mp), back_fraction, _ptr(st),
                                             torch.cuda.current_stream(mp.device).cuda_stream or None), "pt_grid_classify_device")
    else:
        if states is None:
            states = np.zeros(n, np.uint32)
        st = _grid_words("grid_classify", "states", states, n, writable=True)
        _check(lib().pt_grid_classify(C.byref(desc), k, _ptr(idx), _ptr(mp), back_fraction, _ptr(st)), "pt_grid_classify")
    return st


def grid_update(packed, desc, coeff_sums, maps=None, hysteresis=0.0, indices=None):
    """pt_grid_update: blends fresh query outputs into grid_pack's buffer in place and returns it. coeff_sums [k, 9, 4] and, for a
    grid with maps, maps [k, R, R, 4] are Scene.query_sh's and Scene.query_distance's rows for the probes `indices` [k] (None: all n);
    desc carries the FRESH rows' sample counts. Each word becomes fresh + hysteresis * (old - fresh); hysteresis 0 replaces it.
    numpy (packed a C-contiguous float32 array, written where it lies) or tensors on the current HIP device, on torch's current
    stream."""
    like = packed if _is_tensor(packed) else None
    r = desc.map_res
    if (maps is None) != (r == 0):
        raise PtError("grid_update: maps are %s but desc.map_res is %d" % ("missing" if maps is None else "given", r))
    if like is None and not (isinstance(packed, np.ndarray) and packed.dtype == np.float32 and packed.flags.c_contiguous and packed.flags.writeable):
        raise PtError("grid_update: packed must be a writable C-contiguous float32 array: it is updated in place")
    pk = _grid_input("grid_update", "packed", packed, grid_packed_bytes(desc) // 4, like)
    k, idx = _grid_list("grid_update", desc, indices, like)
    s = _grid_input("grid_update", "coeff_sums", coeff_sums, k * 36, like)
    m = None if maps is None else _grid_input("grid_update", "maps", maps, k * r * r * 4, like)
    if like is not None:
        import torch
        _check(lib().pt_grid_update_device(C.byref(desc), k, _ptr(idx), _ptr(s), _ptr(m), hysteresis, _ptr(pk),
                                           torch.cuda.current_stream(pk.device).cuda_stream or None), "pt_grid_update_device")
    else:
        _check(lib().pt_grid_update(C.byref(desc), k, _ptr(idx), _ptr(s), _ptr(m), hysteresis, _ptr(pk)), "pt_grid_update")
    return packed


def grid_relocate_defaults(desc, min_dist=None, max_offset=None):
    """(min_dist, max_offset) as grid_relocate uses them: what is given, and for a None 0.2 of the smallest cell step and, per axis,
    0.45 of its step (on an axis with one probe 0.45 of the smallest step of the others). A grid of one probe has no step: PtError
    unless both are given."""
    if min_dist is not None and max_offset is not None:
        return min_dist, max_offset
    steps = [(float(np.float32(desc.hi[a])) - float(np.float32(desc.lo[a]))) / (desc.counts[a] - 1) if desc.counts[a] > 1 else None for a in range(3)]
    have = [v for v in steps if v is not None]
    if not have:
        raise PtError("grid_relocate: a grid of one probe has no cell: give min_dist and max_offset")
    return (0.2 * min(have) if min_dist is None else min_dist,
            [0.45 * (v if v is not None else min(have)) for v in steps] if max_offset is None else max_offset)


def grid_relocate(desc, maps, offsets=None, back_fraction=0.25, min_dist=None, max_offset=None, indices=None):
    """pt_grid_relocate: an offset per probe from Scene.query_distance's maps [k, R, R, 4] of the probes `indices` [k] (None: all n, in
    the grid's order). A probe that grid_classify's rule finds inside moves out through its nearest back face by the face's distance
    plus min_dist / 2; a probe nearer than min_dist to a front face steps back to min_dist; every offset is clamped to +-max_offset
    (three numbers, or one for all axes). Writes the listed probes' rows of `offsets` [n, 4] float32 (zeros when None: dx, dy, dz and
    what was done, 0 kept, 1 pushed out, 2 pushed off) and returns it. numpy in, numpy out (host form, `offsets` written where it
    lies); tensors on the current HIP device in, a tensor out, on torch's current stream. The defaults are grid_relocate_defaults'."""
    like = maps if _is_tensor(maps) else None
    n, r = desc.counts[0] * desc.counts[1] * desc.counts[2], desc.map_res
    min_dist, max_offset = grid_relocate_defaults(desc, min_dist, max_offset)
    mx = np.ascontiguousarray(np.broadcast_to(np.asarray(max_offset, np.float32).reshape(-1), (3,)))
    k, idx = _grid_list("grid_relocate", desc, indices, like)
    mp = _grid_input("grid_relocate", "maps", maps, k * r * r * 4, like)
    if like is not None:
        import torch
        if offsets is None:
            offsets = torch.zeros((n, 4), dtype=torch.float32, device=mp.device)
        off = _grid_input("grid_relocate", "offsets", offsets, n * 4, like)
        _check(lib().pt_grid_relocate_device(C.byref(desc), k, _ptr(idx), _ptr(mp), back_fraction, min_dist, _p(mx), _ptr(off),
                                             torch.cuda.current_stream(mp.device).cuda_stream or None), "pt_grid_relocate_device")
    else:
        if offsets is None:
            offsets = np.zeros((n, 4), np.float32)
        if not (isinstance(offsets, np.ndarray) and offsets.dtype == np.float32 and offsets.flags.c_contiguous and offsets.flags.writeable):
            raise PtError("grid_relocate: offsets must be a writable C-contiguous float32 array: it is updated in place")
        off = _grid_input("grid_relocate", "offsets", offsets, n * 4)
        _check(lib().pt_grid_relocate(C.byref(desc), k, _ptr(idx), _ptr(mp), back_fraction, min_dist, _p(mx), _ptr(off)), "pt_grid_relocate")
    return offsets


def grid_irradiance(packed, desc, records, states=None, offsets=None):
    """pt_grid_irradiance: the irradiance at surface points from a packed probe grid. records is [m, 8] float32 (point, a word that
    is not read, unit normal, a word that is not read: rays.irradiance_records, rays.records_from_surfaces); packed is grid_pack's
    buffer of the same desc. Returns [m, 4] float32: (E_r, E_g, E_b, W) in rays.grid_irradiance's units, W the weight sum E was
    divided by; exact zeros for a record whose point or normal is not finite. numpy in, numpy out (host form); tensors on the
    current HIP device in, a tensor out, on torch's current stream with no host copy. With `states` [n] (grid_classify's)
    pt_grid_irradiance_states: the probes whose PROBE_INSIDE bit is set are left out. With `offsets` [n, 4] (grid_relocate's)
    pt_grid_irradiance_offsets: probe j stands at its grid position + offsets[j, :3]; with states or without."""
    is_torch, r, m = Scene._query_rays("grid_irradiance", records)
    like = r if is_torch else None
    p = _grid_input("grid_irradiance", "packed", packed, grid_packed_bytes(desc) // 4, like)
    n = desc.counts[0] * desc.counts[1] * desc.counts[2]
    st = None
    if states is not None:
        st = _grid_words("grid_irradiance", "states", states, n, like)
    off = None
    if offsets is not None:
        off = _grid_input("grid_irradiance", "offsets", offsets, n * 4, like)
    # the entry point and the arrays it takes after the packed buffer: offsets go with states or without
    if off is not None:
        name, extra = "pt_grid_irradiance_offsets", (st, off)
    elif st is not None:
        name, extra = "pt_grid_irradiance_states", (st,)
    else:
        name, extra = "pt_grid_irradiance", ()
    if is_torch:
        import torch
        out = torch.empty((m, 4), dtype=torch.float32, device=r.device)
        if m:
            _check(getattr(lib(), name + "_device")(C.byref(desc), _ptr(p), *map(_ptr, extra), m, _ptr(r), _ptr(out),
                                                    torch.cuda.current_stream(r.device).cuda_stream or None), name + "_device")
    else:
        out = np.zeros((m, 4), np.float32)
        _check(getattr(lib(), name)(C.byref(desc), _ptr(p), *map(_ptr, extra), m, _ptr(r), _ptr(out)), name)
    return out


class ProbeGrid:
    """A baked probe volume over a scene: the SH probes and distance maps of a rays.sh_grid(lo, hi, counts), packed for lookups.

        grid = ProbeGrid(sc, lo, hi, (8, 8, 8)).bake(256, 4, 8, map_spp=4)
        e = grid.shade(sc.query_closest(sc.query_camera_rays(cam, w, h), surfaces=True)[1])[:, :3]

    res is the distance maps' resolution (4, 8, 16 or 32), or 0 for a grid without maps (a plain trilinear mix); max_t the distance
    the maps clamp at, by default 1.5 diagonals of a grid cell. With device=True the queries, the pack and the buffers stay on the
    current HIP device as torch tensors; otherwise they are numpy and lookups take numpy."""

    def __init__(self, scene, lo, hi, counts, res=8, max_t=None, device=False):
        self.scene, self.lo, self.hi, self.counts = scene, [float(v) for v in lo], [float(v) for v in hi], [int(c) for c in counts]
        self.res, self.device = int(res), bool(device)
        cell = [(b - a) / (c - 1) for a, b, c in zip(self.lo, self.hi, self.counts) if c > 1]
        self.max_t = float(max_t) if max_t is not None else 1.5 * float(np.sqrt(sum(v * v for v in cell)))
        self.desc = self.sums = self.maps = self.packed = self.states = self.offsets = None
        self.back_fraction = 0.25
        self.relocate_rounds = 0

    def _where(self):
        if not self.device:
            return None
        import torch
        return "cuda:%d" % torch.cuda.current_device()

    def bake(self, lanes, spp_lane, max_depth, map_spp=1, power=3, seed=SEED, integrator=UNIDIRECTIONAL, use_mis=True, map_flags=0):
        """Scene.query_sh (lanes x spp_lane samples a probe, paths of max_depth) and, with maps, Scene.query_distance (map_spp samples
        a texel, flags map_flags) on the grid's records, then grid_pack. Keeps the sums, the maps and the packed buffer; returns self."""
        from . import rays
        self.sums = self.scene.query_sh(rays.sh_grid(self.lo, self.hi, self.counts, device=self._where()), lanes, spp_lane, max_depth, integrator, use_mis, seed)
        self.maps = None
        if self.res:
            self.maps = self.scene.query_distance(rays.sh_grid(self.lo, self.hi, self.counts, self.max_t, self._where()), self.res, map_spp, seed,
                                                  flags=map_flags)
        self.desc = grid_desc(self.lo, self.hi, self.counts, lanes * spp_lane, self.res, map_spp, power)
        self.packed = grid_pack(self.desc, self.sums, self.maps)
        self.states = self.offsets = None
        return self

    def classify(self, back_fraction=0.25):
        """grid_classify on the kept maps: keeps a state word per probe in .states (PROBE_INSIDE, PROBE_IDLE), which the lookups pass
        from then on, so that a probe inside an object lights nothing. bake() forgets them. Returns self."""
        if self.packed is None:
            raise PtError("ProbeGrid: bake() has not run")
        if not self.res:
            raise PtError("ProbeGrid: a grid without maps (res = 0) has nothing to classify")
        self.back_fraction = float(back_fraction)
        self.states = grid_classify(self.desc, self.maps, self.back_fraction)
        return self

    def update(self, lanes, spp_lane, max_depth, map_spp=1, hysteresis=0.9, probes=None, seed=SEED, skip_idle=False, integrator=UNIDIRECTIONAL,
               use_mis=True, map_flags=0):
        """Re-bakes the probes `probes` (numbers in the grid's order; default: all) and blends the fresh samples into the packed buffer
        in place: new = fresh + hysteresis * (old - fresh). The queries run as bake()'s with QUERY_STREAM_PAD, each record's pad word
        its probe number, so a listed probe gets the streams a full bake with these arguments gives it. With skip_idle the probes that
        classify() found PROBE_IDLE are dropped from the list. The fresh rows replace the listed probes' rows of .sums and .maps, and
        where states are kept the listed probes are classified again from their fresh maps. Where offsets are kept (relocate()) the
        records are built at grid position + offset (rays.sh_grid builds them on the host: a device grid's offsets are copied to the
        host for it, once per query). Returns self."""
        from . import rays
        if self.packed is None:
            raise PtError("ProbeGrid: bake() has not run")
        n = self.counts[0] * self.counts[1] * self.counts[2]
        idx = np.arange(n, dtype=np.int32) if probes is None else np.asarray(probes, np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= n):
            raise PtError("ProbeGrid.update: probe numbers must be in 0..%d" % (n - 1))
        idx = idx.astype(np.int32)
        if skip_idle and self.states is not None:
            st = self.states.cpu().numpy() if _is_tensor(self.states) else self.states
            idx = idx[(st[idx].astype(np.int64) & PROBE_IDLE) == 0]
        if not len(idx):
            return self
        where = self._where()

        def records(max_t):
            rec = rays.sh_grid(self.lo, self.hi, self.counts, max_t, where, offsets=self.offsets)
            if where is None:
                rec = np.ascontiguousarray(rec[idx])
                rec.view(np.int32)[:, 7] = idx
            else:
                import torch
                t = torch.from_numpy(idx).to(rec.device)
                rec = rec[t.long()].contiguous()
                rec.view(torch.int32)[:, 7] = t
            return rec
        sums = self.scene.query_sh(records(QUERY_MAX_T), lanes, spp_lane, max_depth, integrator, use_mis, seed, flags=QUERY_STREAM_PAD)
        maps = None
        if self.res:
            maps = self.scene.query_distance(records(self.max_t), self.res, map_spp, seed, flags=map_flags | QUERY_STREAM_PAD)
        desc = grid_desc(self.lo, self.hi, self.counts, lanes * spp_lane, self.res, map_spp, self.desc.power)
        if where is None:
            lst, at = idx, idx
        else:
            import torch
            lst = torch.from_numpy(idx).to(sums.device)
            at = lst.long()
        grid_update(self.packed, desc, sums, maps, hysteresis, lst)
        self.sums[at] = sums
        if maps is not None:
            self.maps[at] = maps
            if self.states is not None:
                grid_classify(desc, maps, self.back_fraction, lst, self.states)
        return self

    def relocate(self, lanes, spp_lane, max_depth, map_spp=1, min_dist=None, max_offset=None, iterations=4, seed=SEED, integrator=UNIDIRECTIONAL,
                 use_mis=True, map_flags=0):
        """Moves the probes out of the way, at most `iterations` rounds: grid_relocate on the kept maps (back_fraction is classify()'s),
        then the probes whose offset changed are re-baked at grid position + offset through update(hysteresis=0, probes=moved) with
        these sample counts, which also classifies them again where states are kept; a round in which nothing moved ends the loop.
        Keeps the offsets in .offsets ([n, 4]), which lookup(), irradiance(), shade() and update() read from then on, and the number of
        rounds that ran grid_relocate in .relocate_rounds; bake() forgets the offsets. The defaults of min_dist and max_offset are
        grid_relocate_defaults'. Returns self."""
        if self.packed is None:
            raise PtError("ProbeGrid: bake() has not run")
        if not self.res:
            raise PtError("ProbeGrid: a grid without maps (res = 0) has nothing to relocate by")
        if int(map_spp) != self.desc.map_samples:
            raise PtError("ProbeGrid.relocate: map_spp %d is not the kept maps' %d: their means would mix" % (map_spp, self.desc.map_samples))
        min_dist, max_offset = grid_relocate_defaults(self.desc, min_dist, max_offset)
        self.relocate_rounds = 0
        for _ in range(int(iterations)):
            before = None if self.offsets is None else (self.offsets.clone() if _is_tensor(self.offsets) else self.offsets.copy())
            self.offsets = grid_relocate(self.desc, self.maps, self.offsets, self.back_fraction, min_dist, max_offset)
            self.relocate_rounds += 1
            now = self.offsets[:, :3]
            changed = (now != (before[:, :3] if before is not None else 0 * now)).any(1)
            moved = (changed.nonzero().reshape(-1).cpu().numpy() if _is_tensor(changed) else np.flatnonzero(changed)).astype(np.int32)
            if not len(moved):
                break
            self.update(lanes, spp_lane, max_depth, map_spp, 0.0, moved, seed, False, integrator, use_mis, map_flags)
        return self

    def lookup(self, records):
        """grid_irradiance on the baked grid: [m, 4] (E_r, E_g, E_b, W) for [m, 8] records; with the states classify() keeps and the
        offsets relocate() keeps."""
        if self.packed is None:
            raise PtError("ProbeGrid: bake() has not run")
        return grid_irradiance(self.packed, self.desc, records, self.states, self.offsets)

    def irradiance(self, points, normals):
        """The lookup at `points` [m, 3] with unit `normals` [m, 3]."""
        from . import rays
        return self.lookup(rays.irradiance_records(points, normals, device=self._where()))

    def shade(self, surfaces):
        """The lookup at Scene.query_closest(..., surfaces=True)'s surfaces (rays.records_from_surfaces). A ray that missed has the
        record (0, 0, 0), normal (0, 0, 1) and is looked up there: mask it by its material word."""
        from . import rays
        return self.lookup(rays.records_from_surfaces(surfaces))


def adaptive_params(min_spp, max_spp, chunk_spp, threshold):
    """pt_adaptive_params from Python numbers (the library checks the values)."""
    return AdaptiveParams(int(min_spp), int(max_spp), int(chunk_spp), float(threshold))


def adaptive_mean(colors, tile_spp):
    """Per-pixel mean of an adaptive frame: colors [h,w,4] float32 (the sums render_adaptive returns) divided by the sample
    count of the pixel's tile, one IEEE f32 division per channel. Pass the result to denoise(..., spp=1)."""
    if not isinstance(colors, np.ndarray) or colors.dtype != np.float32 or colors.ndim != 3 or colors.shape[2] != 4:
        raise PtError("adaptive_mean: colors must be a float32 [h, w, 4] array")
    h, w = colors.shape[:2]
    if not isinstance(tile_spp, np.ndarray) or tile_spp.dtype != np.int32 or tile_spp.shape != ((h + 7) // 8, (w + 7) // 8):
        raise PtError("adaptive_mean: tile_spp must be an int32 [%d, %d] array for a %d x %d frame" % ((h + 7) // 8, (w + 7) // 8, w, h))
    if (tile_spp <= 0).any():
        raise PtError("adaptive_mean: every tile needs at least one sample")
    n = np.repeat(np.repeat(tile_spp, 8, axis=0), 8, axis=1)[:h, :w].astype(np.float32)
    return colors / n[..., None]


def untile_device(w, h, d_tiles_ptr, d_colors_ptr, tiles=None, stream=0):
    _check(lib().pt_untile_device(w, h, C.byref(tiles) if tiles is not None else None, d_tiles_ptr, d_colors_ptr, stream or None), "pt_untile_device")


def tile_device(w, h, d_colors_ptr, d_tiles_ptr, tiles=None, stream=0):
    _check(lib().pt_tile_device(w, h, C.byref(tiles) if tiles is not None else None, d_colors_ptr, d_tiles_ptr, stream or None), "pt_tile_device")


def n_tiles(w, h):
    return ((w + 7) // 8) * ((h + 7) // 8)


def rank_tiles(w, h, rank, world):
    """Interleaved tile ownership: rank r renders tiles {t : t mod world == r} (pt_rank_tiles)."""
    tr = TileRange()
    lib().pt_rank_tiles(w, h, rank, world, C.byref(tr))
    return tr


def probe_rng(subsequences, n_draws, seed=SEED):
    sub = np.ascontiguousarray(subsequences, np.uint32)
    n = len(sub)
    st = np.zeros((n, 6), np.uint32); u = np.zeros((n, max(n_draws, 1)), np.uint32); f = np.zeros((n, max(n_draws, 1)), np.float32)
    _check(lib().pt_probe_rng(seed, n, _p(sub), n_draws, _p(st), _p(u), _p(f)), "pt_probe_rng")
    return st, u[:, :n_draws], f[:, :n_draws]


def probe_adaptive_moments(w, h, live, reps=20):
    """pt_probe_adaptive_moments: the mean time in ms of render_adaptive_moments' bookkeeping pass on `live` tiles of a w x h frame."""
    ms = C.c_float(0.0)
    _check(lib().pt_probe_adaptive_moments(w, h, live, reps, C.byref(ms)), "pt_probe_adaptive_moments")
    return float(ms.value)


def probe_math(x):
    x = np.ascontiguousarray(x, np.float32)
    outs = [np.zeros_like(x) for _ in range(5)]
    _check(lib().pt_probe_math(x.size, _p(x), *[_p(o) for o in outs]), "pt_probe_math")
    return dict(zip(("sin", "cos", "exp", "rsqrt", "pow5"), outs))


def probe_rcp_exhaustive():
    """pt_probe_rcp_exhaustive: {mismatches, in_fast_range, bare_sequence_wrong_outside_range, first_bad} over all 2^32 inputs."""
    out = np.zeros(3, np.uint64)
    first = np.zeros(1, np.uint32)
    _check(lib().pt_probe_rcp_exhaustive(_p(out), _p(first)), "pt_probe_rcp_exhaustive")
    return {"mismatches": int(out[0]), "in_fast_range": int(out[1]), "bare_wrong_outside": int(out[2]), "first_bad": int(first[0])}


def probe_camera_rays(camera, xy, seed=SEED):
    xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    out = np.zeros((len(xy), 6), np.float32)
    _check(lib().pt_probe_camera_rays(C.byref(camera), seed, len(xy), _p(xy), _p(out)), "pt_probe_camera_rays")
    return out


def probe_centre_rays(camera, xy):
    """pt_probe_centre_rays: the centre rays of render_aovs_centre, [n, 6] float32 (o, d); no seed, none is read."""
    xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    out = np.zeros((len(xy), 6), np.float32)
    _check(lib().pt_probe_centre_rays(C.byref(camera), len(xy), _p(xy), _p(out)), "pt_probe_centre_rays")
    return out


def query_camera_rays(camera, w, h, max_t=QUERY_MAX_T, out=None):
    """pt_query_camera_rays_device: ray y*w + x = the centre ray of pixel (x, y) (probe_centre_rays' o and d bit for bit) with the
    given max_t, as an [h*w, 8] float32 torch tensor on the current device (or into `out`, such a tensor), on torch's current stream."""
    import torch
    if out is None:
        out = torch.empty((max(w, 0) * max(h, 0), 8), dtype=torch.float32, device="cuda:%d" % torch.cuda.current_device())
    _check(lib().pt_query_camera_rays_device(C.byref(camera), w, h, max_t, out.data_ptr() or None, torch.cuda.current_stream(out.device).cuda_stream or None),
           "pt_query_camera_rays_device")
    return out
