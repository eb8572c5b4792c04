"""The C ABI of include/mirt.h restated for ctypes: the structs, the constants, and one table of every entry point's
signature.  tests/test_binding_header.py parses the header and holds all three to it, so an entry that disagrees (c_int where
the header says int64_t) fails a CPU test instead of truncating an argument on its way to a kernel launch.

Needs ctypes and os only: torch is imported when the library is loaded, numpy not at all.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MIRT_LIB: load another build of the same library (tools/ab.py builds A/B variants next to the default one)
LIB_PATH = os.environ.get("MIRT_LIB") or os.path.join(HERE, "_build", "libmirt.so")

# MirtStatus
MIRT_OK, MIRT_ERR_IO, MIRT_ERR_PARSE, MIRT_ERR_ARG, MIRT_ERR_HIP, MIRT_ERR_NO_DEVICE, MIRT_ERR_STATE = 0, 1, 2, 3, 4, 5, 6
MIRT_RENDER_COUNTERS = 1
MIRT_HIT_NONE, MIRT_HIT_SPHERE, MIRT_HIT_TRIANGLE, MIRT_HIT_PLANE = 0, 1, 2, 3
MIRT_QUERY_ANY_HIT = 1
MIRT_MULTI_MAX_GPUS = 16
# Defaults of the filter's three scales (DESIGN.md section 6f has the table of mean squared errors against converged frames they
# were chosen from)
MIRT_DENOISE_SIGMA_C = 1.0
MIRT_DENOISE_SIGMA_N = 0.03
MIRT_DENOISE_SIGMA_P = 0.1


class MirtError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"libmirt status {status}: {message}")
        self.status = status
        self.message = message


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def tolist(self):
        return [self.x, self.y, self.z]


class Ray(C.Structure):
    """MirtRay: one row of a float32 [n, 8] ray tensor (pack_rays)."""
    _fields_ = [("o", Vec3), ("tmax", C.c_float), ("d", Vec3), ("pad", C.c_float)]


class Hit(C.Structure):
    """MirtHit: one row of a 4-byte [n, 6] hit tensor (unpack_hits)."""
    _fields_ = [("t", C.c_float), ("kind", C.c_uint32), ("id", C.c_uint32), ("n", Vec3)]


class Camera(C.Structure):
    """MirtCamera: the camera fields of a scene (RawConfig.camera / set_camera)."""
    _fields_ = [("eye", Vec3), ("forward", Vec3), ("right", Vec3), ("up", Vec3),
                ("dof_focus", C.c_float), ("dof_lens", C.c_float), ("fisheye", C.c_int32), ("panorama", C.c_int32)]


class Shading(C.Structure):
    """MirtShading: bounces, gi and expose of a scene (RawConfig.shading / set_shading); expose +inf = exposure off."""
    _fields_ = [("bounces", C.c_int32), ("gi", C.c_int32), ("expose", C.c_float)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("bounces", C.c_int32), ("aa", C.c_int32),
        ("dof_focus", C.c_float), ("dof_lens", C.c_float),
        ("forward", Vec3), ("right", Vec3), ("up", Vec3), ("eye", Vec3),
        ("expose", C.c_float),
        ("fisheye", C.c_int32), ("panorama", C.c_int32), ("gi", C.c_int32),
        ("num_spheres", C.c_int32), ("num_triangles", C.c_int32), ("num_prims", C.c_int32),
        ("num_planes", C.c_int32), ("num_suns", C.c_int32), ("num_bulbs", C.c_int32),
        ("spheres", C.c_void_p), ("triangles", C.c_void_p), ("prim_refs", C.c_void_p),
        ("planes", C.c_void_p), ("suns", C.c_void_p), ("bulbs", C.c_void_p),
    ]


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32),
                ("stripe_rows", C.c_int32), ("num_parts", C.c_int32), ("part", C.c_int32), ("flags", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "rays", "shadow_rays", "internal_visits", "sphere_tests",
                                          "tri_tests", "mat_fetches", "max_stack", "overflow_events")] + \
               [("trace_kernel_ms", C.c_float), ("render_ms", C.c_float), ("build_ms", C.c_float), ("num_nodes", C.c_int32),
                ("trace_kernel_ms_mean", C.c_float), ("frames_timed", C.c_int32), ("trace_launches", C.c_int32), ("node_record_bytes", C.c_int32),
                ("rays_traversed", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MultiStats(C.Structure):
    _fields_ = [("num_gpus", C.c_int32), ("build_ms", C.c_float), ("render_ms", C.c_float * MIRT_MULTI_MAX_GPUS),
                ("gather_ms", C.c_float), ("frame_ms", C.c_float)]


class TreeNode(C.Structure):
    _fields_ = [("xmin", C.c_float), ("xmax", C.c_float), ("ymin", C.c_float), ("ymax", C.c_float),
                ("zmin", C.c_float), ("zmax", C.c_float),
                ("left", C.c_uint32), ("right", C.c_uint32), ("prim_offset", C.c_uint32), ("count", C.c_uint32)]


class RecordInfo(C.Structure):
    """MirtRecordInfo: the element counts of mirt_get_records' regions, and what decodes a child reference."""
    _fields_ = [(n, C.c_uint32) for n in ("num_nodes", "num_qnodes", "num_wnodes", "prim_units", "num_tris_before", "num_tri_boxes", "num_qparams",
                                          "prim_base16", "qnode_base16", "wnode_base16", "root_ref", "root_ref_q", "root_ref_w")] + \
               [("grid_ok", C.c_int32), ("tree_depth", C.c_int32), ("coord_max", C.c_float)]


class SampleOrderInfo(C.Structure):
    """MirtSampleOrderInfo: the lengths of mirt_get_sample_order's arrays."""
    _fields_ = [("total_samples", C.c_int64), ("last_launch_samples", C.c_int64)]


# The header's struct behind each class, for the test that compares them field by field
STRUCTS = {"MirtVec3": Vec3, "MirtRay": Ray, "MirtHit": Hit, "MirtCamera": Camera, "MirtShading": Shading, "MirtSceneDesc": SceneDesc,
           "MirtRenderParams": RenderParams, "MirtStats": Stats, "MirtMultiStats": MultiStats, "MirtTreeNode": TreeNode,
           "MirtRecordInfo": RecordInfo, "MirtSampleOrderInfo": SampleOrderInfo}

_int, _i64, _u32, _u64, _f, _str, _vp = C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_char_p, C.c_void_p
_out = C.POINTER
_params, _camera, _shading, _desc = _out(RenderParams), _out(Camera), _out(Shading), _out(SceneDesc)

# symbol -> (restype, argtypes): every entry point of include/mirt.h, in the header's order.  A handle, a device pointer, a
# host array and a stream are all void*.
SIGNATURES = {
    "mirt_last_error": (_str, []),
    "mirt_version": (_int, []),
    "mirt_parse_scene_file": (_int, [_str, _out(_vp)]),
    "mirt_parse_scene_text": (_int, [_str, C.c_size_t, _out(_vp)]),
    "mirt_synthetic_scene": (_int, [_u64, _int, _int, _out(_vp)]),
    "mirt_host_scene_destroy": (None, [_vp]),
    "mirt_host_scene_desc": (_int, [_vp, _desc]),
    "mirt_host_scene_filename": (_str, [_vp]),
    "mirt_scene_create": (_int, [_desc, _int, _out(_vp)]),
    "mirt_scene_destroy": (None, [_vp]),
    "mirt_scene_set_option": (_int, [_vp, _str, _int]),
    "mirt_scene_get_option": (_int, [_vp, _str, _out(_int)]),
    "mirt_build_lbvh": (_int, [_vp, _vp, _out(_f)]),
    "mirt_render_num_pixels": (_i64, [_params]),
    "mirt_render": (_int, [_vp, _params, _vp, _vp, _vp]),
    "mirt_render_accumulate": (_int, [_vp, _params, _vp, _int, _int, _vp]),
    "mirt_finalize": (_int, [_params, _vp, _int, _vp, _vp]),
    "mirt_render_accumulate_pixels": (_int, [_vp, _params, _vp, _i64, _vp, _vp, _vp, _int, _int, _vp]),
    "mirt_select_pixels": (_int, [_params, _vp, _vp, _vp, _int, _int, _f, _vp, _vp, _vp]),
    "mirt_finalize_counts": (_int, [_params, _vp, _vp, _vp, _vp]),
    "mirt_part_pixel_xy": (_int, [_params, _i64, _out(C.c_int32), _out(C.c_int32)]),
    "mirt_scatter_part": (_int, [_params, _vp, _vp, _vp]),
    "mirt_trace_rays": (_int, [_vp, _vp, _i64, _vp, _u32, _vp]),
    "mirt_camera_rays": (_int, [_vp, _params, _vp, _vp]),
    "mirt_hit_features": (_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "mirt_denoise_work_bytes": (C.c_size_t, [_params]),
    "mirt_denoise": (_int, [_params, _vp, _vp, _vp, _vp, _int, _f, _f, _f, _vp, _vp, _vp]),
    "mirt_scene_get_camera": (_int, [_vp, _camera]),
    "mirt_scene_set_camera": (_int, [_vp, _camera]),
    "mirt_scene_update_spheres": (_int, [_vp, _vp, _int, _int, _vp]),
    "mirt_scene_update_triangles": (_int, [_vp, _vp, _int, _int, _vp]),
    "mirt_scene_get_spheres": (_int, [_vp, _int, _int, _vp, _vp]),
    "mirt_scene_get_triangles": (_int, [_vp, _int, _int, _vp, _vp]),
    "mirt_scene_get_lights": (_int, [_vp, _vp, _vp]),
    "mirt_scene_set_lights": (_int, [_vp, _vp, _vp, _vp]),
    "mirt_scene_get_planes": (_int, [_vp, _int, _int, _vp]),
    "mirt_scene_set_planes": (_int, [_vp, _vp, _int, _int, _vp]),
    "mirt_make_plane": (_int, [_vp, _vp, _vp]),
    "mirt_scene_get_shading": (_int, [_vp, _shading]),
    "mirt_scene_set_shading": (_int, [_vp, _shading]),
    "mirt_scene_update_sphere_materials": (_int, [_vp, _vp, _int, _int, _vp]),
    "mirt_scene_update_triangle_materials": (_int, [_vp, _vp, _int, _int, _vp]),
    "mirt_scene_get_sphere_materials": (_int, [_vp, _int, _int, _vp, _vp]),
    "mirt_scene_get_triangle_materials": (_int, [_vp, _int, _int, _vp, _vp]),
    "mirt_prev_features": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "mirt_temporal_accumulate": (_int, [_params, _camera] + [_vp] * 8 + [_int, _f, _f] + [_vp] * 4),
    "mirt_multi_create": (_int, [_desc, _int, _out(_int), _out(_vp)]),
    "mirt_multi_destroy": (None, [_vp]),
    "mirt_multi_num_parts": (_int, [_vp]),
    "mirt_multi_set_option": (_int, [_vp, _str, _int]),
    "mirt_multi_set_camera": (_int, [_vp, _camera]),
    "mirt_multi_set_lights": (_int, [_vp, _vp, _vp]),
    "mirt_multi_set_planes": (_int, [_vp, _vp, _int, _int]),
    "mirt_multi_set_shading": (_int, [_vp, _shading]),
    "mirt_multi_submit": (_int, [_vp, _int, _int, _int, _int, _vp, _out(_u64)]),
    "mirt_multi_wait": (_int, [_vp, _u64, _out(MultiStats)]),
    "mirt_render_frame_multi": (_int, [_vp, _int, _int, _int, _int, _vp, _out(MultiStats)]),
    "mirt_render_frames_multi": (_int, [_vp, _int, _int, _int, _int, _int, _int, _vp, _out(MultiStats), _out(_f)]),
    "mirt_multi_get_stats": (_int, [_vp, _int, _out(Stats)]),
    "mirt_get_stats": (_int, [_vp, _out(Stats)]),
    "mirt_get_tree": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "mirt_get_records": (_int, [_vp, _out(RecordInfo)] + [_vp] * 8),
    "mirt_probe_math": (_int, [_int, _int, _int, _vp, _vp]),
    "mirt_probe_xorwow": (_int, [_int, _int, _int, _int, _vp]),
    "mirt_probe_qbox": (_int, [_int, _int, _vp, _vp]),
    "mirt_probe_sort": (_int, [_int, _int, _int, _vp, _vp, _vp]),
    "mirt_probe_sched": (_int, [_int, _int, _int, _vp, _vp]),
    "mirt_get_sample_order": (_int, [_vp, _out(SampleOrderInfo), _vp, _vp, _vp]),
    "mirt_write_png": (_int, [_str, _vp, _int, _int]),
}
EXPORTS = list(SIGNATURES)

_lib = None


def lib():
    """Load libmirt.so (fails loudly if it has not been built: `python -m cuda_ray_tracer_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MirtError(-1, f"{LIB_PATH} not found: build it with `python -m cuda_ray_tracer_amd.build` "
                            "(there is no fallback implementation)")
    try:
        import torch  # noqa: F401  (loads the process-wide HIP runtime first so both share one instance)
    except Exception:
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (restype, argtypes) in SIGNATURES.items():
        # (a build that predates an entry point -- MIRT_LIB A/B runs -- still loads: the missing symbol raises AttributeError
        # where it is first called)
        f = getattr(L, name, None)
        if f is not None:
            f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


_applied = {}      # id of an extension's signature table -> the library it was last applied to


def extension_lib(signatures):
    """lib() with an extension header's table (symbol -> (restype, argtypes)) applied, once per loaded library.  A library
    without one of its symbols is an error here: there is no other implementation."""
    L = lib()
    if _applied.get(id(signatures)) is not L:
        for name, (restype, argtypes) in signatures.items():
            f = getattr(L, name, None)
            if f is None:
                raise MirtError(-1, f"{LIB_PATH} does not export {name}: rebuild it with `python -m cuda_ray_tracer_amd.build`")
            f.restype, f.argtypes = restype, argtypes
        _applied[id(signatures)] = L
    return L


def _check(rc):
    if rc != MIRT_OK:
        raise MirtError(rc, lib().mirt_last_error().decode("utf-8", "replace"))
