"""ctypes binding of libuob_rt.so (include/uob_rt.h) for tests and bench.py.

The library is the product; this module is plumbing.  There is no CPU fallback: if the shared library
cannot be loaded, or no HIP device is present when a context is created, the call raises.
"""
import ctypes as C
import os

import numpy as np

# Two HIP runtimes can end up in one process: torch ships its own libamdhip64, libuob_rt.so links the system's.  Loaded in
# the order torch -> libuob_rt.so both work; the other order ends in "No HIP GPUs are available" from torch.  So: if torch
# is installed, it is imported here, before lib() can load the library (torch is plumbing for tests and bench.py; the
# library itself needs none of it).
try:
    import torch as _torch  # noqa: F401
except ImportError:          # a host without torch: nothing to order
    _torch = None

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UOB_RT_LIB", os.path.join(_HERE, "libuob_rt.so"))   # override: kernel experiments only

EXPORTS = (
    "rt_abi_version", "rt_last_error", "rt_config_default", "rt_config_owned_rows", "rt_init", "rt_render",
    "rt_render_device", "rt_count_work", "rt_count_executed", "rt_last_kernel_ms", "rt_destroy", "rt_scene_cornell_box",
    "rt_scene_load_obj", "rt_scene_load_obj_ex", "rt_triangle_compute_normal", "rt_scene_pack", "rt_rotation_matrix",
    "rt_selftest_rcp", "rt_selftest_normalize", "rt_selftest_shade", "rt_selftest_all_within", "rt_debug_trace_rays", "rt_debug_block_costs", "rt_debug_world_masks", "rt_debug_wave_timeline", "rt_debug_wave_seeds", "rt_debug_wave_seeds_wide", "rt_register_output", "rt_unregister_output",
    "rt_debug_band_copy_plan", "rt_update_scene", "rt_update_scene_device", "rt_debug_tile_data",
    "rt_trace_rays", "rt_trace_rays_device", "rt_debug_trace_stats",
    "rt_render_aov", "rt_render_aov_device", "rt_debug_aov_stats",
    "rt_shade_points", "rt_shade_points_device", "rt_debug_shade_stats",
    "rt_radiance_rays", "rt_radiance_rays_device", "rt_debug_radiance_stats",
    "rt_replace_scene", "rt_replace_scene_device", "rt_update_spheres", "rt_debug_scene_capacity",
    "rt_scene_transform", "rt_set_objects", "rt_pose_objects", "rt_pose_objects_device", "rt_debug_object_count",
    "rt_debug_scene_data",
    "rt_scene_skin", "rt_set_skin", "rt_pose_skin", "rt_pose_skin_device", "rt_debug_skin_info",
    "rt_debug_live_device_objects",
    "rt_filter_params_default", "rt_filter_plane", "rt_filter_plane_device", "rt_debug_filter_stats", "rt_filter_plane_host",
    "rt_filter_variance_params_default", "rt_filter_plane_variance", "rt_filter_plane_variance_device",
    "rt_filter_plane_variance_host",
    "rt_accumulate_params_default", "rt_accumulate_plane", "rt_accumulate_plane_device", "rt_debug_accumulate_stats",
    "rt_accumulate_plane_host",
    "rt_motion_snapshot", "rt_motion_release", "rt_debug_motion_info", "rt_motion_planes", "rt_motion_planes_device",
    "rt_motion_planes_host", "rt_debug_motion_stats",
    "rt_accumulate_plane_moving", "rt_accumulate_plane_moving_device", "rt_accumulate_plane_moving_host",
)

# rt_debug_live_device_objects slots
LIVE_OBJECT_KEYS = ("allocations", "bytes", "events", "streams")

# rt_debug_trace_stats slots (include/uob_rt.h)
TRACE_STATS_KEYS = ("rays", "waves", "tiles", "bundle_tiles", "tested_tiles", "triangle_tests", "unculled_rays", "reserved")
# rt_debug_aov_stats slots
AOV_STATS_KEYS = ("samples", "waves", "tiles", "mask_tiles", "tested_tiles", "triangle_tests", "reserved6", "reserved7")

# rt_debug_shade_stats slots
SHADE_STATS_KEYS = ("points", "sample_rays", "waves", "tiles", "bundle_tiles", "tested_tiles", "triangle_tests", "skipped_points")

# rt_debug_radiance_stats slots
RADIANCE_STATS_KEYS = ("rays", "bounce_rays", "shaded_points", "sample_rays", "closest_tested_tiles", "closest_triangle_tests",
                       "shadow_triangle_tests", "unculled_rays")

# rt_debug_filter_stats slots
FILTER_STATS_KEYS = ("pixels", "passes", "accepted_taps", "valid_pixels", "kept", "reserved5", "reserved6", "reserved7")
# the same slots after a variance-guided call (rt_filter_plane_variance): slot 5 counts the taps that its value stop alone rejected
FILTER_VARIANCE_STATS_KEYS = FILTER_STATS_KEYS[:5] + ("variance_stopped",) + FILTER_STATS_KEYS[6:]

# rt_debug_accumulate_stats slots
ACCUMULATE_STATS_KEYS = ("pixels", "valid_pixels", "found_history", "accepted_taps", "no_candidate", "reserved5", "reserved6",
                         "reserved7")

# rt_debug_motion_stats slots
MOTION_STATS_KEYS = ("elements", "valid_elements", "moved", "unmoved", "copied", "prim_out_of_range", "reserved6", "reserved7")

_lib = None


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libuob_rt: error %d: %s" % (code, msg))
        self.code = code


# one tile-seed record (include/uob_rt.h rt_debug_wave_seeds): 64 bytes
SEED_DTYPE = np.dtype([("D0", "<f4", 3), ("ed", "<f4"), ("K", "<u8"), ("Kh", "<u8"), ("Kp", "<u8"), ("h", "<i4"), ("flags", "<u4"),
                       ("pad", "<u4", 4)])
SEED_PRIMARY, SEED_SHADOW = 1, 2
# rt_debug_wave_seeds_wide: the bits the draw kernel reads, and its counters (tiles_<key>, jobs_<key> in this order)
SEED_PRIMARY_WIDE, SEED_PRIMARY_SPH, SEED_SHADOW_WIDE, SEED_SHADOW_SPH, SEED_SHADOW_BLOCKED = 4, 8, 16, 32, 64
SEED_WIDE_KEYS = ("primary", "shadow", "casters", "sphere", "blocked")


def lib():
    """Load libuob_rt.so (built by __graft_entry__.build() / make -C uob_raytracer_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        fp, vp = C.POINTER(C.c_float), C.c_void_p
        L.rt_last_error.restype = C.c_char_p
        L.rt_config_default.argtypes = [C.POINTER(abi.RtConfig)]
        L.rt_config_default.restype = None
        L.rt_config_owned_rows.argtypes = [C.POINTER(abi.RtConfig)]
        L.rt_init.argtypes = [C.POINTER(abi.RtConfig), fp, fp, fp, C.c_int32, C.POINTER(vp)]
        L.rt_update_scene.argtypes = [vp, fp, fp, fp, C.c_int32, C.c_uint32]
        L.rt_update_scene_device.argtypes = [vp, vp, vp, vp, C.c_int32, C.c_uint32, vp]
        L.rt_debug_tile_data.argtypes = [vp, C.POINTER(C.c_int32), fp, C.c_int32]
        L.rt_debug_scene_data.argtypes = [vp, fp, fp, fp, fp, fp, fp, C.POINTER(C.c_int32), fp, fp, C.c_int32]
        L.rt_replace_scene.argtypes = [vp, fp, fp, fp, C.c_int32, C.c_uint32]
        L.rt_replace_scene_device.argtypes = [vp, vp, vp, vp, C.c_int32, C.c_uint32, vp]
        L.rt_update_spheres.argtypes = [vp, C.POINTER(abi.RtSphere), C.c_int32]
        L.rt_debug_scene_capacity.argtypes = [vp, C.POINTER(C.c_int64)]
        L.rt_scene_transform.argtypes = [C.POINTER(abi.RtTriangle), C.c_int32, C.c_int32, C.c_int32, fp]
        L.rt_scene_transform.restype = None
        L.rt_set_objects.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]
        L.rt_pose_objects.argtypes = [vp, fp, C.c_uint32]
        L.rt_pose_objects_device.argtypes = [vp, vp, C.c_uint32, vp]
        L.rt_debug_object_count.argtypes = [vp, C.POINTER(C.c_int32)]
        L.rt_scene_skin.argtypes = [C.POINTER(abi.RtTriangle), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint16), fp, fp,
                                    C.c_int32]
        L.rt_scene_skin.restype = None
        L.rt_set_skin.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_uint16), fp, C.c_int32]
        L.rt_pose_skin.argtypes = [vp, fp, C.c_uint32]
        L.rt_pose_skin_device.argtypes = [vp, vp, C.c_uint32, vp]
        L.rt_debug_skin_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.rt_debug_live_device_objects.argtypes = [C.POINTER(C.c_int64)]
        L.rt_render.argtypes = [vp, fp, fp, fp, C.c_float, C.POINTER(C.c_uint32), fp]
        L.rt_render_device.argtypes = [vp, fp, fp, fp, C.c_float, vp, vp, vp]
        L.rt_count_work.argtypes = [vp, fp, fp, fp, C.c_float, C.POINTER(abi.RtWork)]
        L.rt_count_executed.argtypes = [vp, fp, fp, fp, C.c_float, C.POINTER(C.c_uint64)]
        L.rt_last_kernel_ms.argtypes = [vp, fp]
        L.rt_destroy.argtypes = [vp]
        L.rt_destroy.restype = None
        L.rt_scene_cornell_box.argtypes = [C.POINTER(abi.RtTriangle), C.c_int32]
        L.rt_scene_load_obj.argtypes = [C.c_char_p, C.POINTER(abi.RtTriangle), C.c_int32]
        L.rt_scene_load_obj_ex.argtypes = [C.c_char_p, fp, C.c_float, fp, C.POINTER(abi.RtTriangle), C.c_int32]
        L.rt_debug_trace_rays.argtypes = [vp, C.c_int32, fp, fp, C.c_int64, C.POINTER(C.c_int32), fp]
        L.rt_trace_rays.argtypes = [vp, C.c_int32, fp, fp, C.c_int64, C.POINTER(C.c_int32), fp]
        L.rt_trace_rays_device.argtypes = [vp, C.c_int32, vp, vp, C.c_int64, vp, vp, vp]
        L.rt_debug_trace_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_render_aov.argtypes = [vp, fp, fp, C.c_float, C.c_int32, C.POINTER(abi.RtAovBuffers)]
        L.rt_render_aov_device.argtypes = [vp, fp, fp, C.c_float, C.c_int32, C.POINTER(abi.RtAovBuffers), vp]
        L.rt_debug_aov_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_shade_points.argtypes = [vp, fp, C.POINTER(C.c_int32), C.c_int64, fp, fp, C.POINTER(C.c_int32)]
        L.rt_shade_points_device.argtypes = [vp, vp, vp, C.c_int64, fp, vp, vp, vp]
        L.rt_debug_shade_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_radiance_rays.argtypes = [vp, fp, C.POINTER(C.c_int32), C.c_int64, fp, fp, C.POINTER(C.c_int32)]
        L.rt_radiance_rays_device.argtypes = [vp, vp, vp, C.c_int64, fp, vp, vp, vp]
        L.rt_debug_radiance_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_filter_params_default.argtypes = [C.POINTER(abi.RtFilterParams), C.c_int32, C.c_int32]
        L.rt_filter_params_default.restype = None
        L.rt_filter_plane.argtypes = [vp, C.POINTER(abi.RtFilterParams), fp, fp, fp, fp]
        L.rt_filter_plane_device.argtypes = [vp, C.POINTER(abi.RtFilterParams), vp, vp, vp, vp, vp]
        L.rt_debug_filter_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_filter_plane_host.argtypes = [C.POINTER(abi.RtFilterParams), fp, fp, fp, fp]
        fvp = C.POINTER(abi.RtFilterVarianceParams)
        L.rt_filter_variance_params_default.argtypes = [fvp, C.c_int32, C.c_int32]
        L.rt_filter_variance_params_default.restype = None
        L.rt_filter_plane_variance.argtypes = [vp, fvp, fp, fp, fp, fp, fp, fp]
        L.rt_filter_plane_variance_device.argtypes = [vp, fvp, vp, vp, vp, vp, vp, vp, vp]
        L.rt_filter_plane_variance_host.argtypes = [fvp, fp, fp, fp, fp, fp, fp]
        ap, ip = C.POINTER(abi.RtAccumulateParams), C.POINTER(C.c_int32)
        L.rt_accumulate_params_default.argtypes = [ap, C.c_int32, C.c_int32]
        L.rt_accumulate_params_default.restype = None
        L.rt_accumulate_plane.argtypes = [vp, ap, fp, fp, fp, ip, fp, fp, fp, fp]
        L.rt_accumulate_plane_device.argtypes = [vp, ap] + [vp] * 9
        L.rt_debug_accumulate_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_accumulate_plane_host.argtypes = [ap, fp, fp, fp, ip, fp, fp, fp, fp]
        L.rt_motion_snapshot.argtypes = [vp, vp]
        L.rt_motion_release.argtypes = [vp]
        L.rt_debug_motion_info.argtypes = [vp, ip]
        L.rt_motion_planes.argtypes = [vp, ip, fp, fp, C.c_int64, fp, fp]
        L.rt_motion_planes_device.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, vp]
        L.rt_motion_planes_host.argtypes = [fp, fp, fp, C.c_int32, ip, fp, fp, C.c_int64, fp, fp]
        L.rt_debug_motion_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_accumulate_plane_moving.argtypes = [vp, ap, fp, fp, fp, ip, fp, fp, fp, fp, fp, fp]
        L.rt_accumulate_plane_moving_device.argtypes = [vp, ap] + [vp] * 11
        L.rt_accumulate_plane_moving_host.argtypes = [ap, fp, fp, fp, ip, fp, fp, fp, fp, fp, fp]
        L.rt_debug_block_costs.argtypes = [vp, C.POINTER(C.c_uint32), C.c_int32]
        L.rt_debug_world_masks.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.rt_debug_wave_timeline.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_debug_band_copy_plan.argtypes = [C.c_int32] * 9 + [C.POINTER(abi.RtBandCopy), C.c_int32]
        L.rt_register_output.argtypes = [vp, vp, C.c_size_t]
        L.rt_unregister_output.argtypes = [vp]
        L.rt_triangle_compute_normal.argtypes = [C.POINTER(abi.RtTriangle)]
        L.rt_triangle_compute_normal.restype = None
        L.rt_scene_pack.argtypes = [C.POINTER(abi.RtTriangle), C.c_int32, fp, fp, fp]
        L.rt_scene_pack.restype = None
        L.rt_rotation_matrix.argtypes = [C.c_float, C.c_float, fp]
        L.rt_rotation_matrix.restype = None
        if L.rt_abi_version() != abi.RT_ABI_VERSION:
            raise ImportError("libuob_rt.so ABI %d != binding %d" % (L.rt_abi_version(), abi.RT_ABI_VERSION))
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise RtError(rc, lib().rt_last_error().decode(errors="replace"))
    return rc


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _rays6(a):
    """Caller rays (or points with normals) as a C-contiguous float32 [k, 6] array."""
    return np.ascontiguousarray(a, np.float32).reshape(-1, 6)


def _light3(a):
    """The light position as the library takes it: a float32 [3] array of its own."""
    return np.ascontiguousarray(a, np.float32)[:3].copy()


def _need(name, t, dtype, shape, dev):
    """A tensor argument of a *_device method: a contiguous torch tensor of that dtype and shape on the context's device."""
    if not isinstance(t, _torch.Tensor):
        raise TypeError("%s must be a torch tensor" % name)
    if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s (got %s %s on %s)"
                         % (name, dtype, shape, dev, t.dtype, tuple(t.shape), t.device))


def _out(name, t, dtype, shape, dev):
    """An output tensor of a *_device method: allocated when None, and a tensor argument like any other (_need)."""
    if t is None:
        t = _torch.empty(shape, dtype=dtype, device=dev)
    _need(name, t, dtype, shape, dev)
    return t


def _rows(name, t, cols, dev):
    """The k of a float32 [k, cols] input tensor of a *_device method (_need)."""
    if not isinstance(t, _torch.Tensor) or t.dim() != 2:
        raise ValueError("%s must be a torch tensor of shape [k, %d]" % (name, cols))
    _need(name, t, _torch.float32, (t.shape[0], cols), dev)
    return t.shape[0]


def _guide_tensors(value, position4, normal4, dev):
    """The input planes of a filter or accumulate call on the device: value float32 [h, w], the guides [h, w, 4] -> (h, w)."""
    if not isinstance(value, _torch.Tensor) or value.dim() != 2:
        raise ValueError("value must be a torch tensor of shape [height, width]")
    h, w = value.shape
    _need("value", value, _torch.float32, (h, w), dev)
    _need("position4", position4, _torch.float32, (h, w, 4), dev)
    _need("normal4", normal4, _torch.float32, (h, w, 4), dev)
    return h, w


def _seeds_ptr(seeds, k, what):
    """The optional seeds of a blocking shade / radiance call as the int32 pointer the C ABI takes (None: no seeds)."""
    if seeds is None:
        return None
    seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1)
    if seeds.shape[0] != k:
        raise ValueError("seeds must have one entry per %s" % what)
    return seeds.ctypes.data_as(C.POINTER(C.c_int32))     # (the pointer object keeps the array alive)


def band_copy_plan(num_devices, k, device_band_rows, width, height, elem_bytes, dev_to_dev, peer_ok, same_device):
    """The copies that deliver device k's bands of a multi-device context (rt_debug_band_copy_plan): list of dicts."""
    n = _check(lib().rt_debug_band_copy_plan(num_devices, k, device_band_rows, width, height, elem_bytes, int(dev_to_dev),
                                             int(peer_ok), int(same_device), None, 0))
    buf = (abi.RtBandCopy * max(n, 1))()
    _check(lib().rt_debug_band_copy_plan(num_devices, k, device_band_rows, width, height, elem_bytes, int(dev_to_dev),
                                         int(peer_ok), int(same_device), buf, n))
    return [{f: int(getattr(buf[i], f)) for f, _ in abi.RtBandCopy._fields_ if f != "reserved"} for i in range(n)]


def live_device_objects():
    """Device objects the library holds in this process right now (rt_debug_live_device_objects): dict of LIVE_OBJECT_KEYS."""
    out = (C.c_int64 * 4)()
    _check(lib().rt_debug_live_device_objects(out))
    return {key: int(out[i]) for i, key in enumerate(LIVE_OBJECT_KEYS)}


def selftest_rcp():
    """All-2^32-patterns check of the exact reciprocal (include/uob_rt.h rt_selftest_rcp)."""
    out = (C.c_uint64 * 64)()
    _check(lib().rt_selftest_rcp(out))
    v = list(out)
    return {"safe_mismatch_1step": v[0], "safe_mismatch_2step": v[1], "edge_mismatch_1step": v[2],
            "edge_mismatch_2step": v[3], "examples": [int(b) & 0xFFFFFFFF for b in v[8:8 + min(v[4], 56)]]}


def selftest_normalize(b_stride=64):
    """normalize()'s square root over every FP32 pattern and its quotients over every significand of a and every
    b_stride-th significand of b (include/uob_rt.h rt_selftest_normalize)."""
    out = (C.c_uint64 * 8)()
    _check(lib().rt_selftest_normalize(out, C.c_uint32(b_stride)))
    v = list(out)
    return {"sqrt_mismatches": v[0], "div_mismatches": v[1], "div_pairs": v[2], "sqrt_example": v[3], "div_example": v[4]}


def selftest_shade(ns, lit, secondary, unshadowed, term, col, straight_line=False):
    """The kernels' shade() on caller-given lanes, one wave of 64 per entry of ns (include/uob_rt.h rt_selftest_shade):
    lit, secondary, unshadowed, term [nwaves, 64], col [nwaves, 64, 4] -> float32 [nwaves, 64, 3]."""
    ns = np.ascontiguousarray(ns, np.int32).reshape(-1)
    w = ns.shape[0]
    ints = [np.ascontiguousarray(a, np.int32).reshape(w, 64) for a in (lit, secondary, unshadowed)]
    term = np.ascontiguousarray(term, np.float32).reshape(w, 64)
    col = np.ascontiguousarray(col, np.float32).reshape(w, 64, 4)
    out = np.zeros((w, 64, 3), np.float32)
    _check(lib().rt_selftest_shade(w, _ip(ns), _ip(ints[0]), _ip(ints[1]), _ip(ints[2]), _fp(term), _fp(col),
                                   int(bool(straight_line)), _fp(out)))
    return out


def selftest_all_within(lane_in, v, bound):
    """The wave kernel's all_within() beside the wave reduction it stands for, one wave of 64 per entry of bound (include/uob_rt.h
    rt_selftest_all_within): lane_in, v [nwaves, 64] -> (all_within's answers, the reduction's answers), bool [nwaves] each."""
    bound = np.ascontiguousarray(bound, np.float32).reshape(-1)
    w = bound.shape[0]
    lane_in = np.ascontiguousarray(lane_in, np.int32).reshape(w, 64)
    v = np.ascontiguousarray(v, np.float32).reshape(w, 64)
    out = np.zeros((w, 2), np.int32)
    _check(lib().rt_selftest_all_within(w, _ip(lane_in), _fp(v), _fp(bound), _ip(out)))
    return out[:, 0] != 0, out[:, 1] != 0


def filter_params(width, height, passes=None, normal_min_dot=None, plane_eps=None, value_max_diff=None):
    """rt_filter_params of a width x height plane: rt_filter_params_default's values (5 passes, 0.9, 0.01, +inf) unless given."""
    p = abi.RtFilterParams()
    lib().rt_filter_params_default(C.byref(p), int(width), int(height))
    for key, v in (("passes", passes), ("normal_min_dot", normal_min_dot), ("plane_eps", plane_eps), ("value_max_diff", value_max_diff)):
        if v is not None:
            setattr(p, key, v)
    return p


def _host_planes(value, position4, normal4):
    """The input planes of a blocking filter or accumulate call: value a numpy [h, w] array, the guides [h, w, 4] -> (h, w,
    and the three as C-contiguous float32 arrays)."""
    if not isinstance(value, np.ndarray) or value.ndim != 2:
        raise ValueError("value must be a numpy array of shape [height, width]")
    h, w = value.shape
    v = np.ascontiguousarray(value, np.float32)
    pos = np.ascontiguousarray(position4, np.float32)
    nrm = np.ascontiguousarray(normal4, np.float32)
    if pos.shape != (h, w, 4) or nrm.shape != (h, w, 4):
        raise ValueError("position4 and normal4 must have the shape [%d, %d, 4]" % (h, w))
    return h, w, v, pos, nrm


def _filter_host_planes(value, position4, normal4, out):
    """The numpy planes of a blocking filter call: _host_planes' inputs; out None, `value` itself (in place) or another
    C-contiguous float32 [h, w] array."""
    h, w, v, pos, nrm = _host_planes(value, position4, normal4)
    if out is value and not (value.dtype == np.float32 and value.flags.c_contiguous and value.flags.writeable):
        raise ValueError("in place, value must be a writeable C-contiguous float32 array")
    if out is None:
        out = np.empty((h, w), np.float32)
    elif out is value:
        out = v
    elif not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != (h, w) or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 array of shape (%d, %d)" % (h, w))
    return h, w, v, pos, nrm, out


def filter_plane_host(value, position4, normal4, out=None, **params):
    """The a-trous filter on the host (rt_filter_plane_host; needs no device): value float32 [h, w], position4 / normal4
    float32 [h, w, 4] -> float32 [h, w].  params: passes, normal_min_dot, plane_eps, value_max_diff (filter_params).
    out=value filters in place."""
    h, w, v, pos, nrm, out = _filter_host_planes(value, position4, normal4, out)
    p = filter_params(w, h, **params)
    _check(lib().rt_filter_plane_host(C.byref(p), _fp(v), _fp(pos), _fp(nrm), _fp(out)))
    return out


def filter_variance_params(width, height, sigma_value=None, value_eps=None, **base):
    """rt_filter_variance_params of a width x height plane: rt_filter_variance_params_default's values (rt_filter_params'
    defaults, sigma_value 4, value_eps 0) unless given.  base: passes, normal_min_dot, plane_eps, value_max_diff."""
    p = abi.RtFilterVarianceParams()
    lib().rt_filter_variance_params_default(C.byref(p), int(width), int(height))
    for key, v in base.items():
        if key not in ("passes", "normal_min_dot", "plane_eps", "value_max_diff"):
            raise TypeError("filter_variance_params: unknown parameter %r" % key)
        if v is not None:
            setattr(p.base, key, v)
    for key, v in (("sigma_value", sigma_value), ("value_eps", value_eps)):
        if v is not None:
            setattr(p, key, v)
    return p


def _filter_variance_host_planes(value, variance, position4, normal4, out, out_variance, want_variance):
    """The numpy planes of a blocking variance-guided filter call: _filter_host_planes' for the value, and the same rules for
    variance / out_variance (None: a fresh plane when wanted, else not computed; `variance` itself: in place)."""
    h, w, v, pos, nrm, out = _filter_host_planes(value, position4, normal4, out)
    if not isinstance(variance, np.ndarray) or variance.shape != (h, w):
        raise ValueError("variance must be a numpy array of shape [%d, %d]" % (h, w))
    var = np.ascontiguousarray(variance, np.float32)
    if out_variance is variance:
        if not (variance.dtype == np.float32 and variance.flags.c_contiguous and variance.flags.writeable):
            raise ValueError("in place, variance must be a writeable C-contiguous float32 array")
        out_variance = var
    elif out_variance is None:
        out_variance = np.empty((h, w), np.float32) if want_variance else None
    elif (not isinstance(out_variance, np.ndarray) or out_variance.dtype != np.float32 or out_variance.shape != (h, w)
          or not out_variance.flags.c_contiguous):
        raise ValueError("out_variance must be a C-contiguous float32 array of shape (%d, %d)" % (h, w))
    return h, w, v, var, pos, nrm, out, out_variance


def filter_plane_variance_host(value, variance, position4, normal4, out=None, out_variance=None, want_variance=True, **params):
    """The variance-guided a-trous filter on the host (rt_filter_plane_variance_host; needs no device): value, variance
    float32 [h, w], position4 / normal4 float32 [h, w, 4] -> (value, variance) float32 [h, w], the variance None with
    want_variance=False and no out_variance.  params: filter_variance_params'.  out=value / out_variance=variance filter in
    place."""
    h, w, v, var, pos, nrm, out, ovar = _filter_variance_host_planes(value, variance, position4, normal4, out, out_variance,
                                                                      want_variance)
    p = filter_variance_params(w, h, **params)
    _check(lib().rt_filter_plane_variance_host(C.byref(p), _fp(v), _fp(var), _fp(pos), _fp(nrm), _fp(out), _fp_or_none(ovar)))
    return out, ovar


def accumulate_params(width, height, prev_rot=None, prev_cam=None, prev_focal=None, aa_x=1, **overrides):
    """rt_accumulate_params of a width x height plane: rt_accumulate_params_default's values (identity view, focal = width,
    0.9, 0.01, 32 frames) unless given.  prev_rot / prev_cam / prev_focal are the previous view as rt_render takes it, so
    prev_focal is in AA sub-pixels along x and is divided by aa_x here.  overrides: normal_min_dot, plane_eps, max_history,
    prev_focal_px."""
    p = abi.RtAccumulateParams()
    lib().rt_accumulate_params_default(C.byref(p), int(width), int(height))
    if prev_rot is not None:
        p.prev_rot[:] = [float(v) for v in np.asarray(prev_rot, np.float32).reshape(-1)[:12]]
    if prev_cam is not None:
        p.prev_cam[:] = [float(v) for v in np.asarray(prev_cam, np.float32).reshape(-1)[:3]]
    if prev_focal is not None:
        p.prev_focal_px = np.float32(prev_focal) / np.float32(aa_x)
    for key, v in overrides.items():
        if key not in ("normal_min_dot", "plane_eps", "max_history", "prev_focal_px"):
            raise TypeError("accumulate_params: unknown parameter %r" % key)
        if v is not None:
            setattr(p, key, v)
    return p


def _accumulate_host_planes(value, position4, normal4, prim, prev):
    """The numpy planes of a blocking accumulate call: _host_planes' inputs, prim int32 [h, w] or None, prev float32
    [h, w, 12] (abi.HISTORY_WORDS) or None; and fresh next / out_mean / out_variance."""
    h, w, v, pos, nrm = _host_planes(value, position4, normal4)
    if prim is not None:
        prim = np.ascontiguousarray(prim, np.int32)
        if prim.shape != (h, w):
            raise ValueError("prim must have the shape [%d, %d]" % (h, w))
    if prev is not None:
        if not isinstance(prev, np.ndarray) or prev.dtype != np.float32 or prev.shape != (h, w, abi.HISTORY_WORDS):
            raise ValueError("prev must be a float32 array of shape [%d, %d, %d]" % (h, w, abi.HISTORY_WORDS))
        prev = np.ascontiguousarray(prev)
    nxt = np.empty((h, w, abi.HISTORY_WORDS), np.float32)
    return h, w, v, pos, nrm, prim, prev, nxt, np.empty((h, w), np.float32), np.empty((h, w), np.float32)


def _reproj_host_planes(reproj_position4, reproj_normal4, h, w):
    """The optional reprojection planes of a blocking accumulate call as C-contiguous float32 [h, w, 4] arrays (None stays None;
    one without the other is the library's to refuse)."""
    out = []
    for name, a in (("reproj_position4", reproj_position4), ("reproj_normal4", reproj_normal4)):
        if a is not None:
            a = np.ascontiguousarray(a, np.float32)
            if a.shape != (h, w, 4):
                raise ValueError("%s must have the shape [%d, %d, 4]" % (name, h, w))
        out.append(a)
    return out


def _fp_or_none(a):
    return _fp(a) if a is not None else None


def accumulate_plane_host(value, position4, normal4, prim=None, prev=None, params=None, reproj_position4=None, reproj_normal4=None,
                          **kw):
    """The temporal reprojection on the host (rt_accumulate_plane_host; needs no device): value float32 [h, w], position4 /
    normal4 float32 [h, w, 4], prim int32 [h, w] or None, prev = the `next` of the previous call or None -> (next float32
    [h, w, 12], mean [h, w], variance [h, w]).  params: an abi.RtAccumulateParams, or kw for accumulate_params (prev_rot,
    prev_cam, prev_focal, aa_x, normal_min_dot, plane_eps, max_history).  reproj_position4 / reproj_normal4 float32 [h, w, 4]
    (motion_planes' outputs): rt_accumulate_plane_moving_host."""
    h, w, v, pos, nrm, prim, prev, nxt, mean, var = _accumulate_host_planes(value, position4, normal4, prim, prev)
    rpos, rnrm = _reproj_host_planes(reproj_position4, reproj_normal4, h, w)
    p = params if params is not None else accumulate_params(w, h, **kw)
    if rpos is None and rnrm is None:
        _check(lib().rt_accumulate_plane_host(C.byref(p), _fp(v), _fp(pos), _fp(nrm), _ip(prim), _fp_or_none(prev), _fp(nxt), _fp(mean),
                                              _fp(var)))
    else:
        _check(lib().rt_accumulate_plane_moving_host(C.byref(p), _fp(v), _fp(pos), _fp(nrm), _ip(prim), _fp_or_none(rpos),
                                                     _fp_or_none(rnrm), _fp_or_none(prev), _fp(nxt), _fp(mean), _fp(var)))
    return nxt, mean, var


def _motion_host_planes(prim, position4, normal4):
    """The element planes of a blocking motion call: prim int32 [...], position4 / normal4 float32 [..., 4] of the same
    leading shape -> (count, the three C-contiguous, and fresh outputs shaped like the float4 inputs)."""
    prim = np.ascontiguousarray(prim, np.int32)
    pos = np.ascontiguousarray(position4, np.float32)
    nrm = np.ascontiguousarray(normal4, np.float32)
    if pos.shape != prim.shape + (4,) or nrm.shape != pos.shape:
        raise ValueError("position4 and normal4 must have the shape of prim with a last axis of 4")
    return prim.size, prim, pos, nrm, np.empty_like(pos), np.empty_like(pos)


def motion_planes_host(vertices_now, vertices_then, normals_then, prim, position4, normal4):
    """Where each element's surface point was in a previous scene, on the host (rt_motion_planes_host; needs no device):
    vertices_now, vertices_then float32 [3n, 4], normals_then [n, 4] (the layouts of Scene.packed / scene_data), prim int32
    [...], position4 / normal4 float32 [..., 4] -> (prev_position4, prev_normal4) shaped like position4."""
    vn = np.ascontiguousarray(vertices_now, np.float32)
    vt = np.ascontiguousarray(vertices_then, np.float32)
    nt = np.ascontiguousarray(normals_then, np.float32)
    n = nt.shape[0]
    if vn.shape != (3 * n, 4) or vt.shape != (3 * n, 4) or nt.shape != (n, 4):
        raise ValueError("vertices_now and vertices_then must be [3n, 4] and normals_then [n, 4]")
    count, prim, pos, nrm, opos, onrm = _motion_host_planes(prim, position4, normal4)
    _check(lib().rt_motion_planes_host(_fp(vn), _fp(vt), _fp(nt), n, _ip(prim), _fp(pos), _fp(nrm), count, _fp(opos), _fp(onrm)))
    return opos, onrm


def default_config():
    cfg = abi.RtConfig()
    lib().rt_config_default(C.byref(cfg))
    return cfg


def rotation_matrix(yaw, pitch):
    rot = np.zeros(12, np.float32)
    lib().rt_rotation_matrix(C.c_float(yaw), C.c_float(pitch), _fp(rot))
    return rot


def _object_ranges(ranges, n):
    """The objects of set_objects / Scene.posed as a list of (first, count): each entry a (first, count) pair or a slice of
    step 1 over n triangles."""
    out = []
    for r in ranges:
        if isinstance(r, slice):
            first, stop, step = r.indices(n)
            if step != 1:
                raise ValueError("an object is a contiguous range of triangles (slice step 1)")
            out.append((first, stop - first))
        else:
            first, count = r
            out.append((int(first), int(count)))
    return out


def _skin_table(count, bone_index, weights):
    """The influence table of set_skin / Scene.skinned as (uint16 [3*count,4], float32 [3*count,4]), C-contiguous."""
    idx = np.asarray(bone_index)
    if idx.shape != (3 * count, 4) or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("bone_index must be an integer array of shape [%d, 4]" % (3 * count))
    if idx.size and (idx.min() < 0 or idx.max() > 0xFFFF):
        raise ValueError("bone indices must be in 0 .. 65535")
    w = np.ascontiguousarray(weights, np.float32)
    if w.shape != (3 * count, 4):
        raise ValueError("weights must have shape [%d, 4]" % (3 * count))
    return np.ascontiguousarray(idx, np.uint16), w


class Scene:
    """Triangle list in the reference's AoS format (TestModelH.h:11-38): array [n,5,4] = v0,v1,v2,normal,color."""

    def __init__(self, aos):
        self.aos = np.ascontiguousarray(aos, np.float32).reshape(-1, 5, 4)

    def __len__(self):
        return self.aos.shape[0]

    @classmethod
    def cornell_box(cls):
        """LoadTestModel (TestModelH.h:44)."""
        buf = (abi.RtTriangle * 64)()
        n = _check(lib().rt_scene_cornell_box(buf, 64))
        return cls(np.frombuffer(buf, np.float32, n * 20).copy())

    @classmethod
    def load_obj(cls, path, color=None, scale=1.5, translate=None):
        """load_obj (Loader.cpp:11); colour / scale / translation default to the reference's constants (:20,:42,:48)."""
        col = None if color is None else _fp(np.ascontiguousarray(color, np.float32))
        mv = None if translate is None else _fp(np.ascontiguousarray(translate, np.float32))
        n = _check(lib().rt_scene_load_obj_ex(os.fsencode(path), col, C.c_float(scale), mv, None, 0))
        buf = (abi.RtTriangle * max(n, 1))()
        _check(lib().rt_scene_load_obj_ex(os.fsencode(path), col, C.c_float(scale), mv, buf, n))
        return cls(np.frombuffer(buf, np.float32, n * 20).copy())

    def __add__(self, other):
        """triangles.insert(end, ...) as at skeleton.cpp:103."""
        return Scene(np.concatenate([self.aos, other.aos], axis=0))

    def with_color(self, indices, rgba):
        aos = self.aos.copy()
        aos[list(indices), 4, :] = np.asarray(rgba, np.float32)
        return Scene(aos)

    def transformed(self, indices, matrix, offset=(0.0, 0.0, 0.0)):
        """A new Scene whose triangles `indices` have every vertex v replaced by matrix @ v + offset (float32, the products
        summed left to right) and their normals recomputed by rt_triangle_compute_normal (ComputeNormal, TestModelH.h:26)."""
        xf = np.zeros((3, 4), np.float32)
        xf[:, :3] = np.asarray(matrix, np.float32).reshape(3, 3)
        xf[:, 3] = np.asarray(offset, np.float32).reshape(3)
        aos = self.aos.copy()
        idx = np.arange(len(self))[indices] if not isinstance(indices, (list, tuple)) else np.asarray(indices, np.int64)
        sel = np.ascontiguousarray(aos[idx])                 # the chosen triangles as one range: one call
        lib().rt_scene_transform(sel.ctypes.data_as(C.POINTER(abi.RtTriangle)), len(sel), 0, len(sel), _fp(xf))
        aos[idx] = sel
        return Scene(aos)

    def posed(self, ranges, xforms):
        """The scene P(self, xforms) of include/uob_rt.h "rigid objects": object k = the triangles ranges[k] ((first, count)
        or a slice) transformed by xforms[k] ([3,4]: matrix | translation) with rt_scene_transform, the host restatement of
        RayTracer.pose_objects."""
        ranges = _object_ranges(ranges, len(self))
        xf = np.ascontiguousarray(xforms, np.float32).reshape(len(ranges), 3, 4)
        aos = self.aos.copy()
        tris = aos.ctypes.data_as(C.POINTER(abi.RtTriangle))
        for (first, count), x in zip(ranges, xf):
            lib().rt_scene_transform(tris, len(self), first, count, _fp(np.ascontiguousarray(x)))
        return Scene(aos)

    def skinned(self, first, count, bone_index, weights, bones):
        """The scene S(self, bones) of include/uob_rt.h "skinned meshes": the triangles [first, first + count) blended from
        bones ([nbones,3,4]: matrix | translation) by the influence table (bone_index, weights: [3*count,4], one row per
        corner) with rt_scene_skin, the host restatement of RayTracer.pose_skin."""
        first, count = int(first), int(count)
        idx, w = _skin_table(count, bone_index, weights)
        b = np.ascontiguousarray(bones, np.float32)
        if b.ndim != 3 or b.shape[1:] != (3, 4):
            raise ValueError("bones must have shape [nbones, 3, 4]")
        aos = self.aos.copy()
        lib().rt_scene_skin(aos.ctypes.data_as(C.POINTER(abi.RtTriangle)), len(self), first, count,
                            idx.ctypes.data_as(C.POINTER(C.c_uint16)), _fp(w), _fp(b), b.shape[0])
        return Scene(aos)

    def packed(self):
        """The three float4 arrays uploaded at skeleton.cpp:474-496."""
        n = len(self)
        v = np.zeros((3 * max(n, 1), 4), np.float32)
        nr = np.zeros((max(n, 1), 4), np.float32)
        c = np.zeros((max(n, 1), 4), np.float32)
        tris = self.aos.ctypes.data_as(C.POINTER(abi.RtTriangle))
        lib().rt_scene_pack(tris, n, _fp(v), _fp(nr), _fp(c))
        return v[:3 * n], nr[:n], c[:n]


class RayTracer:
    """One rt_ctx: the scene uploaded once (opencl_initialise), frames rendered on demand (offload_rendering)."""

    def __init__(self, cfg, scene):
        self.cfg = cfg
        self.scene = scene
        v, nr, c = scene.packed()
        self._keep = (v, nr, c)
        h = C.c_void_p()
        _check(lib().rt_init(C.byref(cfg), _fp(v), _fp(nr), _fp(c), len(scene), C.byref(h)))
        self._h = h
        self.width = cfg.width
        self.n_triangles = len(scene)
        self.rows = lib().rt_config_owned_rows(C.byref(cfg))
        self.objects = None         # the (first, count) ranges of set_objects; a scene update or replace forgets them
        self.skin = None            # (first, count, nbones) of set_skin; forgotten likewise, and by set_objects
        # the device the context's queries run on (devices[0]; None: the device that was current at rt_init)
        self.device = cfg.devices[0] if cfg.num_devices >= 1 else (cfg.device if cfg.device >= 0 else None)
        self._history = None        # render_accumulated_light: [the two history tensors, which is current, the view, frames]
        self._moving = False        # a moving=True call of render_accumulated_light left a snapshot

    @staticmethod
    def _update_flags(reorder, device_tiles):
        return (abi.RT_UPDATE_REORDER if reorder else 0) | (abi.RT_UPDATE_DEVICE_TILES if device_tiles else 0)

    def update_scene(self, scene, reorder=False, device_tiles=False):
        """Replace the context's triangles (same count) between frames (rt_update_scene): refit the mesh kernel's tiles on
        the device, or sort them again on the host with reorder=True, or on the device with device_tiles=True."""
        v, nr, c = scene.packed()
        _check(lib().rt_update_scene(self._h, _fp(v), _fp(nr), _fp(c), len(scene), self._update_flags(reorder, device_tiles)))
        self.scene = scene
        self._keep = (v, nr, c)
        self.objects = self.skin = None

    def update_scene_device(self, v_ptr, n_ptr, c_ptr, n, stream=None, reorder=False, device_tiles=False):
        """The same from device memory (raw pointers, e.g. torch .data_ptr() of float32 [3n,4] / [n,4] / [n,4]), enqueued
        on `stream` (rt_update_scene_device).  The source buffers must stay unchanged until the stream has passed it."""
        _check(lib().rt_update_scene_device(self._h, C.c_void_p(v_ptr), C.c_void_p(n_ptr), C.c_void_p(c_ptr), n,
                                            self._update_flags(reorder, device_tiles), C.c_void_p(stream or 0)))
        self.objects = self.skin = None

    def replace_scene(self, scene, device_tiles=False):
        """Replace the context's triangles by a scene of any count (rt_replace_scene), blocking.  scene: a Scene, or the three
        packed arrays (vertices [3n,4], normals [n,4], colours [n,4]) of Scene.packed().  The tiles of a mesh are made on the
        host as rt_init makes them, or on the device (Morton order) with device_tiles=True."""
        if isinstance(scene, Scene):
            v, nr, c = scene.packed()
        else:
            v, nr, c = (np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in scene)
            if v.shape[0] != 3 * nr.shape[0] or c.shape[0] != nr.shape[0]:
                raise ValueError("packed arrays must have shapes [3n,4], [n,4], [n,4]")
            scene = None
        n = nr.shape[0]
        _check(lib().rt_replace_scene(self._h, _fp(v), _fp(nr), _fp(c), n, self._update_flags(False, device_tiles)))
        self.scene = scene
        self._keep = (v, nr, c)
        self.n_triangles = n
        self.objects = self.skin = None

    def replace_scene_device(self, vertices, normals, colors, stream=None, reorder=False):
        """The same from torch tensors on the context's device (float32 [3n,4] / [n,4] / [n,4]), enqueued on `stream` (a torch
        stream or a raw hipStream_t; default: torch's current stream) (rt_replace_scene_device): the tiles are made on the
        device; reorder=True asks for the host's tiles and stages the scene through the host.  The tensors must stay
        unchanged until the stream has passed the call."""
        dev = self._torch_device()
        if not isinstance(normals, _torch.Tensor) or normals.dim() != 2:
            raise ValueError("normals must be a torch tensor of shape [n, 4]")
        n = normals.shape[0]
        _need("vertices", vertices, _torch.float32, (3 * n, 4), dev)
        _need("normals", normals, _torch.float32, (n, 4), dev)
        _need("colors", colors, _torch.float32, (n, 4), dev)
        raw = self._raw_stream(stream, dev)
        _check(lib().rt_replace_scene_device(self._h, C.c_void_p(vertices.data_ptr()), C.c_void_p(normals.data_ptr()),
                                             C.c_void_p(colors.data_ptr()), n, self._update_flags(reorder, False),
                                             C.c_void_p(raw)))
        self.scene = None
        self.n_triangles = n
        self.objects = self.skin = None

    def set_objects(self, ranges):
        """Make the context's current scene the rest pose of rigid objects (rt_set_objects): ranges = a list of
        (first, count) pairs or slices of triangles, non-empty and disjoint; an empty list drops the table."""
        ranges = _object_ranges(ranges or (), self.n_triangles)
        first = np.asarray([r[0] for r in ranges], np.int32)
        count = np.asarray([r[1] for r in ranges], np.int32)
        _check(lib().rt_set_objects(self._h, _ip(first), _ip(count), len(ranges)))
        self.objects = ranges or None
        if ranges:
            self.skin = None

    def object_count(self):
        """Objects in the context's table (rt_debug_object_count)."""
        out = C.c_int32()
        _check(lib().rt_debug_object_count(self._h, C.byref(out)))
        return int(out.value)

    def pose_objects(self, xforms, reorder=False, device_tiles=False):
        """Pose the objects from the rest pose (rt_pose_objects), blocking: xforms = array [nobj, 3, 4], per object the matrix
        and, in the last column, the translation.  The tiles are refitted, or made again with reorder / device_tiles as in
        update_scene.  The context then holds Scene.posed(ranges, xforms) of the rest scene."""
        xf = np.ascontiguousarray(xforms, np.float32)
        if xf.shape != (len(self.objects or ()), 3, 4):
            raise ValueError("xforms must have shape [%d, 3, 4]" % len(self.objects or ()))
        _check(lib().rt_pose_objects(self._h, _fp(xf), self._update_flags(reorder, device_tiles)))
        self.scene = None

    def pose_objects_device(self, xforms, stream=None, device_tiles=False, reorder=False):
        """The same with the matrices in a torch tensor float32 [nobj, 3, 4] on the context's device, enqueued on `stream` (a
        torch stream or a raw hipStream_t; default: torch's current stream) (rt_pose_objects_device).  The tensor must stay
        unchanged until the stream has passed the call."""
        dev = self._torch_device()
        _need("xforms", xforms, _torch.float32, (len(self.objects or ()), 3, 4), dev)
        raw = self._raw_stream(stream, dev)
        _check(lib().rt_pose_objects_device(self._h, C.c_void_p(xforms.data_ptr()), self._update_flags(reorder, device_tiles),
                                            C.c_void_p(raw)))
        self.scene = None

    def set_skin(self, first, count, bone_index, weights, nbones):
        """Make the context's current scene the rest pose of a skin (rt_set_skin): the triangles [first, first + count) with
        four influences per corner, bone_index (integers < nbones) and weights (in [0, 1]) of shape [3*count, 4], one row per
        corner in the order corner 0, 1, 2 of triangle first, then of first + 1, ...  Drops the objects; count = 0 drops
        the skin."""
        first, count, nbones = int(first), int(count), int(nbones)
        if count > 0:
            idx, w = _skin_table(count, bone_index, weights)
        else:                           # (count = 0 drops the skin; a negative count is the library's to reject)
            idx, w = np.zeros((1, 4), np.uint16), np.zeros((1, 4), np.float32)
        _check(lib().rt_set_skin(self._h, first, count, idx.ctypes.data_as(C.POINTER(C.c_uint16)), _fp(w), nbones))
        if count == 0:
            self.skin = None
        else:
            self.objects, self.skin = None, (first, count, nbones)

    def skin_info(self):
        """(first, count, nbones) of the context's skin, zeros without one (rt_debug_skin_info)."""
        out = [C.c_int32() for _ in range(3)]
        _check(lib().rt_debug_skin_info(self._h, *[C.byref(x) for x in out]))
        return tuple(int(x.value) for x in out)

    def pose_skin(self, bones, reorder=False, device_tiles=False):
        """Pose the skin from the rest pose (rt_pose_skin), blocking: bones = array [nbones, 3, 4], per bone the matrix and, in
        the last column, the translation.  The tiles are refitted, or made again with reorder / device_tiles as in
        update_scene.  The context then holds Scene.skinned(first, count, bone_index, weights, bones) of the rest scene."""
        b = np.ascontiguousarray(bones, np.float32)
        if self.skin and b.shape != (self.skin[2], 3, 4):       # (without a skin the library says so)
            raise ValueError("bones must have shape [%d, 3, 4]" % self.skin[2])
        _check(lib().rt_pose_skin(self._h, _fp(b), self._update_flags(reorder, device_tiles)))
        self.scene = None

    def pose_skin_device(self, bones, stream=None, device_tiles=False, reorder=False):
        """The same with the bones in a torch tensor float32 [nbones, 3, 4] on the context's device, enqueued on `stream` (a
        torch stream or a raw hipStream_t; default: torch's current stream) (rt_pose_skin_device).  The tensor must stay
        unchanged until the stream has passed the call."""
        dev = self._torch_device()
        if self.skin:
            _need("bones", bones, _torch.float32, (self.skin[2], 3, 4), dev)
        raw = self._raw_stream(stream, dev)
        _check(lib().rt_pose_skin_device(self._h, C.c_void_p(bones.data_ptr()), self._update_flags(reorder, device_tiles),
                                         C.c_void_p(raw)))
        self.scene = None

    def update_spheres(self, spheres):
        """Replace the sphere table (rt_update_spheres): a list of up to RT_MAX_SPHERES (centre, radius_sq, colour rgba)
        tuples, as abi.make_config takes them.  self.cfg follows."""
        spheres = tuple(spheres or ())
        if len(spheres) > abi.RT_MAX_SPHERES:
            raise ValueError("at most %d spheres" % abi.RT_MAX_SPHERES)
        tab = (abi.RtSphere * abi.RT_MAX_SPHERES)()
        for i, (ctr, r2, col) in enumerate(spheres):
            tab[i].center[:] = ctr
            tab[i].radius_sq = r2
            tab[i].color[:] = col
        _check(lib().rt_update_spheres(self._h, tab, len(spheres)))
        self.cfg.num_spheres = len(spheres)
        for i in range(abi.RT_MAX_SPHERES):
            self.cfg.spheres[i] = tab[i]

    def scene_capacity(self):
        """Triangles the context's buffers can hold without allocating (rt_debug_scene_capacity)."""
        out = C.c_int64()
        _check(lib().rt_debug_scene_capacity(self._h, C.byref(out)))
        return int(out.value)

    def tile_data(self):
        """Mesh kernel: (orig int32 [n], tiles float32 [ntiles, 12]) — the tiled order and per-tile data (rt_debug_tile_data)."""
        nt = _check(lib().rt_debug_tile_data(self._h, None, None, 0))
        orig = np.zeros(self.n_triangles, np.int32)
        tiles = np.zeros((nt, 12), np.float32)
        _check(lib().rt_debug_tile_data(self._h, _ip(orig), _fp(tiles), nt))
        return orig, tiles

    def scene_data(self, tiled=False):
        """The scene the context holds, read back from the device (rt_debug_scene_data): dict with "vertices" [3n,4],
        "normals" [n,4], "colors" [n,4] in original order, "n_shadow" and the vertices' box "vbox_lo" / "vbox_hi" as the
        scene's check left them; with tiled=True also the mesh kernel's tiled copy "vertices_m", "normals_m", "colors_m"."""
        n = _check(lib().rt_debug_scene_data(self._h, None, None, None, None, None, None, None, None, None, 0))
        out = {"vertices": np.zeros((3 * n, 4), np.float32), "normals": np.zeros((n, 4), np.float32),
               "colors": np.zeros((n, 4), np.float32)}
        if tiled:
            out.update(vertices_m=np.zeros((3 * n, 4), np.float32), normals_m=np.zeros((n, 4), np.float32),
                       colors_m=np.zeros((n, 4), np.float32))
        n_shadow, lo, hi = C.c_int32(), np.zeros(3, np.float32), np.zeros(3, np.float32)
        tiled_ptrs = [_fp(out[k]) if tiled else None for k in ("vertices_m", "normals_m", "colors_m")]
        _check(lib().rt_debug_scene_data(self._h, _fp(out["vertices"]), _fp(out["normals"]), _fp(out["colors"]), *tiled_ptrs,
                                         C.byref(n_shadow), _fp(lo), _fp(hi), n))
        out.update(n_shadow=int(n_shadow.value), vbox_lo=lo, vbox_hi=hi)
        return out

    def close(self):
        if getattr(self, "_h", None):
            lib().rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _torch_device(self):
        """The torch device the context's device entries run on (devices[0]; without one, torch's current device)."""
        return _torch.device("cuda", self.device if self.device is not None else _torch.cuda.current_device())

    @staticmethod
    def _raw_stream(stream, dev):
        """A torch stream or a raw hipStream_t (None: torch's current stream on dev) as the integer the C ABI takes."""
        if stream is None:
            stream = _torch.cuda.current_stream(dev)
        return getattr(stream, "cuda_stream", stream) or 0

    def _stats(self, export, keys):
        """The eight counters a rt_debug_*_stats export reports for the context's most recent call of its family."""
        out = (C.c_uint64 * 8)()
        _check(getattr(lib(), export)(self._h, out))
        return {key: int(out[i]) for i, key in enumerate(keys)}

    @staticmethod
    def _args(rot, cam, light):
        return (np.ascontiguousarray(rot, np.float32), np.ascontiguousarray(cam, np.float32)[:3].copy(),
                np.ascontiguousarray(light, np.float32)[:3].copy())

    def render(self, rot, cam, light, focal, want_rgb=False, out=None):
        """Blocking render + readback.  Returns ARGB [rows,W] (and the float4 tap [rows,W,4]).
        `out`: optional C-contiguous uint32 [rows,W] array to receive the frame (screen->buffer)."""
        rot, cam, light = self._args(rot, cam, light)
        if out is not None and (out.dtype != np.uint32 or out.shape != (self.rows, self.width) or not out.flags.c_contiguous):
            raise ValueError("out must be a C-contiguous uint32 array of shape (%d, %d)" % (self.rows, self.width))
        argb = out if out is not None else np.zeros((self.rows, self.width), np.uint32)
        rgb = np.zeros((self.rows, self.width, 4), np.float32) if want_rgb else None
        _check(lib().rt_render(self._h, _fp(rot), _fp(cam), _fp(light), C.c_float(focal),
                               argb.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(rgb) if want_rgb else None))
        return (argb, rgb) if want_rgb else argb

    def register_output(self, arr):
        """Pin and map a host array (the caller's framebuffer): later render(out=arr) calls have the kernel write the pixels
        straight into it over PCIe (rt_register_output).  Keep `arr` alive until unregister_output() / close()."""
        _check(lib().rt_register_output(self._h, C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes)))
        self._registered = arr

    def unregister_output(self):
        _check(lib().rt_unregister_output(self._h))
        self._registered = None

    def render_device(self, rot, cam, light, focal, d_argb_ptr, d_rgb_ptr=None, stream=None):
        """Enqueue a frame into caller-owned device memory (raw pointers, e.g. torch .data_ptr())."""
        rot, cam, light = self._args(rot, cam, light)
        _check(lib().rt_render_device(self._h, _fp(rot), _fp(cam), _fp(light), C.c_float(focal),
                                      C.c_void_p(d_argb_ptr), C.c_void_p(d_rgb_ptr or 0), C.c_void_p(stream or 0)))

    def count_work(self, rot, cam, light, focal):
        rot, cam, light = self._args(rot, cam, light)
        w = abi.RtWork()
        _check(lib().rt_count_work(self._h, _fp(rot), _fp(cam), _fp(light), C.c_float(focal), C.byref(w)))
        return w.as_dict()

    def count_executed(self, rot, cam, light, focal):
        """Executed work of the wave kernel (include/uob_rt.h rt_count_executed)."""
        rot, cam, light = self._args(rot, cam, light)
        out = (C.c_uint64 * 8)()
        _check(lib().rt_count_executed(self._h, _fp(rot), _fp(cam), _fp(light), C.c_float(focal), out))
        if self.n_triangles > 64:      # tiled mesh kernel
            keys = ("primary_tile_visits", "primary_bound_survivors", "shadow_tile_visits", "level1_survivors",
                    "level3_pair_calls", "level3_stage1_iterations", "longest_block_ticks", "wave_task_rounds")
        else:
            keys = ("surface_points", "stage1_wave_iterations", "stage2_wave_iterations", "sphere_wave_evaluations",
                    "culled_pairs", "tasks_resolved_whole", "sampled_points_fully_lit", "sampled_points_fully_blocked")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def trace_in_shadow(self, rays, radius_sq):
        """Device in_shadow (kernels.cl:243) on caller rays [k,6] = start, direction -> uint8 [k]."""
        rays = _rays6(rays)
        r2 = np.ascontiguousarray(radius_sq, np.float32)
        out = np.zeros(rays.shape[0], np.int32)
        _check(lib().rt_debug_trace_rays(self._h, abi.RT_TRACE_IN_SHADOW, _fp(rays), _fp(r2), rays.shape[0], _ip(out), None))
        return out.astype(np.uint8)

    def trace_closest_hit(self, rays):
        """Device single_ray_intersections (kernels.cl:168) on caller rays -> (tri [k], out [k,10])."""
        rays = _rays6(rays)
        tri = np.zeros(rays.shape[0], np.int32)
        out = np.zeros((rays.shape[0], 10), np.float32)
        _check(lib().rt_debug_trace_rays(self._h, abi.RT_TRACE_CLOSEST_HIT, _fp(rays), None, rays.shape[0], _ip(tri), _fp(out)))
        return tri, out

    def query_in_shadow(self, rays, radius_sq):
        """Tile-culled in_shadow (rt_trace_rays) on caller rays [k,6] = start, direction -> uint8 [k]; the same bits as
        trace_in_shadow."""
        rays = _rays6(rays)
        r2 = np.ascontiguousarray(radius_sq, np.float32).reshape(-1)
        if r2.shape[0] != rays.shape[0]:
            raise ValueError("radius_sq must have one entry per ray")
        out = np.zeros(rays.shape[0], np.int32)
        _check(lib().rt_trace_rays(self._h, abi.RT_TRACE_IN_SHADOW, _fp(rays), _fp(r2), rays.shape[0], _ip(out), None))
        return out.astype(np.uint8)

    def query_closest_hit(self, rays):
        """Tile-culled closest hit (rt_trace_rays) on caller rays -> (tri [k], out [k,10]); the same bits as
        trace_closest_hit."""
        rays = _rays6(rays)
        tri = np.zeros(rays.shape[0], np.int32)
        out = np.zeros((rays.shape[0], 10), np.float32)
        _check(lib().rt_trace_rays(self._h, abi.RT_TRACE_CLOSEST_HIT, _fp(rays), None, rays.shape[0], _ip(tri), _fp(out)))
        return tri, out

    def query_device(self, what, rays, radius_sq=None, out_tri=None, out10=None, stream=None):
        """Enqueue a ray query on torch tensors of the context's device (rt_trace_rays_device), without synchronising.
        rays: float32 [k,6]; radius_sq: float32 [k] (RT_TRACE_IN_SHADOW); out_tri: int32 [k]; out10: float32 [k,10]
        (RT_TRACE_CLOSEST_HIT, optional).  Missing outputs are allocated.  stream: a torch stream or a raw hipStream_t
        (default: torch's current stream).  Returns (out_tri, out10) for closest hit, out_tri for in_shadow."""
        import torch
        if what not in (abi.RT_TRACE_IN_SHADOW, abi.RT_TRACE_CLOSEST_HIT):
            raise ValueError("unknown query mode %r" % (what,))
        dev = self._torch_device()
        k = _rows("rays", rays, 6, dev)
        shadow = what == abi.RT_TRACE_IN_SHADOW
        if shadow:
            if radius_sq is None:
                raise ValueError("in_shadow queries need radius_sq")
            _need("radius_sq", radius_sq, torch.float32, (k,), dev)
        out_tri = _out("out_tri", out_tri, torch.int32, (k,), dev)
        if not shadow:
            out10 = _out("out10", out10, torch.float32, (k, 10), dev)
        raw = self._raw_stream(stream, dev)
        if k:
            _check(lib().rt_trace_rays_device(self._h, what, C.c_void_p(rays.data_ptr()),
                                              C.c_void_p(radius_sq.data_ptr() if shadow else 0), k,
                                              C.c_void_p(out_tri.data_ptr()), C.c_void_p(0 if shadow else out10.data_ptr()),
                                              C.c_void_p(raw)))
        return out_tri if shadow else (out_tri, out10)

    def _aov_shape(self, name, sample):
        if name not in abi.AOV_PLANES:
            raise ValueError("unknown AOV plane %r (one of %s)" % (name, ", ".join(abi.AOV_PLANES)))
        ch = abi.AOV_PLANES[name][1]
        aa = self.cfg.aa_x * self.cfg.aa_y
        return (self.rows, self.width) + ((aa,) if sample is None else ()) + ((4,) if ch == 4 else ())

    def render_aov(self, rot, cam, focal, sample=0, planes=("prim", "depth", "position", "normal", "albedo", "direction")):
        """AOV pass of the view (rt_render_aov), blocking: dict plane name -> numpy array [rows, W] (prim int32, depth
        float32) / [rows, W, 4] (float32); sample=None = every AA sample, with an extra axis of aa_x*aa_y samples in front of
        the channel axis."""
        rot, cam, _ = self._args(rot, cam, cam)
        planes = tuple(planes)
        out, bufs = {}, abi.RtAovBuffers()
        for name in planes:
            shape = self._aov_shape(name, sample)
            out[name] = np.zeros(shape, np.int32 if abi.AOV_PLANES[name][2] else np.float32)
            setattr(bufs, abi.AOV_PLANES[name][0], out[name].ctypes.data)
        _check(lib().rt_render_aov(self._h, _fp(rot), _fp(cam), C.c_float(focal),
                                   abi.RT_AOV_ALL_SAMPLES if sample is None else int(sample), C.byref(bufs)))
        return out

    def render_aov_device(self, rot, cam, focal, sample=0, out=None, stream=None):
        """Enqueue an AOV pass into torch tensors of the context's device (rt_render_aov_device), without synchronising.
        out: dict plane name -> contiguous tensor shaped as render_aov's arrays (prim int32, the others float32); only the
        planes named in it are computed.  stream: a torch stream or a raw hipStream_t (default: torch's current stream)."""
        import torch
        if not out:
            raise ValueError("out must name at least one plane")
        dev = self._torch_device()
        rot, cam, _ = self._args(rot, cam, cam)
        bufs = abi.RtAovBuffers()
        for name, t in out.items():
            shape = self._aov_shape(name, sample)
            dtype = torch.int32 if abi.AOV_PLANES[name][2] else torch.float32
            if not isinstance(t, torch.Tensor):
                raise ValueError("plane %r must be a contiguous %s tensor of shape %s on %s" % (name, dtype, shape, dev))
            _need("plane %r" % name, t, dtype, shape, dev)
            setattr(bufs, abi.AOV_PLANES[name][0], t.data_ptr())
        raw = self._raw_stream(stream, dev)
        _check(lib().rt_render_aov_device(self._h, _fp(rot), _fp(cam), C.c_float(focal),
                                          abi.RT_AOV_ALL_SAMPLES if sample is None else int(sample), C.byref(bufs),
                                          C.c_void_p(raw)))
        return out

    def aov_stats(self):
        """Work counters of the context's most recent AOV pass (rt_debug_aov_stats): dict of AOV_STATS_KEYS."""
        return self._stats("rt_debug_aov_stats", AOV_STATS_KEYS)

    def shade_points(self, points, normals, light, seeds=None, want_counts=False):
        """Soft-shadowed direct light at caller points (rt_shade_points), blocking: points, normals [k,3] (intersect and
        intersect_normal, e.g. the AOV position / normal planes), seeds int32 [k] = the global_id of each point's jitter
        stream (None: k & 0xFFFFFF; the frame uses the pixel id) -> light float32 [k], one channel of the reference's
        direct_light; with want_counts also the unblocked samples int32 [k] (0 .. shadow_samples)."""
        p = np.asarray(points, np.float32).reshape(-1, 3)
        nr = np.asarray(normals, np.float32).reshape(-1, 3)
        if p.shape != nr.shape:
            raise ValueError("points and normals must have the same shape [k, 3]")
        k = p.shape[0]
        p6 = np.ascontiguousarray(np.concatenate([p, nr], 1), np.float32)
        li = _light3(light)
        sp = _seeds_ptr(seeds, k, "point")
        out = np.zeros(k, np.float32)
        cnt = np.zeros(k, np.int32) if want_counts else None
        _check(lib().rt_shade_points(self._h, _fp(p6), sp, k, _fp(li), _fp(out), _ip(cnt)))
        return (out, cnt) if want_counts else out

    def shade_points_device(self, points6, light, seeds=None, out_light=None, out_counts=None, want_counts=False, stream=None):
        """Enqueue rt_shade_points_device on torch tensors of the context's device, without synchronising.  points6: float32
        [k,6] (position, normal); seeds: int32 [k] or None; out_light: float32 [k]; out_counts: int32 [k] (allocated when
        want_counts).  stream: a torch stream or a raw hipStream_t (default: torch's current stream).  Returns out_light, or
        (out_light, out_counts) when counts are asked for."""
        import torch
        dev = self._torch_device()
        k = _rows("points6", points6, 6, dev)
        if seeds is not None:
            _need("seeds", seeds, torch.int32, (k,), dev)
        out_light = _out("out_light", out_light, torch.float32, (k,), dev)
        if out_counts is not None or want_counts:
            out_counts = _out("out_counts", out_counts, torch.int32, (k,), dev)
        li = _light3(light)
        raw = self._raw_stream(stream, dev)
        if k:
            _check(lib().rt_shade_points_device(self._h, C.c_void_p(points6.data_ptr()),
                                                C.c_void_p(seeds.data_ptr() if seeds is not None else 0), k, _fp(li),
                                                C.c_void_p(out_light.data_ptr()),
                                                C.c_void_p(out_counts.data_ptr() if out_counts is not None else 0),
                                                C.c_void_p(raw)))
        return out_light if out_counts is None else (out_light, out_counts)

    def _primary_hits(self, method, rot, cam, focal, sample, bands_ok):
        """What the render_*_light methods do up to their shade call.  Refuses, in `method`'s name, a `sample` that is not one
        AA sample index, a context of row bands unless bands_ok, and a frame of more than 2^24 pixels; then an AOV pass of
        that sample -> (planes: fresh prim / position / normal tensors, p6: the shade call's points float32 [rows * W, 6],
        hit: bool [rows, W], the pixels that see something)."""
        import torch
        cfg = self.cfg
        aa = cfg.aa_x * cfg.aa_y
        if sample is None or isinstance(sample, bool) or int(sample) != sample or not 0 <= int(sample) < aa:
            raise ValueError("sample must be one AA sample index in [0, %d)" % aa)
        if not bands_ok and max(cfg.band_count, 1) != 1:
            raise ValueError("%s: a context of row bands does not hold neighbouring rows" % method)
        if cfg.width * cfg.height > abi.RT_SHADE_SEED_MAX:
            raise ValueError("%s: %d x %d pixels exceed the seed domain of 2^24 ids" % (method, cfg.width, cfg.height))
        dev = self._torch_device()
        shape = (self.rows, self.width)
        planes = {"prim": torch.empty(shape, dtype=torch.int32, device=dev),
                  "position": torch.empty(shape + (4,), dtype=torch.float32, device=dev),
                  "normal": torch.empty(shape + (4,), dtype=torch.float32, device=dev)}
        self.render_aov_device(rot, cam, focal, sample=sample, out=planes)
        p6 = torch.cat([planes["position"][..., :3], planes["normal"][..., :3]], -1).reshape(-1, 6).contiguous()
        return planes, p6, planes["prim"] != -1

    def _pixel_ids(self):
        """The global id of every pixel the context owns, its rows top to bottom: int32 [rows * W], the frame's seeds."""
        import torch
        cfg, dev = self.cfg, self._torch_device()
        br, bc = (cfg.band_rows if cfg.band_rows > 0 else cfg.height), max(cfg.band_count, 1)
        ys = torch.tensor([y for y in range(cfg.height) if (y // br) % bc == cfg.band_index], dtype=torch.int32, device=dev)
        return (ys[:, None] * self.width + torch.arange(self.width, dtype=torch.int32, device=dev)[None, :]).reshape(-1).contiguous()

    def _visibility_and_term(self, pos, nrm, hit, counts, light):
        """From a shade call's counts: (zero, V = counts / shadow_samples, term = 16 * max(dot(dir, N), 0) / (4 pi r^2) with
        dir = light - P), float32 [rows, W] each, V and term 0 where the pixel sees nothing."""
        import math
        import torch
        zero = torch.zeros(hit.shape, dtype=torch.float32, device=hit.device)
        vis = torch.where(hit, counts.reshape(hit.shape).to(torch.float32) / float(self.cfg.shadow_samples), zero)
        d = torch.tensor(_light3(light), device=hit.device) - pos[..., :3]
        r2 = (d * d).sum(-1)
        term = 16.0 * (d * nrm[..., :3]).sum(-1).clamp_min(0.0) / (4.0 * math.pi * r2)
        return zero, vis, torch.where(hit, term, zero)

    def render_direct_light(self, rot, cam, light, focal, sample=0):
        """The direct light of every pixel's primary hit, on the device: an AOV pass (position, normal, prim of AA sample
        `sample`) and a shade call seeded with the global pixel id, as the frame seeds it -> torch float32 [rows, W], 0 where
        the pixel sees nothing.  For a diffuse hit, albedo.xyz * (0.5 + light) is that sample's colour in the frame.
        Runs on torch's current stream; does not synchronise.  sample is one AA sample index (not RT_AOV_ALL_SAMPLES: the
        result is one value per pixel); a context of row bands gets its owned rows, seeded with the global ids; frames of
        more than 2^24 pixels are refused (the ids leave the seed domain and the frame's own ids are formed in FP32)."""
        import torch
        planes, p6, hit = self._primary_hits("render_direct_light", rot, cam, focal, sample, bands_ok=True)
        out = self.shade_points_device(p6, light, seeds=self._pixel_ids())
        return torch.where(hit.reshape(-1), out, torch.zeros_like(out)).reshape(hit.shape)

    def filter_plane(self, value, position4, normal4, out=None, **params):
        """The a-trous filter of a per-pixel plane on the device (rt_filter_plane), blocking: numpy planes as
        runtime.filter_plane_host takes them, and the same bits.  out=value filters in place."""
        h, w, v, pos, nrm, out = _filter_host_planes(value, position4, normal4, out)
        p = filter_params(w, h, **params)
        _check(lib().rt_filter_plane(self._h, C.byref(p), _fp(v), _fp(pos), _fp(nrm), _fp(out)))
        return out

    def filter_plane_device(self, value, position4, normal4, out=None, stream=None, **params):
        """Enqueue rt_filter_plane_device on torch tensors of the context's device, without synchronising.  value: float32
        [h, w]; position4, normal4: float32 [h, w, 4] (the AOV planes); out: float32 [h, w], allocated when None, `value`
        itself for in-place use.  stream: a torch stream or a raw hipStream_t (default: torch's current stream)."""
        import torch
        dev = self._torch_device()
        h, w = _guide_tensors(value, position4, normal4, dev)
        out = _out("out", out, torch.float32, (h, w), dev)
        p = filter_params(w, h, **params)
        raw = self._raw_stream(stream, dev)
        _check(lib().rt_filter_plane_device(self._h, C.byref(p), C.c_void_p(value.data_ptr()), C.c_void_p(position4.data_ptr()),
                                            C.c_void_p(normal4.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(raw)))
        return out

    def filter_stats(self):
        """Work counters of the context's most recent filter call (rt_debug_filter_stats): dict of FILTER_STATS_KEYS."""
        return self._stats("rt_debug_filter_stats", FILTER_STATS_KEYS)

    def filter_plane_variance(self, value, variance, position4, normal4, out=None, out_variance=None, want_variance=True, **params):
        """The variance-guided a-trous filter on the device (rt_filter_plane_variance), blocking: numpy planes as
        runtime.filter_plane_variance_host takes them, and the same bits -> (value, variance)."""
        h, w, v, var, pos, nrm, out, ovar = _filter_variance_host_planes(value, variance, position4, normal4, out, out_variance,
                                                                          want_variance)
        p = filter_variance_params(w, h, **params)
        _check(lib().rt_filter_plane_variance(self._h, C.byref(p), _fp(v), _fp(var), _fp(pos), _fp(nrm), _fp(out), _fp_or_none(ovar)))
        return out, ovar

    def filter_plane_variance_device(self, value, variance, position4, normal4, out=None, out_variance=None, want_variance=True,
                                     stream=None, **params):
        """Enqueue rt_filter_plane_variance_device on torch tensors of the context's device, without synchronising.  value,
        variance: float32 [h, w]; position4, normal4: float32 [h, w, 4] (the AOV planes); out, out_variance: float32 [h, w],
        allocated when None (the variance only when wanted), `value` / `variance` themselves for in-place use.  stream: a
        torch stream or a raw hipStream_t (default: torch's current stream).  Returns (out, out_variance), None for a variance
        that was not asked for."""
        import torch
        dev = self._torch_device()
        h, w = _guide_tensors(value, position4, normal4, dev)
        _need("variance", variance, torch.float32, (h, w), dev)
        out = _out("out", out, torch.float32, (h, w), dev)
        if out_variance is not None or want_variance:
            out_variance = _out("out_variance", out_variance, torch.float32, (h, w), dev)
        p = filter_variance_params(w, h, **params)
        raw = self._raw_stream(stream, dev)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        _check(lib().rt_filter_plane_variance_device(self._h, C.byref(p), ptr(value), ptr(variance), ptr(position4), ptr(normal4),
                                                     ptr(out), ptr(out_variance), C.c_void_p(raw)))
        return out, out_variance

    def filter_variance_stats(self):
        """Work counters of the context's most recent filter call as a variance-guided call names them
        (rt_debug_filter_stats): dict of FILTER_VARIANCE_STATS_KEYS."""
        return self._stats("rt_debug_filter_stats", FILTER_VARIANCE_STATS_KEYS)

    def render_filtered_light(self, rot, cam, light, focal, sample=0, want_parts=False, **params):
        """The direct light of every pixel's primary hit with its shadow term reconstructed by the a-trous filter, on the
        device: an AOV pass (position, normal, prim of AA sample `sample`), a shade call with counts seeded like the frame,
        the visibility V = counts / shadow_samples filtered under the AOV planes as guides (params: filter_params), and
        term * V_f with term = 16 * max(dot(dir, N), 0) / (4 pi r^2), dir = light - P, formed in torch -> torch float32
        [rows, W], 0 where the pixel sees nothing.  Filtering V and not the light leaves fully lit and fully shadowed regions
        exactly as they were: only penumbrae are noisy.  Float-accurate, not bit-pinned to the frame (the frame sums term per
        sample).  want_parts: also (term, V, V_f).  Runs on torch's current stream; does not synchronise.  Refuses contexts of
        row bands (their rows are not neighbours) and, like render_direct_light, frames beyond 2^24 pixels."""
        import torch
        planes, p6, hit = self._primary_hits("render_filtered_light", rot, cam, focal, sample, bands_ok=False)
        pos, nrm = planes["position"], planes["normal"]
        _, counts = self.shade_points_device(p6, light, seeds=self._pixel_ids(), want_counts=True)
        zero, vis, term = self._visibility_and_term(pos, nrm, hit, counts, light)
        vis_f = self.filter_plane_device(vis, pos, nrm, **params)
        out = term * torch.where(hit, vis_f, zero)
        return (out, term, vis, vis_f) if want_parts else out

    def motion_snapshot(self, stream=None):
        """Keep the scene as it is now as "the previous view's" (rt_motion_snapshot): enqueued on stream (a torch stream or a
        raw hipStream_t; default: torch's current stream), without synchronising.  Take it after the frame or AOV pass of a view
        and before the pose or update that makes the next one."""
        _check(lib().rt_motion_snapshot(self._h, C.c_void_p(self._raw_stream(stream, self._torch_device()))))

    def motion_release(self):
        """Free the snapshot (rt_motion_release); motion calls are refused until the next motion_snapshot."""
        _check(lib().rt_motion_release(self._h))

    def motion_info(self):
        """Triangles of the context's snapshot, 0 without one (rt_debug_motion_info)."""
        out = C.c_int32()
        _check(lib().rt_debug_motion_info(self._h, C.byref(out)))
        return int(out.value)

    def motion_planes(self, prim, position4, normal4):
        """Where each element's surface point was in the snapshot's scene (rt_motion_planes), blocking: numpy planes as
        runtime.motion_planes_host takes them, and the same bits -> (prev_position4, prev_normal4)."""
        count, prim, pos, nrm, opos, onrm = _motion_host_planes(prim, position4, normal4)
        _check(lib().rt_motion_planes(self._h, _ip(prim), _fp(pos), _fp(nrm), count, _fp(opos), _fp(onrm)))
        return opos, onrm

    def motion_planes_device(self, prim, position4, normal4, out_position4=None, out_normal4=None, stream=None):
        """Enqueue rt_motion_planes_device on torch tensors of the context's device, without synchronising.  prim: int32 [...];
        position4, normal4: float32 [..., 4] of the same leading shape (the AOV planes); out_position4, out_normal4: like
        position4, allocated when None.  stream: a torch stream or a raw hipStream_t (default: torch's current stream)."""
        import torch
        dev = self._torch_device()
        if not isinstance(prim, torch.Tensor):
            raise TypeError("prim must be a torch tensor")
        shape = tuple(prim.shape)
        _need("prim", prim, torch.int32, shape, dev)
        _need("position4", position4, torch.float32, shape + (4,), dev)
        _need("normal4", normal4, torch.float32, shape + (4,), dev)
        out_position4 = _out("out_position4", out_position4, torch.float32, shape + (4,), dev)
        out_normal4 = _out("out_normal4", out_normal4, torch.float32, shape + (4,), dev)
        raw = self._raw_stream(stream, dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        _check(lib().rt_motion_planes_device(self._h, ptr(prim), ptr(position4), ptr(normal4), prim.numel(), ptr(out_position4),
                                             ptr(out_normal4), C.c_void_p(raw)))
        return out_position4, out_normal4

    def motion_stats(self):
        """Work counters of the context's most recent motion call (rt_debug_motion_stats): dict of MOTION_STATS_KEYS."""
        return self._stats("rt_debug_motion_stats", MOTION_STATS_KEYS)

    def accumulate_plane(self, value, position4, normal4, prim=None, prev=None, params=None, reproj_position4=None,
                         reproj_normal4=None, **kw):
        """The temporal reprojection of a per-pixel plane on the device (rt_accumulate_plane), blocking: numpy planes as
        runtime.accumulate_plane_host takes them, and the same bits -> (next, mean, variance).  With reproj_position4 /
        reproj_normal4 (motion_planes' outputs): rt_accumulate_plane_moving."""
        h, w, v, pos, nrm, prim, prev, nxt, mean, var = _accumulate_host_planes(value, position4, normal4, prim, prev)
        rpos, rnrm = _reproj_host_planes(reproj_position4, reproj_normal4, h, w)
        p = params if params is not None else accumulate_params(w, h, **kw)
        if rpos is None and rnrm is None:
            _check(lib().rt_accumulate_plane(self._h, C.byref(p), _fp(v), _fp(pos), _fp(nrm), _ip(prim), _fp_or_none(prev), _fp(nxt),
                                             _fp(mean), _fp(var)))
        else:
            _check(lib().rt_accumulate_plane_moving(self._h, C.byref(p), _fp(v), _fp(pos), _fp(nrm), _ip(prim), _fp_or_none(rpos),
                                                    _fp_or_none(rnrm), _fp_or_none(prev), _fp(nxt), _fp(mean), _fp(var)))
        return nxt, mean, var

    def accumulate_plane_device(self, value, position4, normal4, prim=None, prev=None, next=None, out_mean=None, out_variance=None,
                                want_mean=True, want_variance=True, stream=None, params=None, reproj_position4=None,
                                reproj_normal4=None, **kw):
        """Enqueue rt_accumulate_plane_device on torch tensors of the context's device, without synchronising.  value: float32
        [h, w]; position4, normal4: float32 [h, w, 4] (the AOV planes); prim: int32 [h, w] or None; prev: float32 [h, w, 12]
        (the `next` of the previous call) or None; next, out_mean, out_variance: allocated when None (the two planes only
        when wanted).  stream: a torch stream or a raw hipStream_t (default: torch's current stream).  Returns (next, mean,
        variance), None for a plane that was not asked for.  With reproj_position4 / reproj_normal4, float32 [h, w, 4]
        (motion_planes_device's outputs): rt_accumulate_plane_moving_device."""
        import torch
        dev = self._torch_device()
        h, w = _guide_tensors(value, position4, normal4, dev)
        if prim is not None:
            _need("prim", prim, torch.int32, (h, w), dev)
        if prev is not None:
            _need("prev", prev, torch.float32, (h, w, abi.HISTORY_WORDS), dev)
        next = _out("next", next, torch.float32, (h, w, abi.HISTORY_WORDS), dev)
        if out_mean is not None or want_mean:
            out_mean = _out("out_mean", out_mean, torch.float32, (h, w), dev)
        if out_variance is not None or want_variance:
            out_variance = _out("out_variance", out_variance, torch.float32, (h, w), dev)
        p = params if params is not None else accumulate_params(w, h, **kw)
        raw = self._raw_stream(stream, dev)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        for name, t in (("reproj_position4", reproj_position4), ("reproj_normal4", reproj_normal4)):
            if t is not None:
                _need(name, t, torch.float32, (h, w, 4), dev)
        if reproj_position4 is None and reproj_normal4 is None:
            _check(lib().rt_accumulate_plane_device(self._h, C.byref(p), ptr(value), ptr(position4), ptr(normal4), ptr(prim), ptr(prev),
                                                    ptr(next), ptr(out_mean), ptr(out_variance), C.c_void_p(raw)))
        else:
            _check(lib().rt_accumulate_plane_moving_device(self._h, C.byref(p), ptr(value), ptr(position4), ptr(normal4), ptr(prim),
                                                           ptr(reproj_position4), ptr(reproj_normal4), ptr(prev), ptr(next),
                                                           ptr(out_mean), ptr(out_variance), C.c_void_p(raw)))
        return next, out_mean, out_variance

    def accumulate_stats(self):
        """Work counters of the context's most recent accumulate call (rt_debug_accumulate_stats): dict of
        ACCUMULATE_STATS_KEYS."""
        return self._stats("rt_debug_accumulate_stats", ACCUMULATE_STATS_KEYS)

    def reset_history(self):
        """Forget what render_accumulated_light keeps between its calls: the next one is a first frame again.  A snapshot
        that a moving=True call left is released with it."""
        self._history = None
        if self._moving:
            self._moving = False
            self.motion_release()

    def render_accumulated_light(self, rot, cam, light, focal, sample=0, filter=False, want_parts=False, moving=False, **params):
        """render_filtered_light's direct light with its shadow term accumulated over the calls of a sequence, on the device:
        an AOV pass (position, normal, prim of AA sample `sample`), a shade call with counts whose seeds are (pixel id +
        frame index * rows * width) mod 2^24, so that every frame of a sequence draws another jitter stream, the visibility
        V = counts / shadow_samples, an accumulate call against the history and the view the object kept from its previous
        call (two history tensors alternate; params: normal_min_dot, plane_eps, max_history), and term * V_mean -> torch
        float32 [rows, W], 0 where the pixel sees nothing.  filter=True runs the a-trous filter (its defaults) over V_mean
        first; filter="variance" runs the variance-guided filter (its defaults) over V_mean and the accumulate's variance.
        want_parts: also (term, V, V_mean, variance, count), V_mean as accumulated (unfiltered), and with filter="variance" the
        filtered variance as a sixth part; sigma_value and value_eps among params are then the filter's.  reset_history() starts a new sequence.  Runs on torch's
        current stream; does not synchronise.  The same refusals as render_filtered_light.
        moving=True carries the history across triangles that a pose, a skin or an update moved between the calls: a call
        that has history computes the motion planes of its AOV planes against the snapshot (motion_planes_device) and hands
        them to the moving accumulate, and every call ends with motion_snapshot on the current stream, for the next one."""
        import torch
        if isinstance(filter, str) and filter != "variance":
            raise ValueError("filter must be False, True or \"variance\"")
        stop = {k: params.pop(k) for k in ("sigma_value", "value_eps") if filter == "variance" and k in params}
        planes, p6, hit = self._primary_hits("render_accumulated_light", rot, cam, focal, sample, bands_ok=False)
        pos, nrm, shape = planes["position"], planes["normal"], tuple(hit.shape)
        if self._history is None:
            hist = [torch.empty(shape + (abi.HISTORY_WORDS,), dtype=torch.float32, device=hit.device) for _ in range(2)]
            self._history = [hist, 0, None, 0]
        hist, cur, view, frame = self._history
        seeds = ((self._pixel_ids().to(torch.int64) + frame * hit.numel()) % abi.RT_SHADE_SEED_MAX).to(torch.int32)
        _, counts = self.shade_points_device(p6, light, seeds=seeds, want_counts=True)
        zero, vis, term = self._visibility_and_term(pos, nrm, hit, counts, light)
        if view is None:
            p, prev = accumulate_params(shape[1], shape[0], **params), None
        else:
            p, prev = accumulate_params(shape[1], shape[0], view[0], view[1], view[2], aa_x=self.cfg.aa_x, **params), hist[cur]
        rpos = rnrm = None
        if moving and prev is not None and self._moving:
            rpos, rnrm = self.motion_planes_device(planes["prim"], pos, nrm)
        nxt, vis_m, var = self.accumulate_plane_device(vis, pos, nrm, prim=planes["prim"], prev=prev, next=hist[1 - cur], params=p,
                                                       reproj_position4=rpos, reproj_normal4=rnrm)
        if moving:
            self.motion_snapshot()
            self._moving = True
        r, c, _ = self._args(rot, cam, cam)
        self._history = [hist, 1 - cur, (r, c, float(focal)), frame + 1]
        var_f = None
        if filter == "variance":
            vis_o, var_f = self.filter_plane_variance_device(vis_m, var, pos, nrm, **stop)
        else:
            vis_o = self.filter_plane_device(vis_m, pos, nrm) if filter else vis_m
        out = term * torch.where(hit, vis_o, zero)
        if not want_parts:
            return out
        parts = (out, term, vis, vis_m, var, nxt[..., abi.HISTORY_COUNT].clone())
        return parts + (var_f,) if var_f is not None else parts

    def shade_stats(self):
        """Work counters of the context's most recent shade call (rt_debug_shade_stats): dict of SHADE_STATS_KEYS."""
        return self._stats("rt_debug_shade_stats", SHADE_STATS_KEYS)

    def radiance_rays(self, rays, light, seeds=None, want_prim=False):
        """The frame's full colour along caller rays (rt_radiance_rays), blocking: rays [k,6] = start, direction (used as
        given), seeds int32 [k] = the global_id of each ray's jitter stream (None: k & 0xFFFFFF; the frame uses the pixel
        id) -> rgba float32 [k,4]: xyz the colour rt_render gives that ray (bounces and soft shadows included), w = 1 where
        the ray hits anything, else 0; with want_prim also the first hit int32 [k] (-1 / -2 / original triangle index)."""
        rays = _rays6(rays)
        k = rays.shape[0]
        li = _light3(light)
        sp = _seeds_ptr(seeds, k, "ray")
        out = np.zeros((k, 4), np.float32)
        prim = np.zeros(k, np.int32) if want_prim else None
        _check(lib().rt_radiance_rays(self._h, _fp(rays), sp, k, _fp(li), _fp(out), _ip(prim)))
        return (out, prim) if want_prim else out

    def radiance_rays_device(self, rays6, light, seeds=None, out=None, out_prim=None, stream=None):
        """Enqueue rt_radiance_rays_device on torch tensors of the context's device, without synchronising.  rays6: float32
        [k,6] (start, direction); seeds: int32 [k] or None; out: float32 [k,4] (allocated when None); out_prim: int32 [k] or
        None (not computed).  stream: a torch stream or a raw hipStream_t (default: torch's current stream).  Returns out,
        or (out, out_prim) when out_prim is given."""
        import torch
        dev = self._torch_device()
        k = _rows("rays6", rays6, 6, dev)
        if seeds is not None:
            _need("seeds", seeds, torch.int32, (k,), dev)
        out = _out("out", out, torch.float32, (k, 4), dev)
        if out_prim is not None:
            _need("out_prim", out_prim, torch.int32, (k,), dev)
        li = _light3(light)
        raw = self._raw_stream(stream, dev)
        if k:
            _check(lib().rt_radiance_rays_device(self._h, C.c_void_p(rays6.data_ptr()),
                                                 C.c_void_p(seeds.data_ptr() if seeds is not None else 0), k, _fp(li),
                                                 C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(out_prim.data_ptr() if out_prim is not None else 0),
                                                 C.c_void_p(raw)))
        return out if out_prim is None else (out, out_prim)

    def radiance_stats(self):
        """Work counters of the context's most recent radiance call (rt_debug_radiance_stats): dict of RADIANCE_STATS_KEYS."""
        return self._stats("rt_debug_radiance_stats", RADIANCE_STATS_KEYS)

    def render_panorama(self, width, height, cam, light, yaw=0.0):
        """An equirectangular 360 x 180 degree view from `cam`, on the device (rt_radiance_rays_device) -> torch float32
        [height, width, 4], rgb the frame's colour and w the coverage.  Pixel (x, y) looks along
            (sin(phi) * cos(theta), sin(theta), cos(phi) * cos(theta)),
            phi = yaw + 2 * pi * (x + 0.5) / width - pi,   theta = pi * (y + 0.5) / height - pi / 2,
        evaluated in float32 with torch on the device, left to right as written (x + 0.5 and y + 0.5 from float32 aranges;
        2 * pi, pi and pi / 2 are the float32 values of math.pi's multiples; yaw a float32 scalar); the ray starts at cam
        and its seed is (y * width + x) & 0xFFFFFF.  Runs on torch's current stream; does not synchronise."""
        import math
        import torch
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError("width and height must be positive")
        dev = self._torch_device()
        f32 = dict(dtype=torch.float32, device=dev)
        xs = (torch.arange(width, **f32) + 0.5) * torch.tensor(2.0 * math.pi, **f32) / torch.tensor(float(width), **f32)
        phi = torch.tensor(float(yaw), **f32) + xs - torch.tensor(math.pi, **f32)
        theta = (torch.arange(height, **f32) + 0.5) * torch.tensor(math.pi, **f32) / torch.tensor(float(height), **f32) \
            - torch.tensor(math.pi / 2.0, **f32)
        ct = torch.cos(theta)[:, None]
        d = torch.stack([torch.sin(phi)[None, :] * ct, torch.sin(theta)[:, None].expand(height, width),
                         torch.cos(phi)[None, :] * ct], -1)
        start = torch.tensor(np.ascontiguousarray(cam, np.float32)[:3].copy(), device=dev).expand(height, width, 3)
        rays = torch.cat([start, d], -1).reshape(-1, 6).contiguous()
        seeds = (torch.arange(width * height, dtype=torch.int64, device=dev) & abi.RT_SHADE_SEED_MASK).to(torch.int32)
        return self.radiance_rays_device(rays, light, seeds=seeds).reshape(height, width, 4)

    def trace_stats(self):
        """Work counters of the context's most recent query (rt_debug_trace_stats): dict of TRACE_STATS_KEYS."""
        return self._stats("rt_debug_trace_stats", TRACE_STATS_KEYS)

    def wave_timeline(self):
        """Wave kernel, context created with UOB_RT_TIMELINE=1: start / end statistics of the last frame's persistent waves
        in 100 MHz ticks (rt_debug_wave_timeline)."""
        out = (C.c_uint64 * 8)()
        _check(lib().rt_debug_wave_timeline(self._h, out))
        n = max(int(out[0]), 1)
        first, last = int(out[1]), int(out[2])
        return {"waves": int(out[0]), "span_us": (last - first) / 100.0, "mean_start_us": (int(out[3]) / n - first) / 100.0,
                "mean_idle_tail_us": (last - int(out[4]) / n) / 100.0, "jobs": int(out[5]), "max_jobs_per_wave": int(out[6]), "listed_jobs": int(out[7])}

    def _wave_seed_records(self, export, ncounters):
        """rt_debug_wave_seeds / rt_debug_wave_seeds_wide, asked for the tile grid first and then for its records: -> (dict
        tile_rows, tiles_per_row, rows_per_tile, `records` [tile_rows, tiles_per_row] of SEED_DTYPE; the export's counters)."""
        fn = getattr(lib(), export)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        dims, cnt = (C.c_int32 * 3)(), (C.c_uint64 * ncounters)()
        _check(fn(self._h, None, 0, dims, cnt))
        rec = np.zeros((int(dims[0]), int(dims[1])), SEED_DTYPE)
        if rec.size:
            _check(fn(self._h, rec.ctypes.data_as(C.c_void_p), rec.size, dims, cnt))
        return {"tile_rows": int(dims[0]), "tiles_per_row": int(dims[1]), "rows_per_tile": int(dims[2]), "records": rec}, cnt

    def wave_seeds(self):
        """Wave kernel: the tile seeds of the last frame (rt_debug_wave_seeds).  -> dict: tile_rows, tiles_per_row, rows_per_tile
        (all 0 when the frame took no seed), tiles_primary, tiles_shadow, jobs_primary, jobs_shadow, and `records`, a
        structured array [tile_rows, tiles_per_row] of SEED_DTYPE."""
        d, cnt = self._wave_seed_records("rt_debug_wave_seeds", 4)
        d.update(tiles_primary=int(cnt[0]), tiles_shadow=int(cnt[1]), jobs_primary=int(cnt[2]), jobs_shadow=int(cnt[3]))
        return d

    def wave_seeds_wide(self):
        """Wave kernel: the tile seeds of the last frame as the draw kernel reads them (rt_debug_wave_seeds_wide).  -> dict:
        tile_rows, tiles_per_row, rows_per_tile, tiles_<k> and jobs_<k> for k in SEED_WIDE_KEYS (records with a primary part,
        a shadow part, and of those the ones with casters off h's plane, a sphere candidate, blocked), and the raw `records`."""
        d, cnt = self._wave_seed_records("rt_debug_wave_seeds_wide", 10)
        for q, k in enumerate(SEED_WIDE_KEYS):
            d["tiles_" + k], d["jobs_" + k] = int(cnt[2 * q]), int(cnt[2 * q + 1])
        return d

    def world_masks(self):
        """Mesh kernel: the last frame's shadow-ray tile masks, uint64 [G, G, G, words] indexed [z, y, x] (rt_debug_world_masks)."""
        g, w = C.c_int32(), C.c_int32()
        n = _check(lib().rt_debug_world_masks(self._h, None, 0, C.byref(g), C.byref(w)))
        out = np.zeros(n, np.uint64)
        _check(lib().rt_debug_world_masks(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.byref(g), C.byref(w)))
        return out.reshape(g.value, g.value, g.value, w.value)

    def block_costs(self):
        """Mesh kernel: s_memtime ticks of every 16x16-pixel block of the last frame, [rows/16, W/16] (rt_debug_block_costs)."""
        n = _check(lib().rt_debug_block_costs(self._h, None, 0))
        out = np.zeros(n, np.uint32)
        _check(lib().rt_debug_block_costs(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out.reshape((self.rows + 15) // 16, (self.width + 15) // 16)

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(lib().rt_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)
