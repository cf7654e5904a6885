"""CPU: the scene-edit entry points (rt_replace_scene, rt_replace_scene_device, rt_update_spheres, rt_debug_scene_capacity)
are declared with the documented signatures, exported and bound, and reject bad arguments with RT_E_INVALID and a message
before any device work (no device is present here)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from uob_raytracer_amd import abi, runtime as rt

SIGNATURES = {
    "rt_replace_scene": r"int rt_replace_scene\(rt_ctx\* \w+, const float\* \w+, const float\* \w+, const float\* \w+, "
                        r"int32_t \w+, uint32_t \w+\);",
    "rt_replace_scene_device": r"int rt_replace_scene_device\(rt_ctx\* \w+, const void\* \w+, const void\* \w+, "
                               r"const void\* \w+, int32_t \w+, uint32_t \w+, void\* \w+\);",
    "rt_update_spheres": r"int rt_update_spheres\(rt_ctx\* \w+, const rt_sphere\* \w+, int32_t \w+\);",
    "rt_debug_scene_capacity": r"int rt_debug_scene_capacity\(rt_ctx\* \w+, int64_t\* \w+\);",
}


def _invalid(rc, *words):
    assert rc == abi.RT_E_INVALID
    msg = rt.lib().rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_declared_exported_and_bound():
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "uob_rt.h")).read())
    lib = C.CDLL(rt.LIB_PATH)
    for name, sig in SIGNATURES.items():
        assert re.search(sig, src), name
        assert hasattr(lib, name)
        assert name in rt.EXPORTS
        assert getattr(rt.lib(), name).argtypes is not None
    assert int(re.search(r"#define RT_UPDATE_DEVICE_TILES (\d+)u", src).group(1)) == abi.RT_UPDATE_DEVICE_TILES == 2
    assert int(re.search(r"#define RT_UPDATE_REORDER (\d+)u", src).group(1)) == abi.RT_UPDATE_REORDER == 1
    assert rt.lib().rt_abi_version() == abi.RT_ABI_VERSION == 2
    for method in ("replace_scene", "replace_scene_device", "update_spheres", "scene_capacity"):
        assert callable(getattr(rt.RayTracer, method))


def test_null_context_is_invalid():
    L = rt.lib()
    v, n = np.zeros((3, 4), np.float32), np.zeros((1, 4), np.float32)
    _invalid(L.rt_replace_scene(None, rt._fp(v), rt._fp(n), rt._fp(n), 1, 0), "NULL")
    _invalid(L.rt_replace_scene_device(None, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1, 0, None), "NULL")
    _invalid(L.rt_update_spheres(None, (abi.RtSphere * 4)(), 2), "NULL")
    _invalid(L.rt_debug_scene_capacity(None, C.byref(C.c_int64())), "NULL")


def test_bad_arguments_are_invalid_before_any_device_work():
    """With a context handle that is never dereferenced for device work: the argument checks come first.  (The handle is a
    zeroed block of host memory, large enough for any rt_ctx; the checks below read nothing of it.)"""
    L = rt.lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    v, n = np.zeros((3, 4), np.float32), np.zeros((1, 4), np.float32)
    # NULL arrays
    _invalid(L.rt_replace_scene(h, None, rt._fp(n), rt._fp(n), 1, 0), "NULL")
    _invalid(L.rt_replace_scene(h, rt._fp(v), None, rt._fp(n), 1, 0), "NULL")
    _invalid(L.rt_replace_scene(h, rt._fp(v), rt._fp(n), None, 1, 0), "NULL")
    _invalid(L.rt_replace_scene_device(h, None, None, None, 1, 0, None), "NULL")
    # n_new <= 0
    for bad in (0, -1):
        _invalid(L.rt_replace_scene(h, rt._fp(v), rt._fp(n), rt._fp(n), bad, 0), "n_new")
        _invalid(L.rt_replace_scene_device(h, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), bad, 0, None), "n_new")
    # an unknown flag bit; the two known ones exclude each other
    _invalid(L.rt_replace_scene(h, rt._fp(v), rt._fp(n), rt._fp(n), 1, 4), "flags")
    _invalid(L.rt_replace_scene_device(h, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1, 0x80000000, None), "flags")
    both = abi.RT_UPDATE_REORDER | abi.RT_UPDATE_DEVICE_TILES
    _invalid(L.rt_replace_scene(h, rt._fp(v), rt._fp(n), rt._fp(n), 1, both), "exclude")
    # a vertex outside the bound is caught on the host, before the device is looked for
    bad_v = v.copy()
    bad_v[1, 2] = np.float32(2.0 ** 17)
    _invalid(L.rt_replace_scene(h, rt._fp(bad_v), rt._fp(n), rt._fp(n), 1, 0), "2^16")
    bad_v[1, 2] = np.nan
    _invalid(L.rt_replace_scene(h, rt._fp(bad_v), rt._fp(n), rt._fp(n), 1, 0), "finite")
    # sphere tables
    tab = (abi.RtSphere * 4)()
    _invalid(L.rt_update_spheres(h, tab, -1), "num_spheres")
    _invalid(L.rt_update_spheres(h, tab, abi.RT_MAX_SPHERES + 1), "num_spheres")
    _invalid(L.rt_update_spheres(h, None, 1), "NULL")
    tab[1].center[0] = float("nan")
    _invalid(L.rt_update_spheres(h, tab, 2), "sphere 1")
    tab[1].center[0] = 2.0 ** 17
    _invalid(L.rt_update_spheres(h, tab, 2), "sphere 1")
    tab[1].center[0] = 0.0
    tab[0].radius_sq = float("inf")
    _invalid(L.rt_update_spheres(h, tab, 1), "radius_sq")
    _invalid(L.rt_debug_scene_capacity(h, None), "NULL")


def test_update_entries_know_the_new_flag():
    """rt_update_scene* accept RT_UPDATE_DEVICE_TILES in their flag check (the NULL context is reported first, an unknown
    bit is still refused for a context)."""
    L = rt.lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)                      # zeroed: a context of 0 triangles as far as the checks look
    assert L.rt_update_scene(h, None, None, None, 0, abi.RT_UPDATE_DEVICE_TILES) == abi.RT_OK
    _invalid(L.rt_update_scene(h, None, None, None, 0, 4), "flags")
    _invalid(L.rt_update_scene(h, None, None, None, 0, 3), "exclude")
