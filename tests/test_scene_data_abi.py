"""CPU: the scene readback rt_debug_scene_data is declared with the documented signature, exported and bound, and rejects
a NULL context and a bad capacity with RT_E_INVALID and a message before any device work (no device is present here)."""
import ctypes as C
import os
import re

from conftest import ROOT
from uob_raytracer_amd import abi, runtime as rt

SIGNATURE = (r"int rt_debug_scene_data\(rt_ctx\* \w+, float\* \w+, float\* \w+, float\* \w+, float\* \w+, float\* \w+, "
             r"float\* \w+, int32_t\* \w+, float \w+\[3\], float \w+\[3\], int32_t \w+\);")


def _invalid(rc, *words):
    assert rc == abi.RT_E_INVALID
    msg = rt.lib().rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_declared_exported_and_bound():
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "uob_rt.h")).read())
    assert re.search(SIGNATURE, src)
    assert hasattr(C.CDLL(rt.LIB_PATH), "rt_debug_scene_data")
    assert "rt_debug_scene_data" in rt.EXPORTS
    fp = C.POINTER(C.c_float)
    assert rt.lib().rt_debug_scene_data.argtypes == [C.c_void_p] + [fp] * 6 + [C.POINTER(C.c_int32), fp, fp, C.c_int32]
    assert callable(rt.RayTracer.scene_data)


def test_null_context_and_bad_capacity_are_invalid():
    f = rt.lib().rt_debug_scene_data
    nothing = [None] * 9
    _invalid(f(None, *nothing, 0), "rt_debug_scene_data", "NULL context")
    _invalid(f(None, *nothing, 100), "rt_debug_scene_data", "NULL context")
    _invalid(f(None, *nothing, -1), "rt_debug_scene_data", "capacity -1")     # too small for any scene, whatever the context
    _invalid(f(C.c_void_p(0), *nothing, -(2 ** 31)), "capacity")
