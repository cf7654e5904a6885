"""CPU: the accumulate entry points (rt_accumulate_params_default, rt_accumulate_plane, rt_accumulate_plane_device,
rt_debug_accumulate_stats, rt_accumulate_plane_host) are declared, exported and bound, reject bad arguments without touching a
device, and their gfx950 kernel is part of the library build."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import accumulate_util as au
from uob_raytracer_amd import abi, runtime as rt

NEW = ("rt_accumulate_params_default", "rt_accumulate_plane", "rt_accumulate_plane_device", "rt_debug_accumulate_stats",
       "rt_accumulate_plane_host")
CSRC = os.path.join(ROOT, "uob_raytracer_amd", "csrc")


def test_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "uob_rt.h")).read()
    lib = C.CDLL(rt.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src)
        assert hasattr(lib, name)
        assert name in rt.EXPORTS
        assert getattr(rt.lib(), name).argtypes is not None
    assert re.search(r"#define\s+RT_ABI_VERSION\s+2\b", src)
    assert rt.lib().rt_abi_version() == abi.RT_ABI_VERSION == 2
    for method in ("accumulate_plane", "accumulate_plane_device", "accumulate_stats", "render_accumulated_light", "reset_history"):
        assert callable(getattr(rt.RayTracer, method))
    assert callable(rt.accumulate_plane_host) and callable(rt.accumulate_params)
    assert len(rt.ACCUMULATE_STATS_KEYS) == 8
    assert C.sizeof(abi.RtAccumulateParams) == 84 and C.sizeof(abi.RtHistoryTexel) == 48
    assert abi.HISTORY_WORDS * 4 == 48 == au.WORDS * 4
    assert (abi.HISTORY_MEAN, abi.HISTORY_M2, abi.HISTORY_COUNT, abi.HISTORY_PRIM) == (au.MEAN, au.M2, au.COUNT, au.PRIM)
    assert abi.RtHistoryTexel.mean.offset == 12 and abi.RtHistoryTexel.m2.offset == 28
    assert abi.RtHistoryTexel.count.offset == 32 and abi.RtHistoryTexel.prim.offset == 36


def test_the_defaults():
    p = rt.accumulate_params(320, 200)
    assert (p.width, p.height, p.max_history) == (320, 200, 32)
    assert list(p.prev_rot) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and list(p.prev_cam) == [0, 0, 0]
    assert p.prev_focal_px == 320
    assert p.normal_min_dot == np.float32(0.9) and p.plane_eps == np.float32(0.01)
    assert rt.accumulate_params(320, 200, prev_focal=640.0, aa_x=2).prev_focal_px == 320
    assert open(os.path.join(ROOT, "include", "uob_rt.h")).read().count("stated, not tuned on images") == 2


def _planes(h=3, w=4):
    return (np.zeros((h, w), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32),
            np.zeros((h, w), np.int32), np.zeros((h, w, 12), np.float32), np.zeros((h, w, 12), np.float32),
            np.zeros((h, w), np.float32), np.zeros((h, w), np.float32))


def _host_args(planes):
    v, pos, nrm, prim, prev, nxt, mean, var = planes
    return [rt._fp(v), rt._fp(pos), rt._fp(nrm), rt._ip(prim), rt._fp(prev), rt._fp(nxt), rt._fp(mean), rt._fp(var)]


def _set(p, field, bad):
    if "[" in field:
        name, k = field[:-1].split("[")
        getattr(p, name)[int(k)] = bad
    else:
        setattr(p, field, bad)


BAD_FIELDS = [("width", 0), ("width", -3), ("height", 0), ("prev_rot[7]", math.nan), ("prev_rot[0]", math.inf),
              ("prev_cam[2]", math.nan), ("prev_cam[0]", -math.inf), ("prev_focal_px", 0.0), ("prev_focal_px", -1.0),
              ("prev_focal_px", math.nan), ("prev_focal_px", math.inf), ("normal_min_dot", math.nan), ("plane_eps", -0.5),
              ("plane_eps", math.nan), ("max_history", 0), ("max_history", 65537)]


@pytest.mark.parametrize("field,bad", BAD_FIELDS)
def test_a_parameter_out_of_range_is_invalid_without_a_device(field, bad):
    L = rt.lib()
    host = _host_args(_planes())
    fake = C.c_void_p(16)             # never dereferenced: every case fails its argument check first
    other = C.c_void_p(32)
    p = rt.accumulate_params(4, 3)
    _set(p, field, bad)
    for rc in (L.rt_accumulate_plane(fake, C.byref(p), *host),
               L.rt_accumulate_plane_device(fake, C.byref(p), fake, fake, fake, fake, fake, other, fake, fake, None),
               L.rt_accumulate_plane_host(C.byref(p), *host)):
        assert rc == abi.RT_E_INVALID
        assert field.encode() in L.rt_last_error()


def test_too_many_pixels_are_invalid():
    L = rt.lib()
    host = _host_args(_planes())
    fake, other = C.c_void_p(16), C.c_void_p(32)
    p = rt.accumulate_params(1 << 16, (1 << 15) + 1)
    assert L.rt_accumulate_plane_device(fake, C.byref(p), fake, fake, fake, fake, fake, other, fake, fake, None) == abi.RT_E_INVALID
    assert b"width * height" in L.rt_last_error()
    assert L.rt_accumulate_plane_host(C.byref(p), *host) == abi.RT_E_INVALID


def test_null_arguments_and_aliased_histories_are_invalid_without_a_device():
    L = rt.lib()
    host = _host_args(_planes())
    fake, other = C.c_void_p(16), C.c_void_p(32)
    dev = [fake, fake, fake, fake, fake, other, fake, fake]
    p = rt.accumulate_params(4, 3)
    assert L.rt_accumulate_plane(None, C.byref(p), *host) == abi.RT_E_INVALID
    assert b"ctx" in L.rt_last_error()
    assert L.rt_accumulate_plane_device(None, C.byref(p), *dev, None) == abi.RT_E_INVALID
    assert b"ctx" in L.rt_last_error()
    assert L.rt_accumulate_plane(fake, None, *host) == abi.RT_E_INVALID
    assert b"params" in L.rt_last_error()
    assert L.rt_accumulate_plane_device(fake, None, *dev, None) == abi.RT_E_INVALID
    assert L.rt_accumulate_plane_host(None, *host) == abi.RT_E_INVALID
    for k in (0, 1, 2, 5):            # value, position4, normal4, next: required
        args = list(host)
        args[k] = None
        assert L.rt_accumulate_plane(fake, C.byref(p), *args) == abi.RT_E_INVALID
        assert b"NULL plane" in L.rt_last_error()
        assert L.rt_accumulate_plane_host(C.byref(p), *args) == abi.RT_E_INVALID
        d = list(dev)
        d[k] = None
        assert L.rt_accumulate_plane_device(fake, C.byref(p), *d, None) == abi.RT_E_INVALID
    # next == prev
    args = list(host)
    args[5] = args[4]
    assert L.rt_accumulate_plane(fake, C.byref(p), *args) == abi.RT_E_INVALID
    assert b"next" in L.rt_last_error() and b"prev" in L.rt_last_error()
    assert L.rt_accumulate_plane_host(C.byref(p), *args) == abi.RT_E_INVALID
    d = list(dev)
    d[5] = d[4]
    assert L.rt_accumulate_plane_device(fake, C.byref(p), *d, None) == abi.RT_E_INVALID
    assert b"next" in L.rt_last_error()
    # guides or histories the kernel could not load as float4
    for k, name in ((1, b"d_position4"), (2, b"d_normal4"), (4, b"d_prev"), (5, b"d_next")):
        d = list(dev)
        d[k] = C.c_void_p(52)
        assert L.rt_accumulate_plane_device(fake, C.byref(p), *d, None) == abi.RT_E_INVALID
        assert b"16-byte aligned" in L.rt_last_error() and name in L.rt_last_error()
    stats = (C.c_uint64 * 8)()
    assert L.rt_debug_accumulate_stats(None, stats) == abi.RT_E_INVALID
    assert L.rt_debug_accumulate_stats(fake, None) == abi.RT_E_INVALID


def test_python_wrappers_refuse_wrong_planes():
    v, pos, nrm, prim, prev = _planes()[:5]
    with pytest.raises(ValueError):
        rt.accumulate_plane_host(v, pos[:2], nrm)
    with pytest.raises(ValueError):
        rt.accumulate_plane_host(v, pos, nrm, prim[:, :2])
    with pytest.raises(ValueError):
        rt.accumulate_plane_host(v, pos, nrm, prim, prev[..., :8])
    with pytest.raises(TypeError):
        rt.accumulate_params(4, 3, passes=2)
    with pytest.raises(rt.RtError) as e:
        rt.accumulate_plane_host(v, pos, nrm, max_history=0)
    assert e.value.code == abi.RT_E_INVALID


def test_accumulate_kernel_is_built_for_gfx950():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rt_accumulate.hip" in srcs and "accumulate_host.cpp" in srcs
    assert re.search(r"^ARCH\s*\?=\s*gfx950\s*$", mk, re.M)
    assert re.search(r"kernel-resource-usage -c rt_accumulate\.hip", mk)
    blob = open(rt.LIB_PATH, "rb").read()
    for stub in (b"rt_accumulate_pixels", b"rt_accumulate_counters"):
        assert stub in blob
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    # the host statement is host code only: no kernel, no HIP call
    host = open(os.path.join(CSRC, "accumulate_host.cpp")).read()
    assert "__global__" not in host and "hip_runtime" not in host and "rt_host.h" not in host


def test_the_restated_tile_is_the_kernels():
    """tests/accumulate_util.py restates the tile and the row groups per grid.y; the sizes of the GPU tests are built from them,
    so they must be the constants the kernel is compiled with."""
    host = open(os.path.join(CSRC, "rt_host.h")).read()
    kern = open(os.path.join(CSRC, "rt_accumulate.hip")).read()
    m = re.search(r"constexpr int kFilterTX = (\d+), kFilterTY = (\d+),", host)
    assert m and tuple(int(x) for x in m.groups()) == (au.TILE_TX, au.TILE_TY)
    m = re.search(r"constexpr int kRowGroupsY = (\d+);", kern)
    assert m and int(m.group(1)) == au.ROW_GROUPS_Y
    assert re.search(r"constexpr int TX = kFilterTX, TY = kFilterTY;", kern)
    au.check_sizes()
