"""CPU: the filter entry points (rt_filter_params_default, rt_filter_plane, rt_filter_plane_device, rt_debug_filter_stats,
rt_filter_plane_host) are declared, exported and bound, reject bad arguments without touching a device, and their gfx950
kernels are part of the library build."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import filter_util as fu
from uob_raytracer_amd import abi, runtime as rt

NEW = ("rt_filter_params_default", "rt_filter_plane", "rt_filter_plane_device", "rt_debug_filter_stats", "rt_filter_plane_host")
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
    for method in ("filter_plane", "filter_plane_device", "filter_stats", "render_filtered_light"):
        assert callable(getattr(rt.RayTracer, method))
    assert callable(rt.filter_plane_host)
    assert len(rt.FILTER_STATS_KEYS) == 8
    assert C.sizeof(abi.RtFilterParams) == 24


def test_the_defaults():
    p = rt.filter_params(320, 200)
    assert (p.width, p.height, p.passes) == (320, 200, 5)
    assert p.normal_min_dot == np.float32(0.9) and p.plane_eps == np.float32(0.01) and p.value_max_diff == math.inf
    assert "not tuned on images" in open(os.path.join(ROOT, "include", "uob_rt.h")).read()


def _planes(h=3, w=4):
    return np.zeros((h, w), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)


BAD_FIELDS = [("width", 0), ("width", -3), ("height", 0), ("passes", 0), ("passes", 9), ("normal_min_dot", math.nan),
              ("plane_eps", -0.5), ("plane_eps", math.nan), ("value_max_diff", -1.0), ("value_max_diff", math.nan),
              ("value_max_diff", -math.inf)]


@pytest.mark.parametrize("field,bad", BAD_FIELDS)
def test_a_parameter_out_of_range_is_invalid_without_a_device(field, bad):
    L = rt.lib()
    v, pos, nrm, out = _planes()
    fake = C.c_void_p(16)             # never dereferenced: every case fails its argument check first
    p = rt.filter_params(4, 3)
    setattr(p, field, bad)
    for rc in (L.rt_filter_plane(fake, C.byref(p), rt._fp(v), rt._fp(pos), rt._fp(nrm), rt._fp(out)),
               L.rt_filter_plane_device(fake, C.byref(p), fake, fake, fake, fake, None),
               L.rt_filter_plane_host(C.byref(p), rt._fp(v), rt._fp(pos), rt._fp(nrm), rt._fp(out))):
        assert rc == abi.RT_E_INVALID
        assert field.encode() in L.rt_last_error()


def test_too_many_pixels_are_invalid():
    L = rt.lib()
    v, pos, nrm, out = _planes()
    fake = C.c_void_p(16)
    p = rt.filter_params(1 << 16, (1 << 15) + 1)
    assert L.rt_filter_plane_device(fake, C.byref(p), fake, fake, fake, fake, None) == abi.RT_E_INVALID
    assert b"width * height" in L.rt_last_error()
    assert L.rt_filter_plane_host(C.byref(p), rt._fp(v), rt._fp(pos), rt._fp(nrm), rt._fp(out)) == abi.RT_E_INVALID


def test_null_arguments_are_invalid_without_a_device():
    L = rt.lib()
    v, pos, nrm, out = _planes()
    fake = C.c_void_p(16)
    p = rt.filter_params(4, 3)
    host = [rt._fp(v), rt._fp(pos), rt._fp(nrm), rt._fp(out)]
    assert L.rt_filter_plane(None, C.byref(p), *host) == abi.RT_E_INVALID
    assert b"ctx" in L.rt_last_error()
    assert L.rt_filter_plane_device(None, C.byref(p), fake, fake, fake, fake, None) == abi.RT_E_INVALID
    assert L.rt_filter_plane(fake, None, *host) == abi.RT_E_INVALID
    assert b"params" in L.rt_last_error()
    assert L.rt_filter_plane_device(fake, None, fake, fake, fake, fake, None) == abi.RT_E_INVALID
    assert L.rt_filter_plane_host(None, *host) == abi.RT_E_INVALID
    for k in range(4):
        args = list(host)
        args[k] = None
        assert L.rt_filter_plane(fake, C.byref(p), *args) == abi.RT_E_INVALID
        assert b"NULL plane" in L.rt_last_error()
        assert L.rt_filter_plane_host(C.byref(p), *args) == abi.RT_E_INVALID
        dev = [fake] * 4
        dev[k] = None
        assert L.rt_filter_plane_device(fake, C.byref(p), *dev, None) == abi.RT_E_INVALID
    # guides the kernels could not load as float4
    assert L.rt_filter_plane_device(fake, C.byref(p), fake, C.c_void_p(20), fake, fake, None) == abi.RT_E_INVALID
    assert b"16-byte aligned" in L.rt_last_error()
    stats = (C.c_uint64 * 8)()
    assert L.rt_debug_filter_stats(None, stats) == abi.RT_E_INVALID
    assert L.rt_debug_filter_stats(fake, None) == abi.RT_E_INVALID


def test_python_wrappers_refuse_wrong_planes():
    v, pos, nrm, out = _planes()
    with pytest.raises(ValueError):
        rt.filter_plane_host(v, pos[:2], nrm)
    with pytest.raises(ValueError):
        rt.filter_plane_host(v, pos, nrm, out=np.zeros((3, 4), np.float64))
    with pytest.raises(rt.RtError) as e:
        rt.filter_plane_host(v, pos, nrm, passes=0)
    assert e.value.code == abi.RT_E_INVALID


def test_filter_kernels_are_built_for_gfx950():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rt_filter.hip" in srcs and "filter_host.cpp" in srcs
    assert re.search(r"^ARCH\s*\?=\s*gfx950\s*$", mk, re.M)
    assert re.search(r"kernel-resource-usage -c rt_filter\.hip", mk)
    blob = open(rt.LIB_PATH, "rb").read()
    stubs = [b"rt_filter_pack", b"rt_filter_direct"] + [b"rt_filter_tiledILi%dEEE" % s for s in (1, 2, 4, 8, 16, 32)]
    for inst in stubs:
        assert inst in blob             # the guide packing, the direct form, the tiled form at every spacing it serves
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    # the host statement is host code only: no kernel, no HIP call
    host = open(os.path.join(CSRC, "filter_host.cpp")).read()
    assert "__global__" not in host and "hip_runtime" not in host and "rt_host.h" not in host


def test_the_restated_thresholds_are_the_kernels():
    """tests/filter_util.py restates the tile, the largest tiled spacing and the row groups per grid.y; the sizes of the GPU
    tests are built from them, so they must be the constants the kernels are compiled with."""
    host = open(os.path.join(CSRC, "rt_host.h")).read()
    kern = open(os.path.join(CSRC, "rt_filter.hip")).read()
    m = re.search(r"constexpr int kFilterTX = (\d+), kFilterTY = (\d+), kFilterMaxTiledSpacing = (\d+);", host)
    assert m and tuple(int(x) for x in m.groups()) == (fu.FILTER_TX, fu.FILTER_TY, fu.MAX_TILED_SPACING)
    m = re.search(r"constexpr int kRowGroupsY = (\d+);", kern)
    assert m and int(m.group(1)) == fu.ROW_GROUPS_Y
    assert re.search(r"constexpr int TX = kFilterTX, TY = kFilterTY;", kern)
    # the tiled form is instantiated for every spacing up to the largest, and for no other
    spacings = sorted(int(x) for x in re.findall(r"launch_tiled<(\d+)>\(", kern))
    assert spacings == [1 << i for i in range(fu.MAX_TILED_SPACING.bit_length())]
    fu.check_sizes()
