"""CPU: the ray-query entry points (rt_trace_rays, rt_trace_rays_device, rt_debug_trace_stats) are declared, exported and
bound, reject bad arguments without touching a device, and their gfx950 kernels are part of the library build."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from uob_raytracer_amd import abi, runtime as rt

NEW = ("rt_trace_rays", "rt_trace_rays_device", "rt_debug_trace_stats")
CSRC = os.path.join(ROOT, "uob_raytracer_amd", "csrc")


def test_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "uob_rt.h")).read()
    lib = C.CDLL(rt.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src)
        assert hasattr(lib, name)
        assert name in rt.EXPORTS
        assert getattr(rt.lib(), name).argtypes is not None
    assert rt.lib().rt_abi_version() == abi.RT_ABI_VERSION == 2


def test_bad_arguments_are_invalid_without_a_device():
    L = rt.lib()
    rays = np.zeros((4, 6), np.float32)
    r2 = np.ones(4, np.float32)
    tri = np.zeros(4, np.int32)
    out = np.zeros((4, 10), np.float32)
    ip = tri.ctypes.data_as(C.POINTER(C.c_int32))
    fake = C.c_void_p(16)             # never dereferenced: every case fails its argument check first
    for what in (abi.RT_TRACE_IN_SHADOW, abi.RT_TRACE_CLOSEST_HIT):
        assert L.rt_trace_rays(None, what, rt._fp(rays), rt._fp(r2), 4, ip, rt._fp(out)) == abi.RT_E_INVALID
        assert L.rt_trace_rays_device(None, what, fake, fake, 4, fake, fake, None) == abi.RT_E_INVALID
    assert b"NULL" in L.rt_last_error()
    # NULL rays / out_tri, unknown mode, nray < 0, missing radius_sq: checked before the context is used
    assert L.rt_trace_rays(fake, abi.RT_TRACE_CLOSEST_HIT, None, None, 4, ip, rt._fp(out)) == abi.RT_E_INVALID
    assert L.rt_trace_rays(fake, abi.RT_TRACE_CLOSEST_HIT, rt._fp(rays), None, 4, None, rt._fp(out)) == abi.RT_E_INVALID
    assert L.rt_trace_rays(fake, 7, rt._fp(rays), rt._fp(r2), 4, ip, rt._fp(out)) == abi.RT_E_INVALID
    assert b"unknown mode" in L.rt_last_error()
    assert L.rt_trace_rays(fake, abi.RT_TRACE_CLOSEST_HIT, rt._fp(rays), None, -1, ip, None) == abi.RT_E_INVALID
    assert L.rt_trace_rays(fake, abi.RT_TRACE_IN_SHADOW, rt._fp(rays), None, 4, ip, None) == abi.RT_E_INVALID
    assert b"radius_sq" in L.rt_last_error()
    assert L.rt_trace_rays_device(fake, abi.RT_TRACE_CLOSEST_HIT, None, None, 4, fake, fake, None) == abi.RT_E_INVALID
    assert L.rt_trace_rays_device(fake, abi.RT_TRACE_CLOSEST_HIT, fake, None, 4, None, fake, None) == abi.RT_E_INVALID
    assert L.rt_trace_rays_device(fake, -1, fake, fake, 4, fake, fake, None) == abi.RT_E_INVALID
    assert L.rt_trace_rays_device(fake, abi.RT_TRACE_IN_SHADOW, fake, fake, -5, fake, None, None) == abi.RT_E_INVALID
    assert L.rt_trace_rays_device(fake, abi.RT_TRACE_IN_SHADOW, fake, None, 4, fake, None, None) == abi.RT_E_INVALID
    stats = (C.c_uint64 * 8)()
    assert L.rt_debug_trace_stats(None, stats) == abi.RT_E_INVALID
    assert L.rt_debug_trace_stats(fake, None) == abi.RT_E_INVALID


def test_query_kernels_are_built_for_gfx950():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rt_ray_query.hip" in srcs and "rt_tiles.h" in hdrs
    assert re.search(r"^ARCH\s*\?=\s*gfx950\s*$", mk, re.M)
    blob = open(rt.LIB_PATH, "rb").read()
    for kernel in (b"rt_query_tiled", b"rt_query_flat"):      # the launch stubs are registered by their mangled names
        assert kernel in blob
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
