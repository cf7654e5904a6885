"""CPU: the shade entry points (rt_shade_points, rt_shade_points_device, rt_debug_shade_stats) are declared, exported and
bound, reject bad arguments without touching a device, and their gfx950 kernels are part of the library build."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from uob_raytracer_amd import abi, runtime as rt

NEW = ("rt_shade_points", "rt_shade_points_device", "rt_debug_shade_stats")
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
    for method in ("shade_points", "shade_points_device", "shade_stats", "render_direct_light"):
        assert callable(getattr(rt.RayTracer, method))
    assert len(rt.SHADE_STATS_KEYS) == 8


def test_bad_arguments_are_invalid_without_a_device():
    L = rt.lib()
    pts = np.zeros((4, 6), np.float32)
    light = np.zeros(3, np.float32)
    out = np.zeros(4, np.float32)
    cnt = np.zeros(4, np.int32)
    seeds = np.arange(4, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    fake = C.c_void_p(16)             # never dereferenced: every case fails its argument check first
    assert L.rt_shade_points(None, rt._fp(pts), ip(seeds), 4, rt._fp(light), rt._fp(out), ip(cnt)) == abi.RT_E_INVALID
    assert b"NULL" in L.rt_last_error()
    assert L.rt_shade_points_device(None, fake, fake, 4, rt._fp(light), fake, fake, None) == abi.RT_E_INVALID
    # NULL points6 / light / out_light and npoints < 0: checked before the context is used
    assert L.rt_shade_points(fake, None, ip(seeds), 4, rt._fp(light), rt._fp(out), ip(cnt)) == abi.RT_E_INVALID
    assert L.rt_shade_points(fake, rt._fp(pts), ip(seeds), 4, None, rt._fp(out), ip(cnt)) == abi.RT_E_INVALID
    assert L.rt_shade_points(fake, rt._fp(pts), ip(seeds), 4, rt._fp(light), None, ip(cnt)) == abi.RT_E_INVALID
    assert L.rt_shade_points(fake, rt._fp(pts), None, -1, rt._fp(light), rt._fp(out), None) == abi.RT_E_INVALID
    assert b"npoints" in L.rt_last_error()
    assert L.rt_shade_points_device(fake, None, fake, 4, rt._fp(light), fake, fake, None) == abi.RT_E_INVALID
    assert L.rt_shade_points_device(fake, fake, fake, 4, None, fake, fake, None) == abi.RT_E_INVALID
    assert L.rt_shade_points_device(fake, fake, fake, 4, rt._fp(light), None, fake, None) == abi.RT_E_INVALID
    assert L.rt_shade_points_device(fake, fake, None, -5, rt._fp(light), fake, None, None) == abi.RT_E_INVALID
    # a host seed outside 0 .. 2^24 is rejected before any device work
    for bad in (-1, (1 << 24) + 1):
        s = seeds.copy()
        s[2] = bad
        assert L.rt_shade_points(fake, rt._fp(pts), ip(s), 4, rt._fp(light), rt._fp(out), ip(cnt)) == abi.RT_E_INVALID
        assert b"seeds[2]" in L.rt_last_error()
    assert abi.RT_SHADE_SEED_MAX == 1 << 24 and abi.RT_SHADE_SEED_MASK == 0xFFFFFF
    stats = (C.c_uint64 * 8)()
    assert L.rt_debug_shade_stats(None, stats) == abi.RT_E_INVALID
    assert L.rt_debug_shade_stats(fake, None) == abi.RT_E_INVALID


def test_shade_kernels_are_built_for_gfx950():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rt_shade.hip" in srcs and "rt_tiles.h" in hdrs
    assert re.search(r"^ARCH\s*\?=\s*gfx950\s*$", mk, re.M)
    blob = open(rt.LIB_PATH, "rb").read()
    for inst in (b"8rt_shadeILb0ELb0EE", b"8rt_shadeILb0ELb1EE", b"8rt_shadeILb1ELb0EE", b"8rt_shadeILb1ELb1EE"):
        assert inst in blob             # (tiled copy or not) x (several points per wave or one): the mangled launch stubs
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    # the walk is shared with the ray queries, not copied
    shade = open(os.path.join(CSRC, "rt_shade.hip")).read()
    query = open(os.path.join(CSRC, "rt_ray_query.hip")).read()
    assert "tile_walk<" in shade and "tile_walk<" in query and "tile_clear_for_bundle" not in shade
