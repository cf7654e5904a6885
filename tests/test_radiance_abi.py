"""CPU: the radiance entry points (rt_radiance_rays, rt_radiance_rays_device, rt_debug_radiance_stats) are declared, exported
and bound, reject bad arguments without touching a device, and their gfx950 kernels are part of the library build."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from uob_raytracer_amd import abi, runtime as rt

NEW = ("rt_radiance_rays", "rt_radiance_rays_device", "rt_debug_radiance_stats")
CSRC = os.path.join(ROOT, "uob_raytracer_amd", "csrc")


def test_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "uob_rt.h")).read()
    lib = C.CDLL(rt.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*rt_ctx\s*\*" % name, src)
        assert hasattr(lib, name)
        assert name in rt.EXPORTS
        assert getattr(rt.lib(), name).argtypes is not None
    assert re.search(r"#define\s+RT_ABI_VERSION\s+2\b", src)
    assert rt.lib().rt_abi_version() == abi.RT_ABI_VERSION == 2
    for method in ("radiance_rays", "radiance_rays_device", "radiance_stats", "render_panorama"):
        assert callable(getattr(rt.RayTracer, method))
    assert len(rt.RADIANCE_STATS_KEYS) == 8
    doc = rt.RayTracer.render_panorama.__doc__
    assert "phi = yaw + 2 * pi * (x + 0.5) / width - pi" in doc and "theta = pi * (y + 0.5) / height - pi / 2" in doc


def test_bad_arguments_are_invalid_without_a_device():
    L = rt.lib()
    rays = np.zeros((4, 6), np.float32)
    light = np.zeros(3, np.float32)
    out = np.full((4, 4), 7.0, np.float32)
    prim = np.full(4, 7, np.int32)
    seeds = np.arange(4, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    fake = C.c_void_p(16)             # never dereferenced: every case fails its argument check first
    assert L.rt_radiance_rays(None, rt._fp(rays), ip(seeds), 4, rt._fp(light), rt._fp(out), ip(prim)) == abi.RT_E_INVALID
    assert b"NULL" in L.rt_last_error()
    assert L.rt_radiance_rays_device(None, fake, fake, 4, rt._fp(light), fake, fake, None) == abi.RT_E_INVALID
    # NULL rays6 / light / out_rgba4 and nray < 0 or > 2^31: checked before the context is used
    assert L.rt_radiance_rays(fake, None, ip(seeds), 4, rt._fp(light), rt._fp(out), ip(prim)) == abi.RT_E_INVALID
    assert L.rt_radiance_rays(fake, rt._fp(rays), ip(seeds), 4, None, rt._fp(out), ip(prim)) == abi.RT_E_INVALID
    assert L.rt_radiance_rays(fake, rt._fp(rays), ip(seeds), 4, rt._fp(light), None, ip(prim)) == abi.RT_E_INVALID
    assert L.rt_radiance_rays(fake, rt._fp(rays), None, -1, rt._fp(light), rt._fp(out), None) == abi.RT_E_INVALID
    assert b"nray" in L.rt_last_error()
    assert L.rt_radiance_rays(fake, rt._fp(rays), None, (1 << 31) + 1, rt._fp(light), rt._fp(out), None) == abi.RT_E_INVALID
    assert L.rt_radiance_rays_device(fake, None, fake, 4, rt._fp(light), fake, fake, None) == abi.RT_E_INVALID
    assert L.rt_radiance_rays_device(fake, fake, fake, 4, None, fake, fake, None) == abi.RT_E_INVALID
    assert L.rt_radiance_rays_device(fake, fake, fake, 4, rt._fp(light), None, fake, None) == abi.RT_E_INVALID
    assert L.rt_radiance_rays_device(fake, fake, None, -5, rt._fp(light), fake, None, None) == abi.RT_E_INVALID
    assert L.rt_radiance_rays_device(fake, fake, None, (1 << 31) + 1, rt._fp(light), fake, None, None) == abi.RT_E_INVALID
    # a host seed outside 0 .. 2^24 is rejected before any device work
    for bad in (-1, (1 << 24) + 1):
        s = seeds.copy()
        s[2] = bad
        assert L.rt_radiance_rays(fake, rt._fp(rays), ip(s), 4, rt._fp(light), rt._fp(out), ip(prim)) == abi.RT_E_INVALID
        assert b"seeds[2]" in L.rt_last_error()
    assert (out == 7.0).all() and (prim == 7).all()              # nothing was written
    stats = (C.c_uint64 * 8)()
    assert L.rt_debug_radiance_stats(None, stats) == abi.RT_E_INVALID
    assert L.rt_debug_radiance_stats(fake, None) == abi.RT_E_INVALID


def test_radiance_kernels_are_built_for_gfx950():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rt_radiance.hip" in srcs and "rt_shade_body.h" in hdrs
    blob = open(rt.LIB_PATH, "rb").read()
    for inst in (b"17rt_radiance_traceILb0EE", b"17rt_radiance_traceILb1EE", b"17rt_radiance_shadeILb0ELb0EE",
                 b"17rt_radiance_shadeILb0ELb1EE", b"17rt_radiance_shadeILb1ELb0EE", b"17rt_radiance_shadeILb1ELb1EE"):
        assert inst in blob             # (tiled copy or not) x (several records per wave or one): the mangled launch stubs
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    # the walk and the per-group shade body are shared, not copied
    rad = open(os.path.join(CSRC, "rt_radiance.hip")).read()
    shade = open(os.path.join(CSRC, "rt_shade.hip")).read()
    body = open(os.path.join(CSRC, "rt_shade_body.h")).read()
    assert "tile_walk<false" in rad and "shade_groups<" in rad and "shade_groups<" in shade
    assert "tile_walk<true" in body and "tile_walk<true, BOXES>" not in rad and "tile_clear_for_bundle" not in rad
