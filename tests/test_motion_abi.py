"""The motion entry points (rt_motion_snapshot, rt_motion_release, rt_debug_motion_info, rt_motion_planes*,
rt_debug_motion_stats, rt_accumulate_plane_moving*) are declared, exported and bound, refuse bad arguments without touching a
device, and their gfx950 kernel is part of the library build.  One case needs a context, so a device: a context without a
snapshot refuses motion calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from uob_raytracer_amd import abi, runtime as rt

NEW = ("rt_motion_snapshot", "rt_motion_release", "rt_debug_motion_info", "rt_motion_planes", "rt_motion_planes_device",
       "rt_motion_planes_host", "rt_debug_motion_stats", "rt_accumulate_plane_moving", "rt_accumulate_plane_moving_device",
       "rt_accumulate_plane_moving_host")
CSRC = os.path.join(ROOT, "uob_raytracer_amd", "csrc")
F32 = np.float32


def test_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "uob_rt.h")).read()
    lib = C.CDLL(rt.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src)
        assert hasattr(lib, name)
        assert name in rt.EXPORTS
        assert getattr(rt.lib(), name).argtypes is not None
    assert re.search(r"#define\s+RT_ABI_VERSION\s+2\b", src)
    for method in ("motion_snapshot", "motion_release", "motion_info", "motion_planes", "motion_planes_device", "motion_stats"):
        assert callable(getattr(rt.RayTracer, method))
    assert callable(rt.motion_planes_host) and len(rt.MOTION_STATS_KEYS) == 8
    # the argument counts of the bindings are the header's
    flat = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, flat).group(1)
        assert len(getattr(rt.lib(), name).argtypes) == len(decl.split(",")), name


def test_motion_kernel_is_built_for_gfx950():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rt_motion.hip" in srcs and "motion_host.cpp" in srcs
    assert re.search(r"kernel-resource-usage -c rt_motion\.hip", mk)
    blob = open(rt.LIB_PATH, "rb").read()
    for stub in (b"rt_motion_elements", b"rt_motion_counters"):
        assert stub in blob
    host = open(os.path.join(CSRC, "motion_host.cpp")).read()
    assert "__global__" not in host and "hip_runtime" not in host and "rt_host.h" not in host


def _motion_planes(k=6):
    return [np.zeros(k, np.int32), np.zeros((k, 4), F32), np.zeros((k, 4), F32), np.zeros((k, 4), F32), np.zeros((k, 4), F32)]


def test_motion_null_and_range_refusals_without_a_device():
    L = rt.lib()
    prim, pos, nrm, op, on = _motion_planes()
    host = [rt._ip(prim), rt._fp(pos), rt._fp(nrm), 6, rt._fp(op), rt._fp(on)]
    fake = C.c_void_p(16)             # never dereferenced: every case fails its argument check first
    dev = [fake, fake, fake, 6, fake, fake]
    scene = [rt._fp(np.zeros((3, 4), F32)), rt._fp(np.zeros((3, 4), F32)), rt._fp(np.zeros((1, 4), F32)), 1]
    assert L.rt_motion_planes(None, *host) == abi.RT_E_INVALID and b"ctx" in L.rt_last_error()
    assert L.rt_motion_planes_device(None, *dev, None) == abi.RT_E_INVALID and b"ctx" in L.rt_last_error()
    assert L.rt_motion_snapshot(None, None) == abi.RT_E_INVALID and b"ctx" in L.rt_last_error()
    assert L.rt_motion_release(None) == abi.RT_E_INVALID and b"ctx" in L.rt_last_error()
    assert L.rt_debug_motion_info(None, C.byref(C.c_int32())) == abi.RT_E_INVALID
    assert L.rt_debug_motion_info(fake, None) == abi.RT_E_INVALID
    stats = (C.c_uint64 * 8)()
    assert L.rt_debug_motion_stats(None, stats) == abi.RT_E_INVALID and L.rt_debug_motion_stats(fake, None) == abi.RT_E_INVALID
    for k in (0, 1, 2, 4, 5):         # every plane is required
        args = list(host)
        args[k] = None
        assert L.rt_motion_planes(fake, *args) == abi.RT_E_INVALID and b"NULL plane" in L.rt_last_error()
        assert L.rt_motion_planes_host(*scene, *args) == abi.RT_E_INVALID and b"NULL plane" in L.rt_last_error()
        d = list(dev)
        d[k] = None
        assert L.rt_motion_planes_device(fake, *d, None) == abi.RT_E_INVALID and b"NULL plane" in L.rt_last_error()
    for bad in (-1, (1 << 31) + 1):
        args, d = list(host), list(dev)
        args[3] = d[3] = bad
        for rc in (L.rt_motion_planes(fake, *args), L.rt_motion_planes_device(fake, *d, None), L.rt_motion_planes_host(*scene, *args)):
            assert rc == abi.RT_E_INVALID and b"count" in L.rt_last_error() and b"2^31" in L.rt_last_error()
    for k, name in ((1, b"d_position4"), (2, b"d_normal4"), (4, b"d_out_prev_position4"), (5, b"d_out_prev_normal4")):
        d = list(dev)
        d[k] = C.c_void_p(52)
        assert L.rt_motion_planes_device(fake, *d, None) == abi.RT_E_INVALID
        assert b"16-byte aligned" in L.rt_last_error() and name in L.rt_last_error()
    # the host statement's scene
    assert L.rt_motion_planes_host(scene[0], scene[1], scene[2], -1, *host) == abi.RT_E_INVALID and b"n = -1" in L.rt_last_error()
    assert L.rt_motion_planes_host(None, scene[1], scene[2], 1, *host) == abi.RT_E_INVALID and b"NULL scene" in L.rt_last_error()
    assert L.rt_motion_planes_host(None, None, None, 0, *host) == abi.RT_OK            # no triangles: every prim >= 0 is out of range
    assert not op.any() and not on.any()
    args = list(host)
    args[3] = 0
    assert L.rt_motion_planes_host(*scene, *args) == abi.RT_OK                           # count == 0: a no-op


def test_one_reprojection_plane_without_the_other_is_invalid_without_a_device():
    L = rt.lib()
    h, w = 3, 4
    v, pos, nrm, rp, rn = (np.zeros((h, w), F32), np.zeros((h, w, 4), F32), np.zeros((h, w, 4), F32), np.zeros((h, w, 4), F32),
                           np.zeros((h, w, 4), F32))
    prim, prev, nxt = np.zeros((h, w), np.int32), np.zeros((h, w, 12), F32), np.zeros((h, w, 12), F32)
    mean, var = np.zeros((h, w), F32), np.zeros((h, w), F32)
    p = rt.accumulate_params(w, h)
    fake, other = C.c_void_p(16), C.c_void_p(32)
    for a, b in ((rt._fp(rp), None), (None, rt._fp(rn))):
        host = [rt._fp(v), rt._fp(pos), rt._fp(nrm), rt._ip(prim), a, b, rt._fp(prev), rt._fp(nxt), rt._fp(mean), rt._fp(var)]
        for rc in (L.rt_accumulate_plane_moving(fake, C.byref(p), *host), L.rt_accumulate_plane_moving_host(C.byref(p), *host)):
            assert rc == abi.RT_E_INVALID
            assert b"reproj_position4" in L.rt_last_error() and b"both" in L.rt_last_error()
    for a, b in ((fake, None), (None, fake)):
        rc = L.rt_accumulate_plane_moving_device(fake, C.byref(p), fake, fake, fake, fake, a, b, fake, other, fake, fake, None)
        assert rc == abi.RT_E_INVALID and b"both" in L.rt_last_error()
    for a, b, name in ((C.c_void_p(52), fake, b"d_reproj_position4"), (fake, C.c_void_p(56), b"d_reproj_normal4")):
        rc = L.rt_accumulate_plane_moving_device(fake, C.byref(p), fake, fake, fake, fake, a, b, fake, other, fake, fake, None)
        assert rc == abi.RT_E_INVALID and b"16-byte aligned" in L.rt_last_error() and name in L.rt_last_error()
    # the accumulate family's own checks come first, under the moving entry's name
    assert L.rt_accumulate_plane_moving(None, C.byref(p), *host) == abi.RT_E_INVALID and b"ctx" in L.rt_last_error()
    assert L.rt_accumulate_plane_moving_host(None, *host) == abi.RT_E_INVALID and b"rt_accumulate_plane_moving_host: params" in L.rt_last_error()
    p.max_history = 0
    host[4], host[5] = rt._fp(rp), rt._fp(rn)
    assert L.rt_accumulate_plane_moving_host(C.byref(p), *host) == abi.RT_E_INVALID and b"max_history" in L.rt_last_error()
    with pytest.raises(ValueError):
        rt.accumulate_plane_host(v, pos, nrm, reproj_position4=rp[:2], reproj_normal4=rn)
    with pytest.raises(ValueError):
        rt.motion_planes_host(np.zeros((3, 4), F32), np.zeros((6, 4), F32), np.zeros((1, 4), F32), prim, pos, nrm)


@pytest.mark.gpu
def test_a_context_without_a_snapshot_refuses_motion_calls(scene):
    import torch
    tr = rt.RayTracer(abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=2), scene)
    try:
        assert tr.motion_info() == 0 and tr.motion_stats()["elements"] == 0
        prim, pos, nrm, _, _ = _motion_planes()
        with pytest.raises(rt.RtError) as e:
            tr.motion_planes(prim, pos, nrm)
        assert e.value.code == abi.RT_E_INVALID and "no snapshot" in str(e.value)
        d = [torch.from_numpy(a).cuda() for a in (prim, pos, nrm)]
        with pytest.raises(rt.RtError) as e:
            tr.motion_planes_device(*d)
        assert e.value.code == abi.RT_E_INVALID and "no snapshot" in str(e.value)
        tr.motion_release()                                   # nothing to free: a no-op
        assert tr.motion_info() == 0
    finally:
        tr.close()
