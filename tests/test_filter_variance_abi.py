"""CPU: the variance-guided filter's entry points (rt_filter_variance_params_default, rt_filter_plane_variance,
rt_filter_plane_variance_device, rt_filter_plane_variance_host) are declared, exported and bound, reject bad arguments without
touching a device, and their gfx950 kernels are part of the library build."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import filter_util as fu
import filter_variance_util as fv
from uob_raytracer_amd import abi, runtime as rt

NEW = ("rt_filter_variance_params_default", "rt_filter_plane_variance", "rt_filter_plane_variance_device",
       "rt_filter_plane_variance_host")
CSRC = os.path.join(ROOT, "uob_raytracer_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "uob_rt.h")


def test_declared_exported_and_bound():
    src = open(HEADER).read()
    lib = C.CDLL(rt.LIB_PATH)
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, plain)
        assert decl
        assert hasattr(lib, name)
        assert name in rt.EXPORTS
        assert len(getattr(rt.lib(), name).argtypes) == len(decl.group(1).split(",")), name
    assert re.search(r"#define\s+RT_ABI_VERSION\s+2\b", src)
    assert rt.lib().rt_abi_version() == abi.RT_ABI_VERSION == 2
    for method in ("filter_plane_variance", "filter_plane_variance_device", "filter_variance_stats"):
        assert callable(getattr(rt.RayTracer, method))
    assert callable(rt.filter_plane_variance_host) and callable(rt.filter_variance_params)
    # the plain filter's keys stay; the variance call names slot 5
    assert rt.FILTER_STATS_KEYS[5] == "reserved5" and len(rt.FILTER_STATS_KEYS) == 8
    assert rt.FILTER_VARIANCE_STATS_KEYS == rt.FILTER_STATS_KEYS[:5] + ("variance_stopped",) + rt.FILTER_STATS_KEYS[6:]


def test_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uob_rt.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                    'sizeof(rt_filter_variance_params),offsetof(rt_filter_variance_params,base),'
                    'offsetof(rt_filter_variance_params,sigma_value),offsetof(rt_filter_variance_params,value_eps));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = abi.RtFilterVarianceParams
    assert out == [32, 0, 24, 28] == [C.sizeof(T), T.base.offset, T.sigma_value.offset, T.value_eps.offset]


def test_the_defaults():
    p = rt.filter_variance_params(320, 200)
    assert bytes(p.base) == bytes(rt.filter_params(320, 200))
    assert (p.base.width, p.base.height, p.base.passes) == (320, 200, 5)
    assert p.sigma_value == 4.0 and p.value_eps == 0.0
    q = rt.filter_variance_params(8, 4, sigma_value=2.0, value_eps=0.5, passes=3, value_max_diff=0.25)
    assert (q.sigma_value, q.value_eps, q.base.passes, q.base.value_max_diff) == (2.0, 0.5, 3, 0.25)
    with pytest.raises(TypeError):
        rt.filter_variance_params(8, 4, sigma=1.0)


def _planes(h=3, w=4):
    z = lambda *s: np.zeros(s, np.float32)
    return z(h, w), z(h, w), z(h, w, 4), z(h, w, 4), z(h, w), z(h, w)


BAD_FIELDS = [("width", 0), ("width", -3), ("height", 0), ("passes", 0), ("passes", 9), ("normal_min_dot", math.nan),
              ("plane_eps", -0.5), ("plane_eps", math.nan), ("value_max_diff", -1.0), ("value_max_diff", math.nan),
              ("value_max_diff", -math.inf), ("sigma_value", -1.0), ("sigma_value", math.nan), ("sigma_value", -math.inf),
              ("value_eps", -0.25), ("value_eps", math.nan), ("value_eps", -math.inf)]


def _entries(L, fake, p, host, dev):
    """The return codes of the three entries, and the message of each."""
    out = []
    for call in (lambda: L.rt_filter_plane_variance(fake, p, *host),
                 lambda: L.rt_filter_plane_variance_device(fake, p, *dev, None),
                 lambda: L.rt_filter_plane_variance_host(p, *host)):
        out.append((call(), L.rt_last_error()))
    return out


@pytest.mark.parametrize("field,bad", BAD_FIELDS)
def test_a_parameter_out_of_range_is_invalid_without_a_device(field, bad):
    L = rt.lib()
    host = [rt._fp(a) for a in _planes()]
    fake = C.c_void_p(16)             # never dereferenced: every case fails its argument check first
    p = rt.filter_variance_params(4, 3)
    setattr(p if field in ("sigma_value", "value_eps") else p.base, field, bad)
    for rc, msg in _entries(L, fake, C.byref(p), host, [fake] * 6):
        assert rc == abi.RT_E_INVALID
        assert field.encode() in msg


def test_infinite_stops_are_in_range():
    value, var, pos, nrm, _, _ = _planes()
    out, ovar = rt.filter_plane_variance_host(value, var, pos, nrm, sigma_value=math.inf, value_eps=math.inf)
    assert out.shape == ovar.shape == (3, 4)


def test_too_many_pixels_are_invalid():
    L = rt.lib()
    host = [rt._fp(a) for a in _planes()]
    fake = C.c_void_p(16)
    p = rt.filter_variance_params(1 << 16, (1 << 15) + 1)
    for rc, msg in _entries(L, fake, C.byref(p), host, [fake] * 6):
        assert rc == abi.RT_E_INVALID and b"width * height" in msg


def test_null_arguments_are_invalid_without_a_device():
    L = rt.lib()
    host = [rt._fp(a) for a in _planes()]
    fake = C.c_void_p(16)
    p = rt.filter_variance_params(4, 3)
    assert L.rt_filter_plane_variance(None, C.byref(p), *host) == abi.RT_E_INVALID
    assert b"ctx" in L.rt_last_error()
    assert L.rt_filter_plane_variance_device(None, C.byref(p), *[fake] * 6, None) == abi.RT_E_INVALID
    assert b"ctx" in L.rt_last_error()
    for rc, msg in _entries(L, fake, None, host, [fake] * 6):
        assert rc == abi.RT_E_INVALID and b"params" in msg
    for k in range(5):                # value, variance, position4, normal4, out_value; out_variance (5) is nullable
        args, dev = list(host), [fake] * 6
        args[k] = dev[k] = None
        for rc, msg in _entries(L, fake, C.byref(p), args, dev):
            assert rc == abi.RT_E_INVALID and b"NULL plane" in msg
    # out_variance NULL is no error: the host entry runs
    assert L.rt_filter_plane_variance_host(C.byref(p), *host[:5], None) == abi.RT_OK
    # guides the kernels could not load as float4: position4, then normal4
    for k in (2, 3):
        dev = [fake] * 6
        dev[k] = C.c_void_p(20)
        assert L.rt_filter_plane_variance_device(fake, C.byref(p), *dev, None) == abi.RT_E_INVALID
        assert b"16-byte aligned" in L.rt_last_error()
    rt.lib().rt_filter_variance_params_default(None, 4, 3)      # a no-op


def test_python_wrappers_refuse_wrong_planes():
    value, var, pos, nrm, _, _ = _planes()
    with pytest.raises(ValueError):
        rt.filter_plane_variance_host(value, var[:2], pos, nrm)
    with pytest.raises(ValueError):
        rt.filter_plane_variance_host(value, var, pos[:2], nrm)
    with pytest.raises(ValueError):
        rt.filter_plane_variance_host(value, var, pos, nrm, out_variance=np.zeros((3, 4), np.float64))
    with pytest.raises(rt.RtError) as e:
        rt.filter_plane_variance_host(value, var, pos, nrm, sigma_value=-1.0)
    assert e.value.code == abi.RT_E_INVALID


def test_variance_kernels_are_built_for_gfx950():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rt_filter_variance.hip" in srcs and "filter_variance_host.cpp" in srcs
    assert re.search(r"kernel-resource-usage -c rt_filter_variance\.hip", mk)
    blob = open(rt.LIB_PATH, "rb").read()
    spacings = [1 << i for i in range(fv.MAX_TILED_SPACING.bit_length())]
    stubs = [b"rt_filter_variance_threshold", b"rt_filter_variance_direct", b"rt_filter_variance_counters"]
    stubs += [b"rt_filter_variance_tiledILi%dEEE" % s for s in spacings]
    for inst in stubs:
        assert inst in blob             # the thresholds, the direct form, the tiled form at every spacing it serves
    assert b"rt_filter_variance_tiledILi%dEEE" % (2 * spacings[-1]) not in blob
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    # the plain filter's kernels are still there under their names
    for s in (1, 2, 4, 8, 16, 32):
        assert b"rt_filter_tiledILi%dEEE" % s in blob
    # the host statement is host code only: no kernel, no HIP call
    host = open(os.path.join(CSRC, "filter_variance_host.cpp")).read()
    assert "__global__" not in host and "hip_runtime" not in host and "rt_host.h" not in host and "hip/" not in host


def test_the_restated_thresholds_are_the_kernels():
    """tests/filter_variance_util.py restates the largest tiled spacing of the variance kernels and their row groups per grid.y;
    the tile is the plain filter's."""
    host = open(os.path.join(CSRC, "rt_host.h")).read()
    kern = open(os.path.join(CSRC, "rt_filter_variance.hip")).read()
    m = re.search(r"constexpr int kFilterVarianceMaxTiledSpacing = (\d+);", host)
    assert m and int(m.group(1)) == fv.MAX_TILED_SPACING
    m = re.search(r"constexpr int kRowGroupsY = (\d+);", kern)
    assert m and int(m.group(1)) == fv.ROW_GROUPS_Y
    assert re.search(r"constexpr int TX = kFilterTX, TY = kFilterTY;", kern)
    spacings = sorted(int(x) for x in re.findall(r"launch_tiled<(\d+)>\(", kern))
    assert spacings == [1 << i for i in range(fv.MAX_TILED_SPACING.bit_length())]
    assert "s <= kFilterVarianceMaxTiledSpacing" in kern
    fv.check_sizes()


def test_the_header_states_the_consequences_and_the_scope():
    src = " ".join(open(HEADER).read().split())
    for phrase in ("out_value has rt_filter_plane's bits", "test 5 accepts a difference of 0",
                   "returns both inputs bit for bit", "spatial variance estimate for short histories is not built",
                   "Stated, not tuned on images"):
        assert phrase in src.replace(" * ", " "), phrase
