"""CPU: the rigid-object entry points (rt_scene_transform, rt_set_objects, rt_pose_objects, rt_pose_objects_device,
rt_debug_object_count) are declared with the documented signatures, exported and bound; rt_scene_transform is the arithmetic
of Scene.transformed as it was before it called rt_scene_transform (a numpy FP32 expression + rt_triangle_compute_normal per
triangle, restated here), bit for bit; bad arguments are RT_E_INVALID before any device work (no device is present here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from uob_raytracer_amd import abi, runtime as rt

SIGNATURES = {
    "rt_scene_transform": r"void rt_scene_transform\(rt_triangle\* \w+, int32_t \w+, int32_t \w+, int32_t \w+, "
                          r"const float \w+\[12\]\);",
    "rt_set_objects": r"int rt_set_objects\(rt_ctx\* \w+, const int32_t\* \w+, const int32_t\* \w+, int32_t \w+\);",
    "rt_pose_objects": r"int rt_pose_objects\(rt_ctx\* \w+, const float\* \w+, uint32_t \w+\);",
    "rt_pose_objects_device": r"int rt_pose_objects_device\(rt_ctx\* \w+, const void\* \w+, uint32_t \w+, void\* \w+\);",
    "rt_debug_object_count": r"int rt_debug_object_count\(rt_ctx\* \w+, int32_t\* \w+\);",
}


def test_declared_exported_and_bound():
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "uob_rt.h")).read())
    lib = C.CDLL(rt.LIB_PATH)
    for name, sig in SIGNATURES.items():
        assert re.search(sig, src), name
        assert hasattr(lib, name)
        assert name in rt.EXPORTS
        assert getattr(rt.lib(), name).argtypes is not None
    assert rt.lib().rt_abi_version() == abi.RT_ABI_VERSION == 2          # additions only
    for method in ("set_objects", "pose_objects", "pose_objects_device", "object_count"):
        assert callable(getattr(rt.RayTracer, method))
    assert callable(rt.Scene.posed)


def transformed_reference(scene, indices, matrix, offset=(0.0, 0.0, 0.0)):
    """Scene.transformed as it stood before rt_scene_transform existed: matrix @ v + offset in numpy float32, the products
    summed left to right, and one rt_triangle_compute_normal per triangle."""
    m = np.asarray(matrix, np.float32).reshape(3, 3)
    o = np.asarray(offset, np.float32).reshape(3)
    aos = scene.aos.copy()
    idx = np.arange(len(scene))[indices] if not isinstance(indices, (list, tuple)) else np.asarray(indices, np.int64)
    v = aos[idx, 0:3, 0:3]
    aos[idx, 0:3, 0:3] = ((v[..., 0:1] * m[:, 0] + v[..., 1:2] * m[:, 1]) + v[..., 2:3] * m[:, 2]) + o
    tris = (abi.RtTriangle * len(scene)).from_buffer(aos)
    for i in idx:
        rt.lib().rt_triangle_compute_normal(C.byref(tris[int(i)]))
    return rt.Scene(aos)


def _transform(scene, first, count, matrix, offset):
    xf = np.zeros((3, 4), np.float32)
    xf[:, :3], xf[:, 3] = matrix, offset
    aos = scene.aos.copy()
    rt.lib().rt_scene_transform(aos.ctypes.data_as(C.POINTER(abi.RtTriangle)), len(scene), first, count, rt._fp(xf))
    return rt.Scene(aos)


def _same_bits(a, b):
    return np.array_equal(a.aos.view(np.uint32), b.aos.view(np.uint32))


def _rot_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


MATRICES = {"rotation": _rot_y(0.3) @ np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]]),
            "mirror": np.diag([1.0, -1.0, 1.0]), "squash": np.diag([1.0, 0.5, 1.0]), "identity": np.eye(3)}


@pytest.fixture(scope="module")
def mesh():
    """The Cornell Box + the small golden mesh: irregular triangles, none axis-aligned."""
    return rt.Scene.cornell_box() + rt.Scene.load_obj(os.path.join(ROOT, "tests", "golden", "mesh_small.obj"))


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_scene_transform_is_transformed(name, mesh):
    n = len(mesh)
    offset = (0.0, 0.0, 0.0) if name == "identity" else (0.125, -0.3, 0.07)
    for first, count in ((26, n - 26), (0, n), (n - 1, 1)):                 # the mesh, everything, the last triangle only
        want = transformed_reference(mesh, slice(first, first + count), MATRICES[name], offset)
        got = _transform(mesh, first, count, MATRICES[name], offset)
        assert _same_bits(got, want), (name, first, count)
        assert _same_bits(mesh.transformed(slice(first, first + count), MATRICES[name], offset), want)
        keep = np.r_[0:first, first + count:n]                # triangles outside the range: untouched
        assert np.array_equal(got.aos[keep].view(np.uint32), mesh.aos[keep].view(np.uint32))
    if name != "identity":
        assert not _same_bits(got, mesh)
    # index lists (the existing callers' form) go through the one call too
    idx = [3, 40, 41, n - 1]
    assert _same_bits(mesh.transformed(idx, MATRICES[name], offset), transformed_reference(mesh, idx, MATRICES[name], offset))


def test_degenerate_triangle_keeps_the_nan_bits(mesh):
    aos = mesh.aos.copy()
    aos[30, 1] = aos[30, 0]                                    # two equal corners: the cross product is zero
    aos[31, 0:3, 0:3] = 0.0                                    # all corners at the origin
    aos[32, 0:3, 0:3] = [[0, 0, 0], [1e-20, 0, 0], [0, 1e-20, 0]]      # a denormal cross product whose square is zero
    aos[33, 0:3, 0:3] = [[0, 0, 0], [3e-11, 0, 0], [0, 3e-11, 0]]      # a denormal squared length
    bad = rt.Scene(aos)
    want = transformed_reference(bad, slice(26, 40), MATRICES["rotation"])
    got = _transform(bad, 26, 14, MATRICES["rotation"], (0.0, 0.0, 0.0))
    assert np.isnan(want.aos[30, 3, :3]).all() and np.isnan(want.aos[31, 3, :3]).all()
    assert not np.isfinite(want.aos[32, 3, :3]).all() and np.isfinite(want.aos[33, 3, :3]).all()
    assert _same_bits(got, want)                               # NaN payloads and signs included


def test_posed_is_chained_transformed(mesh):
    n = len(mesh)
    ranges = [(10, 8), slice(26, n)]
    xf = np.zeros((2, 3, 4), np.float32)
    xf[0, :, :3], xf[0, :, 3] = MATRICES["squash"], (0.25, 0.0, -0.125)
    xf[1, :, :3], xf[1, :, 3] = MATRICES["rotation"], (0.0, -0.1, 0.2)
    want = mesh.transformed(slice(10, 18), xf[0, :, :3], xf[0, :, 3]).transformed(slice(26, n), xf[1, :, :3], xf[1, :, 3])
    assert _same_bits(mesh.posed(ranges, xf), want)
    assert _same_bits(mesh.posed([], np.zeros((0, 3, 4), np.float32)), mesh)


def test_scene_transform_ignores_a_range_outside_the_scene(mesh):
    xf = np.zeros((3, 4), np.float32)
    for first, count in ((-1, 2), (len(mesh), 1), (5, len(mesh)), (3, -1)):
        aos = mesh.aos.copy()
        rt.lib().rt_scene_transform(aos.ctypes.data_as(C.POINTER(abi.RtTriangle)), len(mesh), first, count, rt._fp(xf))
        assert np.array_equal(aos.view(np.uint32), mesh.aos.view(np.uint32))


def _invalid(rc, *words):
    assert rc == abi.RT_E_INVALID
    msg = rt.lib().rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_null_context_is_invalid():
    L = rt.lib()
    one = (C.c_int32 * 1)(0)
    xf = np.zeros(12, np.float32)
    _invalid(L.rt_set_objects(None, one, one, 1), "NULL")
    _invalid(L.rt_pose_objects(None, rt._fp(xf), 0), "NULL")
    _invalid(L.rt_pose_objects_device(None, C.c_void_p(16), 0, None), "NULL")
    _invalid(L.rt_debug_object_count(None, C.byref(C.c_int32())), "NULL")


def test_bad_arguments_are_invalid_before_any_device_work():
    """With a context handle that is never dereferenced for device work (a zeroed block of host memory, large enough for any
    rt_ctx: a context of 0 triangles and no object table as far as the checks look)."""
    L = rt.lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    one, zero = (C.c_int32 * 1)(1), (C.c_int32 * 1)(0)
    xf = np.zeros(12, np.float32)
    _invalid(L.rt_set_objects(h, zero, one, -1), "nobj")
    _invalid(L.rt_set_objects(h, zero, one, 65536), "nobj")
    _invalid(L.rt_set_objects(h, None, one, 1), "NULL")
    _invalid(L.rt_set_objects(h, zero, None, 1), "NULL")
    _invalid(L.rt_set_objects(h, zero, one, 1), "object 0")             # no triangle 0 in a context of none
    _invalid(L.rt_set_objects(h, zero, zero, 1), "object 0")            # an empty range
    assert L.rt_set_objects(h, None, None, 0) == abi.RT_OK              # dropping a table that does not exist: nothing to do
    count = C.c_int32(-1)
    assert L.rt_debug_object_count(h, C.byref(count)) == abi.RT_OK and count.value == 0
    _invalid(L.rt_debug_object_count(h, None), "NULL")
    _invalid(L.rt_pose_objects(h, None, 0), "NULL")
    _invalid(L.rt_pose_objects_device(h, None, 0, None), "NULL")
    _invalid(L.rt_pose_objects(h, rt._fp(xf), 4), "flags")
    _invalid(L.rt_pose_objects_device(h, C.c_void_p(16), 0x80000000, None), "flags")
    _invalid(L.rt_pose_objects(h, rt._fp(xf), abi.RT_UPDATE_REORDER | abi.RT_UPDATE_DEVICE_TILES), "exclude")
    _invalid(L.rt_pose_objects(h, rt._fp(xf), 0), "no object table")
    _invalid(L.rt_pose_objects_device(h, C.c_void_p(16), abi.RT_UPDATE_DEVICE_TILES, None), "no object table")
