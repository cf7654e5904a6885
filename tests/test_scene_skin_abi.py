"""CPU: the skin entry points (rt_scene_skin, rt_set_skin, rt_pose_skin, rt_pose_skin_device, rt_debug_skin_info) are declared
with the documented signatures, exported and bound; rt_scene_skin is a numpy float32 restatement of include/uob_rt.h "skinned
meshes" (every product and every sum one numpy operation, in the documented order, + rt_triangle_compute_normal per triangle),
bit for bit; bad arguments are RT_E_INVALID before any device work (no device is present here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_scene_pose_abi import MATRICES
from uob_raytracer_amd import abi, runtime as rt

SIGNATURES = {
    "rt_scene_skin": r"void rt_scene_skin\(rt_triangle\* \w+, int32_t \w+, int32_t \w+, int32_t \w+, const uint16_t\* \w+, "
                     r"const float\* \w+, const float\* \w+, int32_t \w+\);",
    "rt_set_skin": r"int rt_set_skin\(rt_ctx\* \w+, int32_t \w+, int32_t \w+, const uint16_t\* \w+, const float\* \w+, "
                   r"int32_t \w+\);",
    "rt_pose_skin": r"int rt_pose_skin\(rt_ctx\* \w+, const float\* \w+, uint32_t \w+\);",
    "rt_pose_skin_device": r"int rt_pose_skin_device\(rt_ctx\* \w+, const void\* \w+, uint32_t \w+, void\* \w+\);",
    "rt_debug_skin_info": r"int rt_debug_skin_info\(rt_ctx\* \w+, int32_t\* \w+, int32_t\* \w+, int32_t\* \w+\);",
}
F32 = np.float32


def test_declared_exported_and_bound():
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "uob_rt.h")).read())
    lib = C.CDLL(rt.LIB_PATH)
    for name, sig in SIGNATURES.items():
        assert re.search(sig, src), name
        assert hasattr(lib, name)
        assert name in rt.EXPORTS
        assert getattr(rt.lib(), name).argtypes is not None
    assert rt.lib().rt_abi_version() == abi.RT_ABI_VERSION == 2          # additions only
    for method in ("set_skin", "pose_skin", "pose_skin_device", "skin_info"):
        assert callable(getattr(rt.RayTracer, method))
    assert callable(rt.Scene.skinned)


def skinned_reference(scene, first, count, index, weights, bones):
    """include/uob_rt.h "skinned meshes" in numpy float32, one operation per product and per sum:
    p_k = ((v.x*m_r0 + v.y*m_r1) + v.z*m_r2) + t_r for the four bones of a corner, then
    v' = ((w_0*p_0 + w_1*p_1) + w_2*p_2) + w_3*p_3, then rt_triangle_compute_normal per triangle of the range."""
    b = np.asarray(bones, F32).reshape(-1, 3, 4)
    idx = np.asarray(index).reshape(3 * count, 4)
    w = np.asarray(weights, F32).reshape(3 * count, 4)
    aos = scene.aos.copy()
    v = aos[first:first + count, 0:3, 0:3].reshape(3 * count, 3).copy()
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]                  # [corners, 1]
    p = []
    for k in range(4):
        m = b[idx[:, k]]                                       # [corners, 3 rows, 4]
        p.append(((x * m[:, :, 0] + y * m[:, :, 1]) + z * m[:, :, 2]) + m[:, :, 3])
    out = ((w[:, 0:1] * p[0] + w[:, 1:2] * p[1]) + w[:, 2:3] * p[2]) + w[:, 3:4] * p[3]
    assert out.dtype == F32
    aos[first:first + count, 0:3, 0:3] = out.reshape(count, 3, 3)
    tris = (abi.RtTriangle * len(scene)).from_buffer(aos)
    for i in range(first, first + count):
        rt.lib().rt_triangle_compute_normal(C.byref(tris[i]))
    return rt.Scene(aos)


def _same_bits(a, b):
    return np.array_equal(a.aos.view(np.uint32), b.aos.view(np.uint32))


def _bones(names, offsets):
    xf = np.zeros((len(names), 3, 4), F32)
    for k, (name, off) in enumerate(zip(names, offsets)):
        xf[k, :, :3], xf[k, :, 3] = MATRICES[name], off
    return xf


BONES = _bones(["rotation", "mirror", "squash", "identity"],
               [(0.125, -0.3, 0.07), (0.0, 0.1, 0.0), (-0.05, 0.0, 0.2), (0.0, 0.0, 0.0)])


def _table(count, kind, nbones=4, seed=3):
    """[3*count,4] indices and weights: "one" influence (weight 1 in a random slot), "two" (a random split over two slots),
    "four" non-zero weights that sum to 1 up to rounding."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, nbones, (3 * count, 4)).astype(np.uint16)
    w = np.zeros((3 * count, 4), F32)
    rows = np.arange(3 * count)
    if kind == "one":
        w[rows, rng.integers(0, 4, 3 * count)] = 1.0
    elif kind == "two":
        a = rng.integers(0, 4, 3 * count)
        b = (a + rng.integers(1, 4, 3 * count)) % 4
        t = rng.uniform(0.05, 0.95, 3 * count).astype(F32)
        w[rows, a], w[rows, b] = t, F32(1.0) - t
    else:
        r = rng.uniform(0.1, 1.0, (3 * count, 4))
        w[:] = (r / r.sum(axis=1, keepdims=True)).astype(F32)
        assert (w > 0).all()
    return idx, w


@pytest.fixture(scope="module")
def mesh():
    """The Cornell Box + the small golden mesh: irregular triangles, none axis-aligned."""
    return rt.Scene.cornell_box() + rt.Scene.load_obj(os.path.join(ROOT, "tests", "golden", "mesh_small.obj"))


@pytest.mark.parametrize("kind", ["one", "two", "four"])
def test_scene_skin_is_the_restatement(kind, mesh):
    n = len(mesh)
    for first, count in ((26, n - 26), (0, n), (n - 1, 1)):                 # the mesh, everything, the last triangle only
        idx, w = _table(count, kind)
        assert all((idx == k).any() for k in range(4))                      # rotation, mirror, squash and identity all used
        want = skinned_reference(mesh, first, count, idx, w, BONES)
        got = mesh.skinned(first, count, idx, w, BONES)
        assert _same_bits(got, want), (kind, first, count)
        keep = np.r_[0:first, first + count:n]                              # triangles outside the range: untouched
        assert np.array_equal(got.aos[keep].view(np.uint32), mesh.aos[keep].view(np.uint32))
        assert np.array_equal(got.aos[:, 4].view(np.uint32), mesh.aos[:, 4].view(np.uint32))        # the colours
        assert np.array_equal(got.aos[:, :3, 3].view(np.uint32), mesh.aos[:, :3, 3].view(np.uint32))  # w of the vertices
        assert not _same_bits(got, mesh)


def test_weights_are_not_normalised(mesh):
    count = len(mesh) - 26
    idx = np.zeros((3 * count, 4), np.uint16)
    w = np.zeros((3 * count, 4), F32)
    w[:, 0] = 0.5                                                           # half an identity: toward the origin
    ident = _bones(["identity"], [(0.0, 0.0, 0.0)])
    got = mesh.skinned(26, count, idx, w, ident)
    assert _same_bits(got, skinned_reference(mesh, 26, count, idx, w, ident))
    assert np.array_equal(got.aos[26:, :3, :3], mesh.aos[26:, :3, :3] * F32(0.5))


def test_every_influence_is_evaluated(mesh):
    """0 * inf is a NaN: a bone of weight 0 still counts."""
    idx = np.array([[0, 1, 0, 0]] * 3, np.uint16)
    w = np.array([[1.0, 0.0, 0.0, 0.0]] * 3, F32)
    bones = _bones(["identity", "identity"], [(0.0, 0.0, 0.0), (np.inf, 0.0, 0.0)])
    got = mesh.skinned(30, 1, idx, w, bones)
    assert np.isnan(got.aos[30, :3, 0]).all() and np.isfinite(got.aos[30, :3, 1:3]).all()
    assert _same_bits(got, skinned_reference(mesh, 30, 1, idx, w, bones))


def test_degenerate_triangle_keeps_the_nan_bits(mesh):
    first, count = 26, 14
    idx, w = _table(count, "two")
    # triangle 30: corners 0 and 1 blended onto one point — the same rest point, the same influences
    aos = mesh.aos.copy()
    aos[30, 1] = aos[30, 0]
    k = 3 * (30 - first)
    idx[k + 1], w[k + 1] = idx[k], w[k]
    # triangle 31: every corner blended onto the origin by weights of zero
    w[3 * (31 - first):3 * (31 - first) + 3] = 0.0
    bad = rt.Scene(aos)
    want = skinned_reference(bad, first, count, idx, w, BONES)
    got = bad.skinned(first, count, idx, w, BONES)
    assert np.isnan(want.aos[30, 3, :3]).all() and np.isnan(want.aos[31, 3, :3]).all()
    assert np.array_equal(want.aos[30, 0, :3], want.aos[30, 1, :3]) and (want.aos[31, :3, :3] == 0).all()
    assert _same_bits(got, want)                               # NaN payloads and signs included


def test_one_influence_per_object_is_posed():
    """Weights (1, 0, 0, 0) everywhere and one bone per object give Scene.posed as float values (the blend's + 0 * p turns a
    -0 into +0, so not as bits).  On the box's two blocks: the golden mesh has degenerate triangles, whose normals are NaN."""
    box = rt.Scene.cornell_box()
    ranges = [(10, 8), (18, 4), (22, 4)]
    xf = BONES[:3]
    first, count = 10, 16
    idx = np.zeros((3 * count, 4), np.uint16)
    for k, (f, cnt) in enumerate(ranges):
        idx[3 * (f - first):3 * (f - first + cnt), 0] = k
    idx[:, 1:] = np.random.default_rng(4).integers(0, 3, (3 * count, 3))     # whichever bones at weight 0
    w = np.zeros((3 * count, 4), F32)
    w[:, 0] = 1.0
    got, want = box.skinned(first, count, idx, w, xf), box.posed(ranges, xf)
    assert not np.isnan(want.aos).any() and not _same_bits(want, box)
    assert got.aos.dtype == want.aos.dtype == F32 and np.array_equal(got.aos, want.aos)


def test_scene_skin_ignores_a_bad_range_and_a_bad_index(mesh):
    n = len(mesh)
    L = rt.lib()
    u16 = C.POINTER(C.c_uint16)

    def call(first, count, idx, w, nbones):
        aos = mesh.aos.copy()
        L.rt_scene_skin(aos.ctypes.data_as(C.POINTER(abi.RtTriangle)), n, first, count, idx.ctypes.data_as(u16), rt._fp(w),
                        rt._fp(BONES), nbones)
        return aos

    idx, w = _table(n, "four")
    for first, count in ((-1, 2), (n, 1), (5, n), (3, -1)):
        assert np.array_equal(call(first, count, idx, w, 4).view(np.uint32), mesh.aos.view(np.uint32))
    assert not np.array_equal(call(0, n, idx, w, 4).view(np.uint32), mesh.aos.view(np.uint32))
    bad = idx.copy()
    bad[-1, 3] = 4                                             # the very last entry of the table
    assert np.array_equal(call(0, n, bad, w, 4).view(np.uint32), mesh.aos.view(np.uint32))
    assert np.array_equal(call(0, n, idx, w, 3).view(np.uint32), mesh.aos.view(np.uint32))    # nbones below an index in use


def _invalid(rc, *words):
    assert rc == abi.RT_E_INVALID
    msg = rt.lib().rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def _u16(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


def test_null_context_is_invalid():
    L = rt.lib()
    idx, w = np.zeros((3, 4), np.uint16), np.zeros((3, 4), F32)
    out = [C.c_int32() for _ in range(3)]
    _invalid(L.rt_set_skin(None, 0, 1, _u16(idx), rt._fp(w), 1), "NULL")
    _invalid(L.rt_set_skin(None, 0, 0, None, None, 1), "NULL")
    _invalid(L.rt_pose_skin(None, rt._fp(np.zeros(12, F32)), 0), "NULL")
    _invalid(L.rt_pose_skin_device(None, C.c_void_p(16), 0, None), "NULL")
    _invalid(L.rt_debug_skin_info(None, *[C.byref(x) for x in out]), "NULL")


def test_bad_arguments_are_invalid_before_any_device_work():
    """With a context handle that is never dereferenced for device work (a zeroed block of host memory, large enough for any
    rt_ctx: a context of 0 triangles and no skin as far as the checks look)."""
    L = rt.lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    idx, w = np.zeros((6, 4), np.uint16), np.zeros((6, 4), F32)
    w[:, 0] = 1.0
    xf = np.zeros(12, F32)
    _invalid(L.rt_set_skin(h, 0, 2, None, rt._fp(w), 1), "NULL")
    _invalid(L.rt_set_skin(h, 0, 2, _u16(idx), None, 1), "NULL")
    _invalid(L.rt_set_skin(h, 0, 2, _u16(idx), rt._fp(w), 0), "nbones")
    _invalid(L.rt_set_skin(h, 0, 2, _u16(idx), rt._fp(w), 65536), "nbones")
    _invalid(L.rt_set_skin(h, 0, -1, _u16(idx), rt._fp(w), 1), "range")       # an empty range
    _invalid(L.rt_set_skin(h, -1, 2, _u16(idx), rt._fp(w), 1), "range")       # outside
    _invalid(L.rt_set_skin(h, 0, 2, _u16(idx), rt._fp(w), 1), "range", "0 triangles")    # no triangle 0 in a context of none
    bad = idx.copy()
    bad[5, 3] = 7                                                            # the last entry of the table
    _invalid(L.rt_set_skin(h, 0, 2, _u16(bad), rt._fp(w), 7), "corner 5", "index")
    assert L.rt_set_skin(h, 0, 2, _u16(bad), rt._fp(w), 8) == abi.RT_E_INVALID and "range" in L.rt_last_error().decode()
    for value in (np.nan, -0.25, 1.5, np.inf):
        bad = w.copy()
        bad[4, 2] = value
        _invalid(L.rt_set_skin(h, 0, 2, _u16(idx), rt._fp(bad), 1), "corner 4", "weight")
    out = [C.c_int32(-1) for _ in range(3)]
    assert L.rt_debug_skin_info(h, *[C.byref(x) for x in out]) == abi.RT_OK and [x.value for x in out] == [0, 0, 0]
    _invalid(L.rt_debug_skin_info(h, None, C.byref(out[1]), C.byref(out[2])), "NULL")
    assert L.rt_set_skin(h, 0, 0, None, None, 0) == abi.RT_OK                # dropping a skin that does not exist: nothing to do
    _invalid(L.rt_pose_skin(h, None, 0), "NULL")
    _invalid(L.rt_pose_skin_device(h, None, 0, None), "NULL")
    _invalid(L.rt_pose_skin(h, rt._fp(xf), 4), "flags")
    _invalid(L.rt_pose_skin_device(h, C.c_void_p(16), 0x80000000, None), "flags")
    _invalid(L.rt_pose_skin(h, rt._fp(xf), abi.RT_UPDATE_REORDER | abi.RT_UPDATE_DEVICE_TILES), "exclude")
    _invalid(L.rt_pose_skin_device(h, C.c_void_p(16), abi.RT_UPDATE_REORDER | abi.RT_UPDATE_DEVICE_TILES, None), "exclude")
    _invalid(L.rt_pose_skin(h, rt._fp(xf), 0), "no skin")
    _invalid(L.rt_pose_skin_device(h, C.c_void_p(16), abi.RT_UPDATE_DEVICE_TILES, None), "no skin")
    assert bytes(fake.raw) == bytes(1 << 16)                                 # and none of it wrote the context
