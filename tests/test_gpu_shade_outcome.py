"""-m gpu: shade() (rt_wave_common.h) sums a ray's light the way the task's shadow outcome allows — no sum where no lane
needs one, the plain chain where no lane is in penumbra (blocked lanes take 0.0f + 0.0f * term), the predicated chain
otherwise — and every form must leave the bits of direct_light's sequential sum.

Frames: every case renders with the shipped path, without the cull (RT_FLAG_NO_CULL), with the one-thread-per-pixel kernel
(RT_FLAG_GENERIC_KERNEL) and with the unspecialised wave kernel (UOB_RT_NO_SPECIALISE=1) — identical bits, ARGB and float
tap; two frames are also compared with the CPU oracle.  The settings reach the instantiations specialised on 64 samples
(the dispatch, straight-line sums) and on 10 (which keep the two forms they had), the run-time sample count with few samples, more than 64 samples (MULTI), more than 64 AA
samples per pixel (BIGAA) and the mesh kernel; the cases put whole tasks outside the box, tasks half outside it, the whole
floor in umbra, a wall at term == 0 and bounced (secondary) lanes in front of the sums.

Lanes: rt_selftest_shade runs shade() on waves whose lanes the test chooses — every dispatch class, the sample counts
1, 5, 10, 16, 64, 96 and the terms +0, -0, a denormal, 1e-30, 1, 1e30, +inf, NaN — against a float32 sequential sum
written here.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DEFAULT_CAM, DEFAULT_LIGHT, ROOT, focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

MIRROR = (1.0, 1.0, 1.0, 0.0)
FLOOR = [0, 1]            # TestModelH.h: floor, left wall, right wall, ceiling, back wall, two triangles each
LEFT_WALL = [2, 3]
BACK_WALL = [8, 9]

SETTINGS = [
    dict(width=256, height=128, aa_x=4, aa_y=2, shadow_samples=64),     # the headline instantiation
    dict(width=256, height=160, aa_x=2, aa_y=2, shadow_samples=10),     # the reference's constants
    dict(width=128, height=64, aa_x=3, aa_y=3, shadow_samples=5),       # run-time sample count, packed level 3
    dict(width=128, height=64, aa_x=2, aa_y=2, shadow_samples=96),      # two passes of sample lanes
    dict(width=64, height=32, aa_x=9, aa_y=9, shadow_samples=16),       # 81 AA samples per pixel: two tasks per pixel
    dict(width=128, height=128, shadow_samples=1, mesh=True),           # box + mesh: the tiled mesh kernel
]
CASES = ["default_view", "pulled_back", "floor_in_umbra", "light_in_wall_plane", "mirror_back_wall"]
ORACLE_CASES = {("floor_in_umbra", 1), ("pulled_back", 2)}


def _renormal(aos):
    tri = aos.ctypes.data_as(C.POINTER(abi.RtTriangle))
    for i in range(aos.shape[0]):
        rt.lib().rt_triangle_compute_normal(C.byref(tri[i]))


def _case(name, scene):
    """-> (scene, extra config, (yaw, pitch), cam, light)"""
    view0 = (0.0, 0.0)
    if name == "default_view":
        return scene, {}, view0, DEFAULT_CAM, DEFAULT_LIGHT
    if name == "pulled_back":                  # the box fills part of the frame: tasks outside it, tasks across its outline
        return scene, {}, (0.15, 0.05), [0.6, -0.2, -4.6], DEFAULT_LIGHT
    if name == "floor_in_umbra":               # a quad a little below the light, wider than the light's jitter by far
        q = scene.aos[FLOOR].copy()
        q[:, :3, 0] = np.float32(0.6) * q[:, :3, 0] + np.float32(DEFAULT_LIGHT[0])
        q[:, :3, 2] = np.float32(0.6) * q[:, :3, 2] + np.float32(DEFAULT_LIGHT[2])
        q[:, :3, 1] = np.float32(DEFAULT_LIGHT[1]) + np.float32(0.1)       # y points down
        q[:, 4, :] = np.asarray((0.2, 0.7, 0.3, 1.0), np.float32)
        _renormal(q)
        return scene + rt.Scene(q), {}, view0, DEFAULT_CAM, DEFAULT_LIGHT
    if name == "light_in_wall_plane":          # term == 0 on the whole wall
        x = float(scene.aos[LEFT_WALL[0], 0, 0])
        assert (scene.aos[LEFT_WALL, :3, 0] == x).all()
        return scene, {}, view0, DEFAULT_CAM, [x, 0.2, -0.3]
    if name == "mirror_back_wall":             # secondary lanes
        return scene.with_color(BACK_WALL, MIRROR), dict(max_bounces=5), (0.2, -0.1), [0.1, 0.0, -3.0], [0.2, -0.4, -0.6]
    raise KeyError(name)


def _render(kw, flags, scene, rot, cam, light, unspecialised=False):
    cfg = abi.make_config(flags=flags, **kw)
    if unspecialised:
        os.environ["UOB_RT_NO_SPECIALISE"] = "1"        # read by rt_init
    try:
        tr = rt.RayTracer(cfg, scene)
    finally:
        if unspecialised:
            del os.environ["UOB_RT_NO_SPECIALISE"]
    argb, rgb = tr.render(rot, cam, light, focal_for(cfg), want_rgb=True)
    tr.close()
    return argb, rgb


@pytest.fixture(scope="module")
def mesh_scene(scene):
    return scene + rt.Scene.load_obj(os.path.join(ROOT, "tests", "golden", "mesh_small.obj"))


@pytest.mark.parametrize("si", range(len(SETTINGS)))
@pytest.mark.parametrize("name", CASES)
def test_shade_outcome_changes_no_pixel(name, si, scene, mesh_scene, oracle):
    kw = dict(SETTINGS[si])
    mesh = kw.pop("mesh", False)
    s, extra, (yaw, pitch), cam, light = _case(name, mesh_scene if mesh else scene)
    assert (len(s) > 64) == mesh                          # more than 64 triangles run on the mesh kernel
    kw.update(extra)
    rot = rt.rotation_matrix(yaw, pitch)
    a0, f0 = _render(kw, 0, s, rot, cam, light)
    hit = (a0 != 0xFF000000).mean()
    assert hit > 0.15, "the view misses the scene"
    if name == "pulled_back":
        assert hit < 0.6, "the view has no tasks outside the box"
    others = {"no cull": _render(kw, abi.RT_FLAG_NO_CULL, s, rot, cam, light),
              "generic kernel": _render(kw, abi.RT_FLAG_GENERIC_KERNEL, s, rot, cam, light),
              "unspecialised wave kernel": _render(kw, 0, s, rot, cam, light, unspecialised=True)}
    for what, (a, f) in others.items():
        bad = np.argwhere(a0 != a)
        assert bad.size == 0, "shipped path differs from %s in %d pixels, first at %s" % (what, len(bad), bad[0])
        assert np.array_equal(f0.view(np.uint32), f.view(np.uint32)), what
    if (name, si) in ORACLE_CASES:
        cfg = abi.make_config(**kw)
        v, n, c = s.packed()
        want, _ = oracle.render(cfg, v, n, c, rot, cam, light, focal_for(cfg), nthreads=8)
        assert np.array_equal(a0.ravel(), want)


# ---- shade() lane by lane ------------------------------------------------------------------------------------------

NS_VALUES = [1, 5, 10, 16, 64, 96]
TERMS = np.array([0.0, -0.0, 1e-40, 1e-30, 1.0, 1e30, np.inf, np.nan], np.float32)
CLASSES = ["all_unlit", "all_blocked", "blocked_and_lit", "one_partial", "all_partial", "unlit_and_lit", "mixed"]


def _wave(cls, ns, rng):
    """-> lit [64], unshadowed [64] of one wave of the dispatch class"""
    part = lambda k: rng.integers(1, ns, k) if ns > 1 else rng.integers(0, 2, k) * ns     # (one sample: no penumbra)
    lit = np.ones(64, np.int32)
    if cls == "all_unlit":
        return np.zeros(64, np.int32), rng.integers(0, ns + 1, 64)
    if cls == "all_blocked":
        u = np.zeros(64, np.int64)
    elif cls == "blocked_and_lit":
        u = rng.integers(0, 2, 64) * ns
        u[3], u[40] = 0, ns
    elif cls == "one_partial":
        u = rng.integers(0, 2, 64) * ns
        u[17] = part(1)[0]
    elif cls == "all_partial":
        u = part(64)
    elif cls == "unlit_and_lit":
        u = np.full(64, ns)
    else:
        u = rng.integers(0, ns + 1, 64)
    if cls in ("blocked_and_lit", "one_partial", "unlit_and_lit", "mixed"):
        lit = (rng.random(64) < 0.8).astype(np.int32)
        if cls != "mixed":
            lit[[3, 17, 40]] = 1
    u = np.where(lit != 0, u, rng.integers(-1, ns + 2, 64))       # an unlit lane's count is never read
    return lit, u


def _shade_ref(ns, lit, secondary, unshadowed, term, col):
    """direct_light's sum (one add of 0 * term if a sample was blocked, then term once per unblocked sample, in sequence),
    0.5 + total / S, times 0.9 for a secondary ray, times the colour — all in float32."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        total = np.where(unshadowed < ns[:, None], f32(0.0) + f32(0.0) * term, f32(0.0)).astype(f32)
        for i in range(int(ns.max())):
            total = np.where(i < np.minimum(unshadowed, ns[:, None]), total + term, total).astype(f32)
        l = (f32(0.5) + total / ns[:, None].astype(f32)).astype(f32)
        k = np.where(secondary != 0, f32(0.9) * l, l).astype(f32)
        out = (col[:, :, :3] * k[:, :, None]).astype(f32)
    return np.where((lit != 0)[:, :, None], out, f32(0.0)).astype(f32)


@pytest.fixture(scope="module")
def lanes():
    rng = np.random.default_rng(20260)
    ns, lit, unsh, term = [], [], [], []
    for n in NS_VALUES:
        for cls in CLASSES:
            for t in TERMS:                                # one term in every lane ...
                l, u = _wave(cls, n, rng)
                ns.append(n); lit.append(l); unsh.append(u); term.append(np.full(64, t, np.float32))
            for _ in range(2):                             # ... and the terms mixed over the lanes
                l, u = _wave(cls, n, rng)
                ns.append(n); lit.append(l); unsh.append(u); term.append(rng.choice(TERMS, 64))
    ns = np.asarray(ns, np.int32)
    lit, unsh, term = np.asarray(lit, np.int32), np.asarray(unsh, np.int32), np.asarray(term, np.float32)
    secondary = rng.integers(0, 2, lit.shape).astype(np.int32)
    col = rng.random(lit.shape + (4,)).astype(np.float32)
    col[:, ::7, 1] = 0.0
    return ns, lit, secondary, unsh, term, col, _shade_ref(ns, lit, secondary, unsh, term, col)


@pytest.mark.parametrize("straight_line", [False, True])
def test_shade_lanes_match_sequential_sum(lanes, straight_line):
    ns, lit, secondary, unsh, term, col, want = lanes
    got = rt.selftest_shade(ns, lit, secondary, unsh, term, col, straight_line=straight_line)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))     # (any NaN for a NaN)
    bad = np.argwhere(~same)
    assert bad.size == 0, "wave %d (S = %d) lane %d: got %r, want %r, term %r, unshadowed %d" % (
        bad[0][0], ns[bad[0][0]], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], term[bad[0][0], bad[0][1]],
        unsh[bad[0][0], bad[0][1]])
