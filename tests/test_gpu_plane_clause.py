"""-m gpu: level 1's plane clause (rt_wave_common.h plane_slab_tneg) drops, for a task whose lit points all lie on one
triangle, the casters in whose plane that triangle lies.  The scenes below are the smallest in which such a clause can
go wrong: lights that graze a surface or lie in a wall's plane, quads a hair above and below the floor (which really do
or do not shadow it), rows whose jobs cross a face's diagonal and edge (the certified triangle changes inside a job
while level 1 is reused), bounced surface points, the corners of the accepted coordinate domain, and a floor with
reversed winding.  Every case renders with the shipped path, without the cull (RT_FLAG_NO_CULL), with the
one-thread-per-pixel kernel (RT_FLAG_GENERIC_KERNEL) and with the unspecialised wave kernel (UOB_RT_NO_SPECIALISE=1;
both settings run on a specialised instantiation) — identical bits, ARGB and float tap; two small frames are also
compared with the CPU oracle.

The kernel computes the clause only for at least eight AA samples per pixel (jobs of eight tasks), so it is the 4x2
setting that exercises it — in the specialised and, through UOB_RT_NO_SPECIALISE, the unspecialised instantiation; the
2x2 setting (the reference's constants) runs instantiations compiled without it and checks that they stayed what they were.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

MIRROR = (1.0, 1.0, 1.0, 0.0)
FLOOR = [0, 1]            # TestModelH.h: floor, left wall, right wall, ceiling, back wall, two triangles each
LEFT_WALL = [2, 3]
BACK_WALL = [8, 9]

SETTINGS = [
    dict(width=256, height=128, aa_x=4, aa_y=2, shadow_samples=64),     # headline sampling: 8 pixels per task
    dict(width=256, height=160, aa_x=2, aa_y=2, shadow_samples=10),     # the reference's constants: 16 pixels per task
]


def _renormal(aos):
    tri = aos.ctypes.data_as(C.POINTER(abi.RtTriangle))
    for i in range(aos.shape[0]):
        rt.lib().rt_triangle_compute_normal(C.byref(tri[i]))


def _floor_y(scene):
    ys = scene.aos[FLOOR, :3, 1]
    assert (ys == ys.flat[0]).all()
    return float(ys.flat[0])                 # y points down: the floor is the box's largest y


def _with_quad(scene, dy):
    """A copy of the floor's two triangles, 0.4 x the size, over part of the floor, at floor_y + dy (dy < 0: above it)."""
    q = scene.aos[FLOOR].copy()
    q[:, :3, 0] = np.float32(0.4) * q[:, :3, 0] - np.float32(0.15)
    q[:, :3, 2] = np.float32(0.4) * q[:, :3, 2] - np.float32(0.2)
    q[:, :3, 1] = np.float32(_floor_y(scene)) + np.float32(dy)
    q[:, 4, :] = np.asarray((0.2, 0.7, 0.3, 1.0), np.float32)
    _renormal(q)
    return scene + rt.Scene(q)


def _moved(scene, spheres, k, t):
    """x -> k x + t on triangles and spheres, in float32; normals recomputed by the product's ComputeNormal."""
    aos = scene.aos.copy()
    aos[:, :3, :3] = (np.float32(k) * aos[:, :3, :3] + np.asarray(t, np.float32)).astype(np.float32)
    _renormal(aos)
    sph = tuple((tuple((np.float32(k) * np.asarray(c, np.float32) + np.asarray(t, np.float32)).tolist()),
                 float(np.float32(k) * np.float32(k) * np.float32(r2)), col) for c, r2, col in spheres)
    return rt.Scene(aos), sph


def _case(name, scene):
    """-> (scene, extra config, (yaw, pitch), cam, light)"""
    view0 = (0.0, 0.0)
    fy = _floor_y(scene)
    if name.startswith("light_over_floor_"):
        h = float(name.rsplit("_", 1)[1])
        return scene, {}, view0, DEFAULT_CAM, [0.1, float(np.float32(fy) - np.float32(h)), -0.2]
    if name == "light_in_wall_plane":
        x = float(scene.aos[LEFT_WALL[0], 0, 0])
        assert (scene.aos[LEFT_WALL, :3, 0] == x).all()
        return scene, {}, view0, DEFAULT_CAM, [x, 0.2, -0.3]
    if name == "light_at_wall_vertex":
        return scene, {}, view0, DEFAULT_CAM, scene.aos[LEFT_WALL[0], 1, :3].tolist()
    if name.startswith("quad_"):
        _, side, d = name.split("_")
        return _with_quad(scene, -float(d) if side == "above" else float(d)), {}, view0, DEFAULT_CAM, DEFAULT_LIGHT
    if name == "rows_across_diagonal":        # seen from the side and above: the floor's and walls' diagonals cross every row
        return scene, {}, (0.45, 0.3), [0.5, -0.35, -2.6], [-0.3, -0.5, -0.4]
    if name == "rows_across_edges":           # rolled view: the wall / floor / ceiling edges cross the rows obliquely
        return scene, {}, (-0.4, -0.2), [-0.4, 0.2, -2.8], [0.3, -0.4, -0.5]
    if name == "mirror_wall_glass_sphere":    # bench.py's cfg3 scene: bounced surface points
        return scene.with_color(BACK_WALL, MIRROR), dict(max_bounces=5), (0.2, -0.1), [0.1, 0.0, -3.0], [0.2, -0.4, -0.6]
    if name.startswith("moved_"):
        k, t = {"moved_2e-10": (2.0 ** -10, (0.0, 0.0, 0.0)), "moved_2e14": (2.0 ** 14, (0.0, 0.0, 0.0)),
                "moved_by_3e4": (1.0, (3.0e4, -1.5e4, 2.0e4))}[name]
        s, sph = _moved(scene, abi.REFERENCE_SPHERES, k, t)
        mv = lambda p: (np.float32(k) * np.asarray(p, np.float32) + np.asarray(t, np.float32)).tolist()
        return s, dict(spheres=sph, light_spread=0.05 * k), view0, mv(DEFAULT_CAM), mv(DEFAULT_LIGHT)
    if name == "inside_out_floor":            # reversed winding, the stored normal kept: cof(e1, e2) changes sign
        aos = scene.aos.copy()
        aos[FLOOR, 1, :], aos[FLOOR, 2, :] = scene.aos[FLOOR, 2, :], scene.aos[FLOOR, 1, :]
        return rt.Scene(aos), {}, view0, DEFAULT_CAM, DEFAULT_LIGHT
    raise KeyError(name)


CASES = ["light_over_floor_1e-3", "light_over_floor_1e-5", "light_in_wall_plane", "light_at_wall_vertex",
         "quad_above_1e-5", "quad_above_1e-4", "quad_above_1e-3", "quad_below_1e-5", "quad_below_1e-4", "quad_below_1e-3",
         "rows_across_diagonal", "rows_across_edges", "mirror_wall_glass_sphere",
         "moved_2e-10", "moved_2e14", "moved_by_3e4", "inside_out_floor"]
ORACLE_CASES = {("light_over_floor_1e-3", 1), ("quad_above_1e-4", 1)}


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


@pytest.mark.parametrize("si", range(len(SETTINGS)))
@pytest.mark.parametrize("name", CASES)
def test_plane_clause_changes_no_pixel(name, si, scene, oracle):
    s, extra, (yaw, pitch), cam, light = _case(name, scene)
    assert len(s) <= 32                                   # the specialised instantiations take up to 32 triangles
    kw = dict(SETTINGS[si], **extra)
    rot = rt.rotation_matrix(yaw, pitch)
    a0, f0 = _render(kw, 0, s, rot, cam, light)
    assert (a0 != 0xFF000000).mean() > 0.15, "the view misses the scene"
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

