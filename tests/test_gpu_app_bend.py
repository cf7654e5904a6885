"""-m gpu: uob_raytracer --bend skins the loaded mesh to two bones by height through rt_set_skin / rt_pose_skin; the saved
frame is the Python frame of Scene.skinned with the weights and the bone of the last frame (and the light position of the last
frame)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_host_surface import read_bmp
from uob_raytracer_amd import abi, runtime as rt


@pytest.mark.gpu
def test_bend_matches_scene_skinned(tmp_path, scene, oracle):
    exe = os.path.join(ROOT, "uob_raytracer_amd", "uob_raytracer")
    obj = os.path.join(ROOT, "tests", "golden", "mesh_small.obj")
    out = str(tmp_path / "bend.bmp")
    frames, rad = 3, 0.2
    res = subprocess.run([exe, "--size", "128", "--frames", str(frames), "--obj", obj, "--bend", repr(rad), "--out", out],
                         check=True, capture_output=True, text=True)
    assert res.stdout.count("Frame Rate:") == frames
    f32 = np.float32
    lx, lor = f32(0.0), True                              # update()'s light oscillation, as test_host_surface replays it
    for _ in range(frames):
        if lor:
            diff = f32(-0.5) - lx
            if diff > f32(-0.001):
                lor = False
        else:
            diff = f32(0.5) - lx
            if diff < f32(0.001):
                lor = True
        lx = lx + diff / f32(20.0)
    mesh = rt.Scene.load_obj(obj)
    # bend_begin() and bend_mesh(frames), float32 operation by operation: the weight of bone 1 is (y - ymin) / (ymax - ymin)
    # of the rest corner, clamped, bone 0 gets 1 - that; bone 0 is the identity, bone 1 M = rt_rotation_matrix(f * RAD, 0)
    # with t = c - M c about the centre c of the rest mesh's bounding box
    v = mesh.aos[:, :3, :3].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c = (lo + hi) * f32(0.5)
    t = np.clip((v[:, 1] - lo[1]) / (hi[1] - lo[1]), f32(0.0), f32(1.0))
    assert t.dtype == f32 and t.min() == 0.0 and t.max() == 1.0
    idx = np.zeros((len(v), 4), np.uint16)
    idx[:, 1] = 1
    w = np.zeros((len(v), 4), f32)
    w[:, 0], w[:, 1] = f32(1.0) - t, t
    bones = np.zeros((2, 3, 4), f32)
    bones[0, :, :3] = np.eye(3, dtype=f32)
    xf = rt.rotation_matrix(f32(frames) * f32(rad), 0.0).reshape(3, 4).copy()
    for r in range(3):
        xf[r, 3] = c[r] - ((c[0] * xf[r, 0] + c[1] * xf[r, 1]) + c[2] * xf[r, 2])
    bones[1] = xf
    both = scene + mesh
    bent = both.skinned(len(scene), len(mesh), idx, w, bones)
    cfg = abi.make_config(width=128, height=128)
    focal = 1100.0 * 128 / 1024 * 2
    view = (rt.rotation_matrix(0.0, 0.0), [0.0, 0.0, -3.2], [lx, -0.5, -0.7], focal)
    tr = rt.RayTracer(cfg, bent)
    want = tr.render(*view)
    tr.close()
    got = read_bmp(out)
    assert np.array_equal(got, want)
    pv, pn, pc = bent.packed()
    o_argb, _ = oracle.render(cfg, pv, pn, pc, *view)                 # and that frame is the oracle's
    assert np.array_equal(got.ravel(), o_argb)
    tr = rt.RayTracer(cfg, both)
    still = tr.render(*view)
    tr.close()
    assert not np.array_equal(want, still)                            # the mesh has bent in the picture
