"""-m gpu: uob_raytracer --spin turns the loaded mesh as one rigid object through rt_set_objects / rt_pose_objects; the saved
frame is the Python frame of Scene.posed with the matrix of the last frame (and the light position of the last frame)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_host_surface import read_bmp
from uob_raytracer_amd import abi, runtime as rt


@pytest.mark.gpu
def test_spin_matches_scene_posed(tmp_path, scene, oracle):
    exe = os.path.join(ROOT, "uob_raytracer_amd", "uob_raytracer")
    obj = os.path.join(ROOT, "tests", "golden", "mesh_small.obj")
    out = str(tmp_path / "spin.bmp")
    frames, rad = 3, 0.2
    res = subprocess.run([exe, "--size", "128", "--frames", str(frames), "--obj", obj, "--spin", repr(rad), "--out", out],
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
    # spin_mesh(frames), float32 operation by operation: M = rt_rotation_matrix(f * RAD, 0), t = c - M c about the centre c
    # of the rest mesh's bounding box
    v = mesh.aos[:, :3, :3].reshape(-1, 3)
    c = (v.min(axis=0) + v.max(axis=0)) * f32(0.5)
    xf = rt.rotation_matrix(f32(frames) * f32(rad), 0.0).reshape(3, 4).copy()
    for r in range(3):
        xf[r, 3] = c[r] - ((c[0] * xf[r, 0] + c[1] * xf[r, 1]) + c[2] * xf[r, 2])
    both = scene + mesh
    ranges = [(len(scene), len(mesh))]
    posed = both.posed(ranges, xf[None])
    cfg = abi.make_config(width=128, height=128)
    focal = 1100.0 * 128 / 1024 * 2
    view = (rt.rotation_matrix(0.0, 0.0), [0.0, 0.0, -3.2], [lx, -0.5, -0.7], focal)
    tr = rt.RayTracer(cfg, posed)
    want = tr.render(*view)
    tr.close()
    got = read_bmp(out)
    assert np.array_equal(got, want)
    pv, pn, pc = posed.packed()
    o_argb, _ = oracle.render(cfg, pv, pn, pc, *view)                 # and that frame is the oracle's
    assert np.array_equal(got.ravel(), o_argb)
    tr = rt.RayTracer(cfg, both)
    still = tr.render(*view)
    tr.close()
    assert not np.array_equal(want, still)                            # the mesh has turned in the picture
