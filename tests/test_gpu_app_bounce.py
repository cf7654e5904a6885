"""-m gpu: uob_raytracer --bounce-sphere moves sphere 0 along its parabola through rt_update_spheres; the saved frame is
the CPU oracle's frame for the sphere position (and the light position) of the last frame."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_host_surface import read_bmp
from uob_raytracer_amd import abi, runtime as rt


@pytest.mark.gpu
def test_bounce_sphere_matches_the_oracle(tmp_path, scene, oracle):
    exe = os.path.join(ROOT, "uob_raytracer_amd", "uob_raytracer")
    out = str(tmp_path / "bounce.bmp")
    frames = 3
    res = subprocess.run([exe, "--size", "128", "--frames", str(frames), "--bounce-sphere", "--out", out], check=True,
                         capture_output=True, text=True)
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
    u = f32(frames % 8) * f32(0.125)                      # bounce_sphere(frames), float32 operation by operation
    cx = f32(0.3) - u * f32(0.25)
    cy = f32(0.1) - (u * (f32(1.0) - u)) * f32(0.8)
    glass, mirror = abi.REFERENCE_SPHERES
    moved = ((float(cx), float(cy), glass[0][2]), glass[1], glass[2])
    cfg = abi.make_config(width=128, height=128, spheres=(moved, mirror))
    v, n, c = scene.packed()
    focal = 1100.0 * 128 / 1024 * 2
    want, _ = oracle.render(cfg, v, n, c, rt.rotation_matrix(0.0, 0.0), [0.0, 0.0, -3.2], [lx, -0.5, -0.7], focal)
    got = read_bmp(out)
    assert np.array_equal(got.ravel(), want)
    still, _ = oracle.render(abi.make_config(width=128, height=128), v, n, c, rt.rotation_matrix(0.0, 0.0), [0.0, 0.0, -3.2],
                             [lx, -0.5, -0.7], focal)
    assert not np.array_equal(want, still)                # the ball has moved in the picture
