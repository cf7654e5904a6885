"""-m gpu: rt_skin_triangles beyond its capped grid (2048 workgroups of 256 lanes, shared with rt_pose_triangles: DESIGN.md
4.2d) and at the bone limit: one scene just above the cap, skinned whole with 65 535 bones and indices up to 65 534, compared
with Scene.skinned on the host value by value, bit for bit."""
import numpy as np
import pytest

import scene_sizes_util as U
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

F32 = np.float32


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_skin_beyond_the_grid_cap(scene):
    import torch
    nbones = U.MAX_OBJECTS
    rest, ranges, centres = U.pose_scene(scene, nbones)
    n = len(rest)
    assert nbones == 65535 and n == 524306 and 0 < n - U.POSE_GRID < 256      # the loop's second trip, in one workgroup
    # influences: the bone of the triangle's object (the box: the highest bones), a scattered second bone, the last bone
    tri = np.arange(n)
    own = np.where(tri < U.N_BOX, nbones - 1 - tri, (tri - U.N_BOX) // U.OBJ_TRIS)
    idx = np.zeros((3 * n, 4), np.uint16)
    idx[:, 0] = np.repeat(own, 3)
    idx[:, 1] = (np.repeat(own, 3) * 7919 + np.arange(3 * n)) % nbones
    idx[:, 2] = nbones - 1
    idx[:, 3] = np.arange(3 * n) % 251
    assert idx.max() == 65534 and (idx[-3:, 0] == 65534).all() and idx[0, 0] == 65534
    w = np.zeros((3 * n, 4), F32)
    w[:] = (0.625, 0.25, 0.125, 0.0)
    rest_packed = rest.packed()
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=1)
    tr = rt.RayTracer(cfg, rest)
    tr.set_skin(0, n, idx, w, nbones)
    assert tr.skin_info() == (0, n, nbones)
    for entry, seed in (("host", 9), ("device", 10)):
        bones = U.pose_xforms(centres, seed=seed)
        want = rest.skinned(0, n, idx, w, bones).packed()
        if entry == "host":
            tr.pose_skin(bones)
        else:
            d_bones = torch.from_numpy(bones).cuda()
            torch.cuda.synchronize()
            tr.pose_skin_device(d_bones, stream=torch.cuda.Stream(), device_tiles=True)
            torch.cuda.synchronize()
        d = tr.scene_data()
        assert np.array_equal(_u32(d["vertices"]), _u32(want[0])), entry       # all n, the tail past the cap included
        assert np.array_equal(_u32(d["normals"]), _u32(want[1])), entry
        assert np.array_equal(_u32(d["colors"]), _u32(rest_packed[2])), entry
        tail = slice(3 * U.POSE_GRID, 3 * n)
        assert not np.array_equal(_u32(d["vertices"])[tail], _u32(rest_packed[0])[tail])
    tr.close()
