"""CPU: the builders and restatements of tests/scene_sizes_util.py — counts, coordinate range, no degenerate triangle
unless asked, the extreme vertices and glass colours where the GPU tests need them, and morton_order_np against a naive
per-triangle Python sort."""
import os

import numpy as np
import pytest

import scene_sizes_util as U
from conftest import ROOT

F32 = np.float32


def _areas2(sc):
    a = sc.aos[:, :3, :3].astype(np.float64)
    return np.linalg.norm(np.cross(a[:, 1] - a[:, 0], a[:, 2] - a[:, 0]), axis=1)


def _sound(sc, n):
    assert len(sc) == n and sc.aos.shape == (n, 5, 4) and sc.aos.dtype == F32
    assert np.isfinite(sc.aos).all() and (np.abs(sc.aos[:, :3, :3]) <= 2.0 ** 16).all()
    assert (_areas2(sc) > 1e-9).all()                                           # no degenerate triangle
    assert np.allclose(np.linalg.norm(sc.aos[:, 3, :3], axis=1), 1.0, atol=1e-5)    # the normals are filled


@pytest.mark.parametrize("n", [1024, 1025, 16385])
def test_random_scene(n, scene):
    sc = U.random_scene(scene, n, seed=n)
    _sound(sc, n)
    assert np.array_equal(sc.aos[:U.N_BOX, :3], scene.aos[:, :3])               # the box first, vertices unchanged
    assert np.array_equal(sc.aos[:U.N_BOX, 3].view(np.uint32), scene.aos[:, 3].view(np.uint32))   # and its normals
    assert not np.array_equal(sc.aos, U.random_scene(scene, n, seed=n + 1).aos)
    assert np.array_equal(sc.aos, U.random_scene(scene, n, seed=n).aos)         # seeded


def test_thresholds_arithmetic():
    assert [U.scan_steps(n) for n in (1024, 16384, 16385, 32768, 32769, 40000)] == [1, 1, 2, 2, 3, 3]
    assert [U.sort_chunks(n) for n in (1024, 1025, 16385, 32769)] == [1, 2, 17, 33]
    assert 32769 - 32 * U.SORT_CHUNK == 1                                       # a last chunk of one element


M = 16385


@pytest.mark.parametrize("case", ["equal_keys", "top_byte", "bottom_byte", "hot_digit", "many_large"])
def test_key_cases(case, scene):
    sc = U.key_case(scene, case, M)
    _sound(sc, U.N_BOX + M)
    keys = U.morton_keys_np(sc.packed()[0])
    small = keys[U.N_BOX:]
    if case == "equal_keys":
        assert len(set(small.tolist())) == 1 and small[0] != 0
    if case == "top_byte":
        diff = small ^ small[0]
        assert (diff & np.uint32(0x00FFFFFF) == 0).all() and len(set(small.tolist())) == 8
    if case == "bottom_byte":
        diff = small ^ small[0]
        assert (diff & np.uint32(0xFFFFFF00) == 0).all() and len(set(small.tolist())) > 32
    if case == "hot_digit":
        for shift in (0, 8, 16, 24):
            counts = np.bincount((keys >> np.uint32(shift)) & np.uint32(255), minlength=256)
            assert counts.max() > 0.9 * len(keys), shift
            assert (counts > 0).sum() > (1 if shift < 24 else 0)                # and the digit is not the only one
    if case == "many_large":
        at = U.N_BOX + U.large_positions(M)
        assert len(at) == U.N_LARGE == len(set(at.tolist())) and at[0] == U.N_BOX and at[-1] > U.N_BOX + M - 8
        assert (keys[at] == 0).all()
        rest = np.setdiff1d(np.arange(U.N_BOX, U.N_BOX + M), at)
        assert (keys[rest] != 0).all()
        assert (keys == 0).sum() // 64 >= 46 and (np.diff(at) > 1).all()        # scattered, more than 46 tiles of them


def test_check_scene(scene):
    n = U.CHECK_GRID + U.N_BOX + 70
    sc = U.check_scene(scene, n)
    _sound(sc, n)
    assert n > U.CHECK_GRID and n % 64 != 0
    V = sc.aos[:, :3, :3]
    lo, hi = V.reshape(-1, 3).min(axis=0), V.reshape(-1, 3).max(axis=0)
    first = V[:U.CHECK_GRID].reshape(-1, 3)                                     # the loop's first trip
    assert (first.min(axis=0) > lo).all() and (first.max(axis=0) < hi).all()    # every extreme lies beyond it
    assert np.array_equal(sc.aos[n - U.N_BOX:, :3], scene.aos[:, :3])           # the box last
    glass = np.nonzero(sc.aos[:, 4, 3] == -1.0)[0]
    assert np.array_equal(glass, U.check_glass_indices(n)) and glass.min() >= U.CHECK_GRID
    shrunk = U.check_scene(scene, n, box_scale=0.9)
    _sound(shrunk, n)
    assert np.array_equal(shrunk.aos[:n - U.N_BOX], sc.aos[:n - U.N_BOX])
    assert np.abs(shrunk.aos[:, :3, :3]).max() == F32(0.9)


def test_pose_scene_and_xforms(scene):
    nobj = 300
    sc, ranges, centres = U.pose_scene(scene, nobj)
    _sound(sc, U.N_BOX + U.OBJ_TRIS * nobj)
    assert ranges[0] == (26, 8) and ranges[-1] == (26 + 8 * (nobj - 1), 8) and len(ranges) == nobj
    for k in (0, nobj - 1):
        tri = sc.aos[ranges[k][0]:ranges[k][0] + 8, :3, :3].reshape(-1, 3)
        assert np.abs(tri - centres[k]).max() < 0.02
    xf = U.pose_xforms(centres)
    assert xf.shape == (nobj, 3, 4) and xf.dtype == F32 and np.isfinite(xf).all()
    special = U.special_poses(nobj)
    assert 0 in special["mirror"] and nobj - 1 in special["stretch"] and nobj - 2 in special["zero"]
    det = np.linalg.det(xf[:, :, :3].astype(np.float64))
    plain = np.setdiff1d(np.arange(nobj), sum(special.values(), []))
    assert np.allclose(det[plain], 1.0, atol=1e-5)                              # rotations
    assert np.allclose(det[special["mirror"]], -1.0) and (det[special["zero"]] == 0).all()
    posed = sc.posed(ranges, xf)
    assert (np.abs(posed.aos[:, :3, :3]) <= 1.0).all()                          # the objects stay in the box
    moved = posed.aos[26:, :3, :3].reshape(nobj, -1, 3)
    assert np.abs(moved.mean(axis=1) - centres).max() < 0.05                    # about their centres
    z = special["zero"][0]
    assert np.isnan(posed.aos[ranges[z][0], 3, :3]).all()                       # the collapsed object: degenerate normals
    assert (posed.aos[ranges[z][0], 3, :3].view(np.uint32) == 0xffc00000).all()
    assert np.array_equal(posed.aos[:26], sc.aos[:26])


def test_morton_order_is_a_permutation(scene):
    for sc in (U.random_scene(scene, 5000, 1), U.key_case(scene, "many_large", 4000), U.key_case(scene, "equal_keys", 300)):
        order = U.morton_order_np(sc.packed()[0])
        assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(len(sc)))


def _naive_code(tri, lo, ext, inv):
    """One triangle's key, scalar by scalar, bit by bit."""
    tl = [min(tri[v][k] for v in range(3)) for k in range(3)]
    th = [max(tri[v][k] for v in range(3)) for k in range(3)]
    te = max(F32(th[k] - tl[k]) for k in range(3))
    if te > F32(0.25) * ext:
        return 0
    code = 0x40000000
    for k in range(3):
        f = F32(F32(F32(0.5) * F32(tl[k] + th[k])) - lo[k]) * inv
        q = (int(f) if f < 1023 else 1023) if f >= 0 else 0
        for b in range(10):
            code |= ((q >> b) & 1) << (3 * b + k)
    return code


def test_morton_order_against_a_naive_sort(scene):
    import uob_raytracer_amd.runtime as rt
    mesh = np.load(os.path.join(ROOT, "tests", "golden", "mesh_small_aos.npy"))
    sc = scene + rt.Scene(mesh)
    v4 = sc.packed()[0]
    n = len(sc)
    V = v4.reshape(n, 3, 4)[:, :, :3]
    lo = [min(F32(x) for x in V[:, :, k].ravel()) for k in range(3)]
    hi = [max(F32(x) for x in V[:, :, k].ravel()) for k in range(3)]
    ext = max(F32(hi[k] - lo[k]) for k in range(3))
    inv = F32(1023.0) / ext
    codes = [_naive_code(V[i], lo, ext, inv) for i in range(n)]
    assert 0 < sum(c == 0 for c in codes) < n and len(set(codes)) > 10
    assert codes == U.morton_keys_np(v4).tolist()
    assert sorted(range(n), key=lambda i: (codes[i], i)) == U.morton_order_np(v4).tolist()


def test_tile_sampling():
    keys = np.concatenate([np.zeros(100, np.uint32), np.arange(1, 10000, dtype=np.uint32)])
    tiles = U.sample_tiles(keys)
    ntiles = (len(keys) + 63) // 64
    assert tiles[0] == 0 and tiles[-1] == ntiles - 1 and 2 in tiles and len(tiles) <= 19
    assert tiles == U.sample_tiles(keys) and all(0 <= t < ntiles for t in tiles)
