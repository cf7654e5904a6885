"""-m gpu: rigid objects — rt_set_objects snapshots a rest pose on the device, rt_pose_objects / rt_pose_objects_device pose
triangle ranges of it with one 3x4 matrix per object.  After every pose the context must give exactly the bits of
rt_update_scene(pack(Scene.posed(ranges, xforms))): every frame is checked (ARGB and the float tap) against the CPU oracle on
Scene.posed and against a fresh context rt_init'ed with it (test_gpu_scene_update._check), the tile data against a context
updated with the same posed arrays and the same flags."""
import numpy as np
import pytest

import test_gpu_scene_update as su
from conftest import focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

VIEWS = su.VIEWS
SHORT_BLOCK, TALL_BLOCK = (su.SHORT_BLOCK[0], len(su.SHORT_BLOCK)), (18, 8)      # the two blocks of LoadTestModel
FLAG_KW = {0: {}, abi.RT_UPDATE_DEVICE_TILES: {"device_tiles": True}, abi.RT_UPDATE_REORDER: {"reorder": True}}


def rot_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def xform(matrix=np.eye(3), offset=(0.0, 0.0, 0.0), about=None):
    """[3,4] float32: matrix | translation; with `about` the matrix acts about that point.  (How the entries are rounded
    does not matter: the device and Scene.posed receive the same float32 values.)"""
    m = np.asarray(matrix, np.float64)
    t = np.asarray(offset, np.float64)
    if about is not None:
        t = t + np.asarray(about, np.float64) - m @ np.asarray(about, np.float64)
    return np.concatenate([m, t[:, None]], axis=1).astype(np.float32)


IDENT = xform()


def centre_of(scene, first, count):
    return scene.aos[first:first + count, :3, :3].reshape(-1, 3).mean(axis=0)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---- box: n <= 64, the wave kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, abi.RT_FLAG_NO_CULL, abi.RT_FLAG_GENERIC_KERNEL])
def test_box_blocks(flags, scene, oracle):
    cfg = abi.make_config(width=64, height=48, aa_x=2, aa_y=1, shadow_samples=4, flags=flags)
    ranges = [SHORT_BLOCK, TALL_BLOCK]
    cs, ct = centre_of(scene, *SHORT_BLOCK), centre_of(scene, *TALL_BLOCK)
    poses = [
        [xform(rot_y(0.3), (0.1, 0.0, -0.05), about=cs), xform(rot_y(-0.3), (-0.05, 0.0, 0.1), about=ct)],   # rotation + translation
        [xform(np.diag([-1.0, 1.0, 1.0]), about=cs), IDENT],                                                 # a mirror (det < 0)
        # the short block (diffuse: no glass in it) lifted into the light's path, between the light and the floor
        [xform(np.eye(3), np.array([0.0, -0.2, -0.7]) - cs), IDENT],
        [IDENT, IDENT],
    ]
    tr = rt.RayTracer(cfg, scene)
    rest = su._check(tr, cfg, scene, oracle)
    tr.set_objects(ranges)
    assert tr.object_count() == 2
    for k, pose in enumerate(poses):
        tr.pose_objects(np.stack(pose))
        frames = su._check(tr, cfg, scene.posed(ranges, np.stack(pose)), oracle)
        if k == 0:
            assert not np.array_equal(rest[0][0], frames[0][0])
    # the identity recomputes the normals: the picture is the rest picture
    assert np.array_equal(rest[0][0], frames[0][0])
    tr.close()


# ---- meshes: n > 64, the mesh kernel ------------------------------------------------------------------------------------
def _layouts(both, nf):
    """(ranges, xforms): the whole mesh as one object; two objects, one inside one 64-triangle tile of the caller's order,
    one that ends at triangle n - 1."""
    n = len(both)
    cm = centre_of(both, 26, nf)
    one = [(26, nf)], np.stack([xform(rot_y(0.4), (0.1, -0.05, -0.1), about=cm)])
    ra, rb = (70, 20), slice(n - 30, n)
    assert 64 <= ra[0] and ra[0] + ra[1] <= 128
    two = [ra, rb], np.stack([xform(np.diag([1.0, -0.5, 1.0]), (0.0, 0.1, 0.0), about=centre_of(both, *ra)),
                              xform(rot_y(-0.8), (0.0, 0.0, -0.2), about=centre_of(both, n - 30, 30))])
    return [one, two]


@pytest.mark.parametrize("n_lon,n_lat", [(10, 8), (40, 30)])      # 166: one LDS stage; 2346: HBM records, tile masks
@pytest.mark.parametrize("flags", [0, abi.RT_FLAG_NO_TILE_BINS])
@pytest.mark.parametrize("pose_flags", [0, abi.RT_UPDATE_DEVICE_TILES, abi.RT_UPDATE_REORDER])
def test_mesh_objects(n_lon, n_lat, flags, pose_flags, scene, oracle, tmp_path):
    both, nf = su._mesh_scene(scene, tmp_path, n_lon, n_lat)
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3, flags=flags)
    for ranges, xf in _layouts(both, nf):
        posed = both.posed(ranges, xf)
        tr = rt.RayTracer(cfg, both)
        su._frame(tr, cfg, VIEWS[0])                       # the context has a previous frame
        tr.set_objects(ranges)
        tr.pose_objects(xf, **FLAG_KW[pose_flags])
        su._check(tr, cfg, posed, oracle, VIEWS[:1])
        ref = rt.RayTracer(cfg, both)
        ref.update_scene(posed, **FLAG_KW[pose_flags])
        (o1, t1), (o2, t2) = tr.tile_data(), ref.tile_data()
        assert np.array_equal(o1, o2) and np.array_equal(t1.view(np.uint32), t2.view(np.uint32))
        ref.close()
        tr.close()


@pytest.mark.parametrize("n_lon,n_lat", [(10, 8), (40, 30)])
@pytest.mark.parametrize("pose_flags", [0, abi.RT_UPDATE_DEVICE_TILES])
def test_posed_values_are_the_hosts(n_lon, n_lat, pose_flags, scene, tmp_path):
    """Value by value, not through pixels: the scene the device posed is Scene.posed (rt_scene_transform), every vertex and
    every normal of every triangle bit for bit; the colours and the triangles in no object are the rest scene's."""
    both, nf = su._mesh_scene(scene, tmp_path, n_lon, n_lat)
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    rest = both.packed()
    for ranges, xf in _layouts(both, nf):
        want = both.posed(ranges, xf).packed()
        tr = rt.RayTracer(cfg, both)
        tr.set_objects(ranges)
        tr.pose_objects(xf, **FLAG_KW[pose_flags])
        d = tr.scene_data()
        assert np.array_equal(d["vertices"].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(d["normals"].view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(d["colors"].view(np.uint32), rest[2].view(np.uint32))
        assert not np.array_equal(d["vertices"], rest[0])
        static = np.ones(len(both), bool)
        for first, count in rt._object_ranges(ranges, len(both)):
            static[first:first + count] = False
        assert static.any() and np.array_equal(d["normals"].view(np.uint32)[static], rest[1].view(np.uint32)[static])
        assert np.array_equal(d["vertices"].view(np.uint32).reshape(-1, 12)[static], rest[0].view(np.uint32).reshape(-1, 12)[static])
        tr.close()


@pytest.fixture(scope="module")
def small(scene, tmp_path_factory):
    """Box + the 140-triangle sphere, its mesh as one object."""
    both, nf = su._mesh_scene(scene, tmp_path_factory.mktemp("pose"), 10, 8)
    return both, [(26, nf)], centre_of(both, 26, nf)


def _spin(centre, angle):
    return np.stack([xform(rot_y(angle), about=centre)])


def test_no_drift(small):
    both, ranges, cm = small
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    a, b = rt.RayTracer(cfg, both), rt.RayTracer(cfg, both)
    a.set_objects(ranges)
    b.set_objects(ranges)
    for k in range(40):
        a.pose_objects(_spin(cm, 0.1 * k))
    a.pose_objects(_spin(cm, 0.7))
    b.pose_objects(_spin(cm, 0.7))
    for view in VIEWS:
        assert _same(su._frame(a, cfg, view), su._frame(b, cfg, view))
    (o1, t1), (o2, t2) = a.tile_data(), b.tile_data()
    assert np.array_equal(o1, o2) and np.array_equal(t1.view(np.uint32), t2.view(np.uint32))
    a.close(); b.close()


@pytest.mark.parametrize("device_tiles", [False, True])
def test_device_entry_ordering(device_tiles, small, oracle):
    import torch
    both, ranges, cm = small
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    xf = _spin(cm, 0.5)
    host = rt.RayTracer(cfg, both)
    host.set_objects(ranges)
    host.pose_objects(xf, device_tiles=device_tiles)
    want = su._frame(host, cfg, VIEWS[0])
    host.close()
    tr = rt.RayTracer(cfg, both)
    tr.set_objects(ranges)
    d_xf = torch.from_numpy(xf).cuda()
    out = (torch.zeros((48, 64), dtype=torch.int32, device="cuda"), torch.zeros((48, 64, 4), device="cuda"))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    tr.pose_objects_device(d_xf, stream=s1, device_tiles=device_tiles)
    su._render_dev(tr, cfg, VIEWS[0], out, s2)             # another stream, no host synchronisation in between
    s1.synchronize()
    d_xf.fill_(float("nan"))                               # the stream has passed the pose: the source may change
    s2.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), want[0])
    assert np.array_equal(out[1].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert su._same_as_oracle(out, su._oracle_frame(oracle, cfg, both.posed(ranges, xf), VIEWS[0]))
    tr.close()


def test_the_other_calls_see_the_pose(small):
    both, ranges, cm = small
    cfg = abi.make_config(width=48, height=32, shadow_samples=4)
    xf = np.stack([xform(rot_y(0.6), (0.1, 0.0, -0.2), about=cm)])
    posed = both.posed(ranges, xf)
    tr, fresh = rt.RayTracer(cfg, both), rt.RayTracer(cfg, posed)
    tr.set_objects(ranges)
    tr.pose_objects(xf)
    rng = np.random.default_rng(11)
    start = rng.uniform(-0.9, 0.9, size=(2000, 3)).astype(np.float32)
    d = rng.normal(size=(2000, 3)).astype(np.float32)
    aim = posed.aos[26:, :3, :3].reshape(-1, 3).mean(axis=0) - start[:700]          # a third of the rays at the posed mesh
    d[:700] = aim
    rays = np.concatenate([start, d], axis=1)
    (tri, hit), (f_tri, f_hit) = tr.query_closest_hit(rays), fresh.query_closest_hit(rays)
    assert np.array_equal(tri, f_tri) and np.array_equal(hit.view(np.uint32), f_hit.view(np.uint32))
    assert (tri >= 26).sum() > 100
    on = tri >= 0                                                                    # shade the hit points, with their normals
    light = VIEWS[0][3]
    got, want = tr.shade_points(hit[on, 0:3], hit[on, 3:6], light), fresh.shade_points(hit[on, 0:3], hit[on, 3:6], light)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (got > 0).any()
    yaw, pitch, cam, li = VIEWS[1]
    rot = rt.rotation_matrix(yaw, pitch)
    assert tr.count_work(rot, cam, li, focal_for(cfg)) == fresh.count_work(rot, cam, li, focal_for(cfg))
    g, w = tr.render_aov(rot, cam, focal_for(cfg)), fresh.render_aov(rot, cam, focal_for(cfg))
    for name in w:
        assert np.array_equal(g[name].view(np.uint32), w[name].view(np.uint32)), name
    got, want = tr.radiance_rays(rays[:500], light), fresh.radiance_rays(rays[:500], light)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    tr.close(); fresh.close()


@pytest.mark.parametrize("pose_flags", [0, abi.RT_UPDATE_DEVICE_TILES, abi.RT_UPDATE_REORDER])
def test_rejected_poses_keep_everything(pose_flags, small, oracle):
    import torch
    both, ranges, cm = small
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    tr = rt.RayTracer(cfg, both)
    tr.set_objects(ranges)
    tr.pose_objects(_spin(cm, 0.3))
    want = su._frame(tr, cfg, VIEWS[0])
    nan = _spin(cm, 0.2); nan[0, 1, 2] = np.nan
    far = _spin(cm, 0.2); far[0, 0, 3] = 2.0 ** 17              # every vertex of the object beyond 2^16
    for bad in (nan, far):
        with pytest.raises(rt.RtError) as e:
            tr.pose_objects(bad, **FLAG_KW[pose_flags])
        assert e.value.code == abi.RT_E_INVALID
        d_bad = torch.from_numpy(bad).cuda()
        torch.cuda.synchronize()
        with pytest.raises(rt.RtError) as e:
            tr.pose_objects_device(d_bad, **FLAG_KW[pose_flags])
        assert e.value.code == abi.RT_E_INVALID
        assert tr.object_count() == 1
        assert _same(su._frame(tr, cfg, VIEWS[0]), want)
    ok = _spin(cm, -0.4)
    tr.pose_objects(ok, **FLAG_KW[pose_flags])                 # from the rest pose, not from the pose of 0.3
    su._check(tr, cfg, both.posed(ranges, ok), oracle, VIEWS[:1])
    tr.close()


def _pose_rc(tr, xf):
    return rt.lib().rt_pose_objects(tr._h, rt._fp(np.ascontiguousarray(xf, np.float32)), 0)


def _no_table(tr):
    assert _pose_rc(tr, IDENT) == abi.RT_E_INVALID
    assert "no object table" in rt.lib().rt_last_error().decode()
    assert tr.object_count() == 0 and tr.objects is None


def test_lifetime_of_the_table(small, scene, oracle):
    both, ranges, cm = small
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    tr = rt.RayTracer(cfg, scene)                               # 26 triangles
    _no_table(tr)                                               # before the first rt_set_objects
    tr.set_objects([SHORT_BLOCK])
    tr.pose_objects(np.stack([xform(np.eye(3), (0.1, 0.0, 0.0))]))
    tr.update_spheres(abi.REFERENCE_SPHERES[:1])                # the spheres do not touch the table
    assert tr.object_count() == 1
    tr.update_scene(scene)
    _no_table(tr)
    tr.set_objects([SHORT_BLOCK, TALL_BLOCK])
    assert tr.object_count() == 2
    tr.replace_scene(both)                                      # across n = 64
    _no_table(tr)
    # objects again, on the new scene
    tr.set_objects(ranges)
    xf = _spin(cm, 0.9)
    tr.pose_objects(xf)
    cfg1 = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3, spheres=abi.REFERENCE_SPHERES[:1])
    su._check(tr, cfg1, both.posed(ranges, xf), oracle, VIEWS[:1])
    # bad tables leave the old one in force
    n = len(both)
    for bad in ([(26, 40), (60, 10)], [(n - 5, 6)], [(-1, 3)], [(30, 0)], [(n, 1)]):
        with pytest.raises(rt.RtError) as e:
            tr.set_objects(bad)
        assert e.value.code == abi.RT_E_INVALID
        assert tr.object_count() == 1
    xf = _spin(cm, -0.5)
    tr.pose_objects(xf)                                         # still the rest pose and the ranges of the last good call
    su._check(tr, cfg1, both.posed(ranges, xf), oracle, VIEWS[:1])
    tr.set_objects([])
    _no_table(tr)
    tr.close()


def test_multi_device_context(small):
    import torch
    both, ranges, cm = small
    kw = dict(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    cfg = abi.make_config(**kw)
    multi = rt.RayTracer(abi.make_config(devices=(0, 0), device_band_rows=8, **kw), both)
    single = rt.RayTracer(cfg, both)
    for tr in (multi, single):
        tr.set_objects(ranges)
        tr.pose_objects(_spin(cm, 0.35))
    for view in VIEWS:
        assert _same(su._frame(multi, cfg, view), su._frame(single, cfg, view))
    xf = _spin(cm, -0.6)
    d_xf = torch.from_numpy(xf).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    multi.pose_objects_device(d_xf, stream=stream, device_tiles=True)
    single.pose_objects(xf, device_tiles=True)
    stream.synchronize()
    for view in VIEWS:
        assert _same(su._frame(multi, cfg, view), su._frame(single, cfg, view))
    with pytest.raises(rt.RtError):
        bad = xf.copy(); bad[0, 2, 3] = np.inf
        multi.pose_objects(bad)
    assert _same(su._frame(multi, cfg, VIEWS[0]), su._frame(single, cfg, VIEWS[0]))
    multi.close(); single.close()
