"""-m gpu: skinned meshes — rt_set_skin snapshots a rest pose on the device and uploads four (bone, weight) influences per
corner of a triangle range, rt_pose_skin / rt_pose_skin_device blend the bones' 3x4 matrices per vertex.  After every pose the
context must give exactly the bits of rt_update_scene(pack(Scene.skinned(...))): every frame is checked (ARGB and the float
tap) against the CPU oracle on Scene.skinned and against a fresh context rt_init'ed with it (test_gpu_scene_update._check),
the tile data against a context updated with the same skinned arrays and the same flags."""
import numpy as np
import pytest

import test_gpu_scene_pose as sp
import test_gpu_scene_update as su
from conftest import focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

VIEWS = su.VIEWS
TALL_BLOCK = sp.TALL_BLOCK
FLAG_KW = sp.FLAG_KW
F32 = np.float32
xform, rot_y, centre_of, _same = sp.xform, sp.rot_y, sp.centre_of, sp._same


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def by_height(scene, first, count):
    """Two bones: bone 1 weighs (y - ymin) / (ymax - ymin) of the rest corner, bone 0 the rest."""
    y = scene.aos[first:first + count, :3, 1].reshape(-1)
    t = np.clip((y - y.min()) / (y.max() - y.min()), F32(0), F32(1)).astype(F32)
    idx = np.zeros((3 * count, 4), np.uint16)
    idx[:, 1] = 1
    w = np.zeros((3 * count, 4), F32)
    w[:, 0], w[:, 1] = F32(1) - t, t
    return idx, w


class Skin:
    """A skin and the host's statement of it."""

    def __init__(self, rest, first, count, idx, w, nbones):
        self.rest, self.first, self.count, self.idx, self.w, self.nbones = rest, first, count, idx, w, nbones

    def set(self, tr):
        tr.set_skin(self.first, self.count, self.idx, self.w, self.nbones)
        assert tr.skin_info() == (self.first, self.count, self.nbones) == tr.skin

    def skinned(self, bones):
        return self.rest.skinned(self.first, self.count, self.idx, self.w, bones)


# ---- box: n <= 64, the wave kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, abi.RT_FLAG_NO_CULL, abi.RT_FLAG_GENERIC_KERNEL])
def test_box_block(flags, scene, oracle):
    cfg = abi.make_config(width=64, height=48, aa_x=2, aa_y=1, shadow_samples=4, flags=flags)
    skin = Skin(scene, *TALL_BLOCK, *by_height(scene, *TALL_BLOCK), 2)
    ct = centre_of(scene, *TALL_BLOCK)
    under_light = np.array([0.0, ct[1], -0.7]) - ct             # under the light at (0, -0.5, -0.7): between it and the floor
    poses = [
        [sp.IDENT, xform(rot_y(0.5), (0.05, 0.0, -0.05), about=ct)],                    # a bend
        [sp.IDENT, xform(np.diag([-1.0, 1.0, 1.0]), about=ct)],                         # a mirror (det < 0)
        [xform(np.eye(3), under_light), xform(np.eye(3), under_light - [0.0, 0.1, 0.0])],   # a lift into the light's path
        [sp.IDENT, sp.IDENT],
    ]
    tr = rt.RayTracer(cfg, scene)
    rest = su._check(tr, cfg, scene, oracle)
    skin.set(tr)
    assert tr.object_count() == 0
    for k, pose in enumerate(poses):
        tr.pose_skin(np.stack(pose))
        frames = su._check(tr, cfg, skin.skinned(np.stack(pose)), oracle)
        if k < 3:
            assert not np.array_equal(rest[0][0], frames[0][0])
    # the identity recomputes the normals: the picture is the rest picture
    assert np.array_equal(rest[0][0], frames[0][0])
    tr.close()


# ---- meshes: n > 64, the mesh kernel ------------------------------------------------------------------------------------
def _layouts(both, nf):
    """(Skin, bones): A the whole mesh, two bones by height; B the range (70, 20) inside one 64-triangle tile of the caller's
    order, four non-zero influences per corner; C a range that ends at triangle n - 1, 300 bones, indices above 255 in use."""
    n = len(both)
    rng = np.random.default_rng(21)
    cm = centre_of(both, 26, nf)
    a = Skin(both, 26, nf, *by_height(both, 26, nf), 2)
    bones_a = np.stack([xform(np.eye(3), (0.02, 0.0, 0.0)), xform(rot_y(0.6), (0.1, -0.05, -0.1), about=cm)])
    first, count = 70, 20
    assert 64 <= first and first + count <= 128
    r = rng.uniform(0.1, 1.0, (3 * count, 4))
    w = (r / r.sum(axis=1, keepdims=True)).astype(F32)
    idx = np.stack([rng.permutation(4) for _ in range(3 * count)]).astype(np.uint16)
    assert (w > 0).all()
    cb = centre_of(both, first, count)
    b = Skin(both, first, count, idx, w, 4)
    bones_b = np.stack([xform(rot_y(0.7), about=cb), xform(np.diag([1.0, -0.5, 1.0]), (0.0, 0.1, 0.0), about=cb),
                        xform(np.diag([1.3, 1.0, 0.8]), (0.05, 0.0, 0.0), about=cb), xform(np.eye(3), (0.0, 0.0, -0.1))])
    first, count, nbones = n - 30, 30, 300
    idx = rng.integers(0, nbones, (3 * count, 4)).astype(np.uint16)
    idx[::7, 0] = 299
    assert (idx > 255).sum() > 20 and idx.max() == 299
    t = rng.uniform(0.05, 0.95, 3 * count).astype(F32)
    w = np.zeros((3 * count, 4), F32)
    w[:, 0], w[:, 2] = t, F32(1) - t
    cc = centre_of(both, first, count)
    c = Skin(both, first, count, idx, w, nbones)
    bones_c = np.stack([xform(rot_y(x), off, about=cc)
                        for x, off in zip(rng.uniform(-0.5, 0.5, nbones), rng.uniform(-0.05, 0.05, (nbones, 3)))])
    return [(a, bones_a), (b, bones_b), (c, bones_c)]


@pytest.mark.parametrize("n_lon,n_lat", [(10, 8), (40, 30)])      # 166: one LDS stage; 2346: HBM records, tile masks
@pytest.mark.parametrize("flags", [0, abi.RT_FLAG_NO_TILE_BINS])
@pytest.mark.parametrize("pose_flags", [0, abi.RT_UPDATE_DEVICE_TILES, abi.RT_UPDATE_REORDER])
def test_mesh_skins(n_lon, n_lat, flags, pose_flags, scene, oracle, tmp_path):
    both, nf = su._mesh_scene(scene, tmp_path, n_lon, n_lat)
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3, flags=flags)
    for skin, bones in _layouts(both, nf):
        want = skin.skinned(bones)
        tr = rt.RayTracer(cfg, both)
        su._frame(tr, cfg, VIEWS[0])                       # the context has a previous frame
        skin.set(tr)
        tr.pose_skin(bones, **FLAG_KW[pose_flags])
        su._check(tr, cfg, want, oracle, VIEWS[:1])
        ref = rt.RayTracer(cfg, both)
        ref.update_scene(want, **FLAG_KW[pose_flags])
        (o1, t1), (o2, t2) = tr.tile_data(), ref.tile_data()
        assert np.array_equal(o1, o2) and np.array_equal(t1.view(np.uint32), t2.view(np.uint32))
        ref.close()
        tr.close()


@pytest.mark.parametrize("n_lon,n_lat", [(10, 8), (40, 30)])
@pytest.mark.parametrize("pose_flags", [0, abi.RT_UPDATE_DEVICE_TILES])
def test_skinned_values_are_the_hosts(n_lon, n_lat, pose_flags, scene, tmp_path):
    """Value by value, not through pixels: the scene the device skinned is Scene.skinned (rt_scene_skin), every vertex and
    every normal of every triangle bit for bit; the colours and the triangles outside the range are the rest scene's."""
    both, nf = su._mesh_scene(scene, tmp_path, n_lon, n_lat)
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    rest = both.packed()
    n = len(both)
    for skin, bones in _layouts(both, nf):
        want = skin.skinned(bones).packed()
        tr = rt.RayTracer(cfg, both)
        skin.set(tr)
        tr.pose_skin(bones, **FLAG_KW[pose_flags])
        d = tr.scene_data()
        assert np.array_equal(_u32(d["vertices"]), _u32(want[0]))
        assert np.array_equal(_u32(d["normals"]), _u32(want[1]))
        assert np.array_equal(_u32(d["colors"]), _u32(rest[2]))
        inside = np.zeros(n, bool)
        inside[skin.first:skin.first + skin.count] = True
        assert not np.array_equal(_u32(d["vertices"]).reshape(n, 12)[inside], _u32(rest[0]).reshape(n, 12)[inside])
        assert np.array_equal(_u32(d["normals"])[~inside], _u32(rest[1])[~inside])
        assert np.array_equal(_u32(d["vertices"]).reshape(n, 12)[~inside], _u32(rest[0]).reshape(n, 12)[~inside])
        tr.close()


@pytest.fixture(scope="module")
def small(scene, tmp_path_factory):
    """Box + the 140-triangle sphere, its mesh skinned to two bones by height."""
    both, nf = su._mesh_scene(scene, tmp_path_factory.mktemp("skin"), 10, 8)
    return both, Skin(both, 26, nf, *by_height(both, 26, nf), 2), centre_of(both, 26, nf)


def _bend(centre, angle):
    return np.stack([sp.IDENT, xform(rot_y(angle), about=centre)])


def test_no_drift(small):
    both, skin, cm = small
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    a, b = rt.RayTracer(cfg, both), rt.RayTracer(cfg, both)
    skin.set(a)
    skin.set(b)
    for k in range(40):
        a.pose_skin(_bend(cm, 0.1 * k))
    a.pose_skin(_bend(cm, 0.7))
    b.pose_skin(_bend(cm, 0.7))
    for view in VIEWS:
        assert _same(su._frame(a, cfg, view), su._frame(b, cfg, view))
    (o1, t1), (o2, t2) = a.tile_data(), b.tile_data()
    assert np.array_equal(o1, o2) and np.array_equal(t1.view(np.uint32), t2.view(np.uint32))
    a.close(); b.close()


@pytest.mark.parametrize("device_tiles", [False, True])
def test_device_entry_ordering(device_tiles, small, oracle):
    import torch
    both, skin, cm = small
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    bones = _bend(cm, 0.5)
    host = rt.RayTracer(cfg, both)
    skin.set(host)
    host.pose_skin(bones, device_tiles=device_tiles)
    want = su._frame(host, cfg, VIEWS[0])
    host.close()
    tr = rt.RayTracer(cfg, both)
    skin.set(tr)
    d_bones = torch.from_numpy(bones).cuda()
    out = (torch.zeros((48, 64), dtype=torch.int32, device="cuda"), torch.zeros((48, 64, 4), device="cuda"))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    tr.pose_skin_device(d_bones, stream=s1, device_tiles=device_tiles)
    su._render_dev(tr, cfg, VIEWS[0], out, s2)             # another stream, no host synchronisation in between
    s1.synchronize()
    d_bones.fill_(float("nan"))                            # the stream has passed the pose: the source may change
    s2.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), want[0])
    assert np.array_equal(out[1].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert su._same_as_oracle(out, su._oracle_frame(oracle, cfg, skin.skinned(bones), VIEWS[0]))
    tr.close()


def test_the_other_calls_see_the_skin(small):
    both, skin, cm = small
    cfg = abi.make_config(width=48, height=32, shadow_samples=4)
    bones = np.stack([xform(np.eye(3), (0.0, 0.0, -0.1)), xform(rot_y(0.6), (0.1, 0.0, -0.2), about=cm)])
    skinned = skin.skinned(bones)
    tr, fresh = rt.RayTracer(cfg, both), rt.RayTracer(cfg, skinned)
    skin.set(tr)
    tr.pose_skin(bones)
    rng = np.random.default_rng(11)
    start = rng.uniform(-0.9, 0.9, size=(2000, 3)).astype(F32)
    d = rng.normal(size=(2000, 3)).astype(F32)
    d[:700] = skinned.aos[26:, :3, :3].reshape(-1, 3).mean(axis=0) - start[:700]     # a third of the rays at the bent mesh
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
    both, skin, cm = small
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    tr = rt.RayTracer(cfg, both)
    skin.set(tr)
    tr.pose_skin(_bend(cm, 0.3))
    want = su._frame(tr, cfg, VIEWS[0])
    nan = _bend(cm, 0.2); nan[0, 1, 2] = np.nan
    far = _bend(cm, 0.2); far[1, 0, 3] = 2.0 ** 17             # bone 1 weighs up to 1: the upper vertices go beyond 2^16
    assert (skin.w[:, 1] > 0.5).any()
    for bad in (nan, far):
        with pytest.raises(rt.RtError) as e:
            tr.pose_skin(bad, **FLAG_KW[pose_flags])
        assert e.value.code == abi.RT_E_INVALID
        d_bad = torch.from_numpy(bad).cuda()
        torch.cuda.synchronize()
        with pytest.raises(rt.RtError) as e:
            tr.pose_skin_device(d_bad, **FLAG_KW[pose_flags])
        assert e.value.code == abi.RT_E_INVALID
        assert tr.skin_info() == (skin.first, skin.count, 2)
        assert _same(su._frame(tr, cfg, VIEWS[0]), want)
    ok = _bend(cm, -0.4)
    tr.pose_skin(ok, **FLAG_KW[pose_flags])                    # from the rest pose, not from the pose of 0.3
    su._check(tr, cfg, skin.skinned(ok), oracle, VIEWS[:1])
    tr.close()


def _no_skin(tr):
    two = np.ascontiguousarray(np.stack([sp.IDENT, sp.IDENT]))
    assert rt.lib().rt_pose_skin(tr._h, rt._fp(two), 0) == abi.RT_E_INVALID
    assert "no skin" in rt.lib().rt_last_error().decode()
    assert tr.skin_info() == (0, 0, 0) and tr.skin is None


def _no_table(tr):
    assert rt.lib().rt_pose_objects(tr._h, rt._fp(np.ascontiguousarray(sp.IDENT)), 0) == abi.RT_E_INVALID
    assert "no object table" in rt.lib().rt_last_error().decode()
    assert tr.object_count() == 0 and tr.objects is None


def test_lifetime_of_the_skin(small, scene, oracle):
    both, skin, cm = small
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    box_skin = Skin(scene, *TALL_BLOCK, *by_height(scene, *TALL_BLOCK), 2)
    ct = centre_of(scene, *TALL_BLOCK)
    tr = rt.RayTracer(cfg, scene)                               # 26 triangles
    _no_skin(tr)                                                # before the first rt_set_skin
    box_skin.set(tr)
    tr.pose_skin(_bend(ct, 0.2))
    tr.update_spheres(abi.REFERENCE_SPHERES[:1])                # the spheres do not touch the skin
    assert tr.skin_info() == (18, 8, 2)
    tr.update_scene(scene)
    _no_skin(tr)
    box_skin.set(tr)
    tr.replace_scene(both)                                      # across n = 64
    _no_skin(tr)
    # a skin again, on the new scene; the objects and the skin displace each other
    tr.set_objects([(26, skin.count)])
    skin.set(tr)
    _no_table(tr)
    bones = _bend(cm, 0.9)
    tr.pose_skin(bones)
    cfg1 = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3, spheres=abi.REFERENCE_SPHERES[:1])
    su._check(tr, cfg1, skin.skinned(bones), oracle, VIEWS[:1])
    tr.set_objects([])                                          # dropping no objects leaves the skin alone
    assert tr.skin_info() == (26, skin.count, 2)
    # bad tables leave the old one in force
    n = len(both)
    bad_idx = skin.idx.copy(); bad_idx[-1, 3] = 2
    bad_w = skin.w.copy(); bad_w[5, 1] = np.nan
    for args in ((26, skin.count, bad_idx, skin.w, 2), (26, skin.count, skin.idx, bad_w, 2), (26, skin.count, skin.idx, skin.w, 0),
                 (n - skin.count + 1, skin.count, skin.idx, skin.w, 2), (-1, skin.count, skin.idx, skin.w, 2),
                 (n, skin.count, skin.idx, skin.w, 2)):
        with pytest.raises(rt.RtError) as e:
            tr.set_skin(*args)
        assert e.value.code == abi.RT_E_INVALID
        assert tr.skin_info() == (26, skin.count, 2)
    bones = _bend(cm, -0.5)
    tr.pose_skin(bones)                                         # still the rest pose and the table of the last good call
    su._check(tr, cfg1, skin.skinned(bones), oracle, VIEWS[:1])
    # the objects displace the skin; the rest pose is snapshot again: the scene as bent
    bent = skin.skinned(bones)
    tr.set_objects([(26, skin.count)])
    _no_skin(tr)
    assert tr.object_count() == 1
    with pytest.raises(rt.RtError):                             # a bad skin leaves the objects in force too
        tr.set_skin(26, skin.count, bad_idx, skin.w, 2)
    assert tr.object_count() == 1
    turn = np.stack([xform(rot_y(0.3), about=cm)])
    tr.pose_objects(turn)
    su._check(tr, cfg1, bent.posed([(26, skin.count)], turn), oracle, VIEWS[:1])
    skin.set(tr)
    tr.set_skin(0, 0, None, None, 0)                            # count == 0 drops the skin
    _no_skin(tr)
    _no_table(tr)
    tr.close()


def test_multi_device_context(small):
    import torch
    both, skin, cm = small
    kw = dict(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    cfg = abi.make_config(**kw)
    multi = rt.RayTracer(abi.make_config(devices=(0, 0), device_band_rows=8, **kw), both)
    single = rt.RayTracer(cfg, both)
    for tr in (multi, single):
        skin.set(tr)
        tr.pose_skin(_bend(cm, 0.35))
    for view in VIEWS:
        assert _same(su._frame(multi, cfg, view), su._frame(single, cfg, view))
    bones = _bend(cm, -0.6)
    d_bones = torch.from_numpy(bones).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    multi.pose_skin_device(d_bones, stream=stream, device_tiles=True)
    single.pose_skin(bones, device_tiles=True)
    stream.synchronize()
    for view in VIEWS:
        assert _same(su._frame(multi, cfg, view), su._frame(single, cfg, view))
    with pytest.raises(rt.RtError):
        bad = bones.copy(); bad[1, 2, 3] = np.inf
        multi.pose_skin(bad)
    assert _same(su._frame(multi, cfg, VIEWS[0]), su._frame(single, cfg, VIEWS[0]))
    multi.close(); single.close()
