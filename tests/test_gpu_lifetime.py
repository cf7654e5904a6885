"""-m gpu: a context gives back what it took.  rt_debug_live_device_objects counts the device allocations, their bytes, the
events and the streams that the library's owners hold in this process.  Every test reads the four figures
first and finds exactly them again after close(), whatever the context did in between: every entry that allocates on first
use, a scene that outgrows the capacity, tables that are swapped and dropped, rejected calls, a multi-device handle, two
contexts closed in the order they were made.  Where the project says that nothing is allocated (a replace within the
capacity, a second pose), the figures stand still while the context is alive."""
import gc

import numpy as np
import pytest

import test_gpu_scene_pose as sp
from conftest import focal_for
from test_gpu_scene_skin import by_height
from uob_raytracer_amd import abi, meshgen, runtime as rt

pytestmark = pytest.mark.gpu

VIEW = (0.2, 0.1, [0.1, 0.1, -3.0], [0.1, -0.5, -0.6])
LIGHT = VIEW[3]
F32 = np.float32


def _cfg(**kw):
    return abi.make_config(width=64, height=48, shadow_samples=4, **kw)          # 2x2 AA


def _live():
    gc.collect()                                   # (a context another test forgot must not go in the middle of this one)
    return rt.live_device_objects()


@pytest.fixture(scope="module")
def pool(scene, tmp_path_factory):
    """The Cornell Box followed by a sphere of 390 triangles (tiled copy, no masks): scene_of(pool, n) = its first n."""
    path = str(tmp_path_factory.mktemp("lifetime") / "ball.obj")
    assert meshgen.write_sphere_obj(path, 15, 14) == 390
    return scene + rt.Scene.load_obj(path)


@pytest.fixture(scope="module")
def big(scene, tmp_path_factory):
    """The box and a sphere of 2320 triangles: 2346, beyond the 1024 at which the tile masks and aux_stream appear."""
    path = str(tmp_path_factory.mktemp("lifetime_big") / "ball.obj")
    assert meshgen.write_sphere_obj(path, 40, 30) == 2320
    return scene + rt.Scene.load_obj(path)


def scene_of(sc, n):
    assert n <= len(sc)
    return rt.Scene(sc.aos[:n].copy())


@pytest.fixture(scope="module")
def probes():
    rng = np.random.default_rng(5)
    o = np.array([0.0, 0.0, -2.5], F32) + rng.uniform(-0.2, 0.2, (128, 3)).astype(F32)
    rays = np.ascontiguousarray(np.concatenate([o, rng.uniform(-0.9, 0.9, (128, 3)).astype(F32) - o], 1), F32)
    r2 = rng.uniform(0.5, 9.0, 128).astype(F32)
    pts = rng.uniform(-0.8, 0.8, (64, 3)).astype(F32)
    nrm = rng.normal(size=(64, 3)).astype(F32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(F32)
    return rays, r2, pts, nrm


def _to_device(sc):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in sc.packed()]
    torch.cuda.synchronize()
    return out


def _view(cfg):
    yaw, pitch, cam, light = VIEW
    return rt.rotation_matrix(yaw, pitch), cam, light, focal_for(cfg)


def _frames_and_calls(tr, cfg, probes):
    """Frames to host memory (with and without the float tap, and into a registered buffer), the blocking and the device
    entry of every call beside the frame, the debug tracer and the counting passes."""
    import torch
    rays, r2, pts, nrm = probes
    rot, cam, light, focal = _view(cfg)
    tr.render(rot, cam, light, focal)
    tr.render(rot, cam, light, focal, want_rgb=True)
    fb = np.zeros((tr.rows, tr.width), np.uint32)
    tr.register_output(fb)
    tr.render(rot, cam, light, focal, out=fb)
    assert fb.any()
    tr.unregister_output()
    d_rays, d_r2 = torch.from_numpy(rays).cuda(), torch.from_numpy(r2).cuda()
    tr.query_closest_hit(rays)
    tr.query_in_shadow(rays, r2)
    tr.query_device(abi.RT_TRACE_CLOSEST_HIT, d_rays)
    tr.query_device(abi.RT_TRACE_IN_SHADOW, d_rays, d_r2)
    tr.shade_points(pts, nrm, LIGHT)
    tr.shade_points_device(torch.from_numpy(np.ascontiguousarray(np.concatenate([pts, nrm], 1))).cuda(), LIGHT)
    tr.radiance_rays(rays, LIGHT)
    tr.radiance_rays_device(d_rays, LIGHT)
    tr.render_aov(rot, cam, focal)
    tr.render_aov_device(rot, cam, focal, out={"prim": torch.zeros((tr.rows, tr.width), dtype=torch.int32, device="cuda"),
                                                "normal": torch.zeros((tr.rows, tr.width, 4), device="cuda")})
    torch.cuda.synchronize()
    tr.trace_closest_hit(rays)
    tr.trace_in_shadow(rays, r2)
    tr.count_work(rot, cam, light, focal)
    try:
        tr.count_executed(rot, cam, light, focal)
    except rt.RtError as e:                          # the generic kernel has no counting build of its own
        assert e.code == abi.RT_E_UNSUPPORTED


def _replaces(tr, pool, n_grow, grow_from):
    """Host and device replaces across n = 64 both ways (every kernel family's buffers on first use), with the host's and
    the device's tiles, then one to n_grow triangles"""
    tr.replace_scene(scene_of(pool, 65))
    tr.replace_scene(scene_of(pool, 40))
    tr.replace_scene(scene_of(pool, 300), device_tiles=True)
    tr.replace_scene_device(*_to_device(scene_of(pool, 26)))
    tr.replace_scene_device(*_to_device(scene_of(pool, 129)))                    # the device's tiles
    tr.replace_scene_device(*_to_device(scene_of(pool, 200)), reorder=True)      # without: staged to the host, its tiles
    if n_grow:
        cap = tr.scene_capacity()
        assert n_grow > cap
        tr.replace_scene(scene_of(grow_from, n_grow))                            # the growth path
        assert tr.scene_capacity() >= n_grow > cap


def _bend(scene, first, count, angle):
    ct = sp.centre_of(scene, first, count)
    return np.stack([sp.IDENT, sp.xform(sp.rot_y(angle), about=ct)])


def _poses(tr, sc):
    """An object table and two skins (the second swaps the table) on the last 8 triangles of `sc`, the context's scene;
    each posed through the blocking and the device entry"""
    import torch
    first, count = len(sc) - 8, 8
    turn = np.stack([sp.xform(sp.rot_y(0.3), about=sp.centre_of(sc, first, count))])
    tr.set_objects([(first, count)])
    tr.pose_objects(turn)
    tr.pose_objects_device(torch.from_numpy(turn).cuda(), device_tiles=len(sc) > 64)
    idx, w = by_height(sc, first, count)
    tr.set_skin(first, count, idx, w, 2)
    tr.pose_skin(_bend(sc, first, count, 0.2))
    tr.set_skin(first + 2, count - 2, idx[6:], w[6:], 2)                         # a new table takes the old one's place
    tr.pose_skin(_bend(sc, first, count, -0.2))
    tr.pose_skin_device(torch.from_numpy(_bend(sc, first, count, 0.1)).cuda())
    torch.cuda.synchronize()


# ---- a context that does everything ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["box", "mesh416", "mesh2346", "box_generic"])
def test_a_context_gives_everything_back(which, scene, pool, big, probes):
    sc = {"box": scene, "mesh416": pool, "mesh2346": big, "box_generic": scene}[which]
    cfg = _cfg(flags=abi.RT_FLAG_GENERIC_KERNEL if which == "box_generic" else 0)
    start = _live()
    tr = rt.RayTracer(cfg, sc)
    alive = _live()
    assert alive["allocations"] > start["allocations"] and alive["bytes"] > start["bytes"]
    assert alive["events"] >= start["events"] + 2 and alive["streams"] >= start["streams"] + 1
    if which == "mesh2346":                                                     # the masks are built on a stream of their own
        assert alive["streams"] == start["streams"] + 2
    _frames_and_calls(tr, cfg, probes)
    moved = sc.transformed(list(range(len(sc) - 8, len(sc))), np.eye(3), (0.0, -0.05, 0.0))
    tr.update_scene(moved)
    dv, dn, dc = _to_device(sc)
    tr.update_scene_device(dv.data_ptr(), dn.data_ptr(), dc.data_ptr(), len(sc))
    _poses(tr, sc)
    tr.update_spheres(abi.REFERENCE_SPHERES[:1])
    # beyond the capacity: the pool for the box, 600 of the big mesh for the pool, the big mesh and the pool for the big mesh
    grow = {"box": (len(pool), pool), "mesh416": (600, big), "mesh2346": (len(big) + len(pool), big + pool),
            "box_generic": (len(pool), pool)}[which]
    _replaces(tr, pool, *grow)
    _frames_and_calls(tr, cfg, probes)                                          # on the grown scene: whatever is sized by it
    _poses(tr, tr.scene)                                                        # a table is alive when the context goes
    assert _live()["allocations"] > alive["allocations"]
    tr.close()
    assert _live() == start


# ---- where nothing is allocated, the figures stand still ----------------------------------------------------------------------
def test_a_second_replace_sequence_within_capacity_allocates_nothing(pool):
    start = _live()
    tr = rt.RayTracer(_cfg(), pool)
    _replaces(tr, pool, 0, None)
    once = _live()
    _replaces(tr, pool, 0, None)
    assert _live() == once
    tr.close()
    assert _live() == start


@pytest.mark.parametrize("which", ["box", "mesh416"])
def test_a_second_pose_allocates_nothing(which, scene, pool):
    sc = {"box": scene, "mesh416": pool}[which]
    start = _live()
    tr = rt.RayTracer(_cfg(), sc)
    _poses(tr, sc)
    once = _live()
    _poses(tr, sc)
    assert _live() == once
    tr.close()
    assert _live() == start


# ---- rejected calls -----------------------------------------------------------------------------------------------------------
def test_rejected_calls_take_nothing_and_leave_nothing(pool):
    """Each rejected call follows an accepted one of its kind, so that what the entry makes on first use (the staging scene,
    the check's result block) exists: the rejection itself must neither allocate nor free."""
    import torch
    start = _live()
    tr = rt.RayTracer(_cfg(), pool)
    first, count = len(pool) - 8, 8
    # a pose with a NaN matrix: RT_E_INVALID from the check of the staging scene
    tr.set_objects([(first, count)])
    tr.pose_objects(np.stack([sp.IDENT]))
    before = _live()
    nan = np.stack([sp.IDENT]).copy()
    nan[0, 1, 2] = np.nan
    with pytest.raises(rt.RtError) as e:
        tr.pose_objects(nan)
    assert e.value.code == abi.RT_E_INVALID and _live() == before and tr.object_count() == 1
    # a skin with a bone index that is no bone: the old table stays in force
    idx, w = by_height(pool, first, count)
    tr.set_skin(first, count, idx, w, 2)
    before = _live()
    bad = idx.copy()
    bad[-1, 3] = 2
    with pytest.raises(rt.RtError) as e:
        tr.set_skin(first, count, bad, w, 2)
    assert e.value.code == abi.RT_E_INVALID and _live() == before and tr.skin_info() == (first, count, 2)
    # a device replace with a vertex beyond 2^16: found by the check pass, the scene stays
    tr.replace_scene_device(*_to_device(scene_of(pool, 300)))
    before = _live()
    v, nr, c = scene_of(pool, 200).packed()
    v = v.copy()
    v[17, 0] = 2.0 ** 17
    dv, dn, dc = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (v, nr, c))
    torch.cuda.synchronize()
    with pytest.raises(rt.RtError) as e:
        tr.replace_scene_device(dv, dn, dc)
    assert e.value.code == abi.RT_E_INVALID and _live() == before and tr.n_triangles == 300
    tr.close()
    assert _live() == start


# ---- several devices, several contexts -----------------------------------------------------------------------------------------
def test_a_multi_device_handle_on_one_gpu(pool):
    import torch
    cfg = _cfg(devices=(0, 0), device_band_rows=8)
    start = _live()
    tr = rt.RayTracer(cfg, scene_of(pool, 26))
    rot, cam, light, focal = _view(cfg)
    tr.render(rot, cam, light, focal, want_rgb=True)
    d_argb = torch.zeros((cfg.height, cfg.width), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tr.render_device(rot, cam, light, focal, d_argb.data_ptr())
    torch.cuda.synchronize()
    assert d_argb.any()
    sc = scene_of(pool, 300)
    tr.replace_scene(sc)                                                        # grows, on both children
    assert tr.scene_capacity() >= 300
    tr.set_objects([(292, 8)])
    tr.pose_objects(np.stack([sp.xform(sp.rot_y(0.3), about=sp.centre_of(sc, 292, 8))]))
    tr.render(rot, cam, light, focal)
    assert _live()["streams"] == start["streams"] + 3                           # the handle's and one per child
    tr.close()
    assert _live() == start


def test_two_contexts_closed_in_the_order_they_were_made(scene, pool):
    cfg = _cfg()
    start = _live()
    a = rt.RayTracer(cfg, scene)
    only_a = _live()
    b = rt.RayTracer(cfg, pool)
    rot, cam, light, focal = _view(cfg)
    one, two = a.render(rot, cam, light, focal), b.render(rot, cam, light, focal)
    assert not np.array_equal(one, two)
    both = _live()
    a.close()                                                                   # the first made goes first
    after_a = _live()
    assert {k: both[k] - after_a[k] for k in both} == {k: only_a[k] - start[k] for k in both}
    assert np.array_equal(b.render(rot, cam, light, focal), two)                # b is whole
    b.close()
    assert _live() == start
