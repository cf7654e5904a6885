"""-m gpu: the motion planes on the device (rt_motion_snapshot, rt_motion_planes / rt_motion_planes_device, rt_motion.hip) give
the bits of the numpy restatement in tests/motion_util.py through both entries, with the restatement's counts as counters — on
the box with its two blocks posed as objects and on a mesh context posed by a skin, where a tiled copy of the scene exists
beside the original order the snapshot keeps; the moving accumulate (rt_accumulate_plane_moving*) gives the restatement's bits
and counters and, without reprojection planes, the plain entry's; a snapshot of another triangle count is refused; the snapshot
goes with rt_motion_release and with the context; a device pose on another stream waits for the snapshot — observed behind a
gate; and a multi-device context answers on its first device."""
import numpy as np
import pytest

import accumulate_util as au
import motion_util as mu
import ordering_util as ou
import test_gpu_scene_pose as sp
import test_gpu_scene_skin as sk
import test_gpu_scene_update as su
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu
F32 = np.float32
KW = dict(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=2)
RANGES = [sp.SHORT_BLOCK, sp.TALL_BLOCK]
SHAPES = [(1,), (63,), (64,), (65,), (257,), (37, 100)]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _box_pose(box, k=0):
    cs, ct = sp.centre_of(box, *sp.SHORT_BLOCK), sp.centre_of(box, *sp.TALL_BLOCK)
    poses = [np.stack([sp.xform(sp.rot_y(0.3), (0.1, 0.0, -0.05), about=cs), sp.xform(sp.rot_y(-0.3), (-0.05, 0.0, 0.1), about=ct)]),
             np.stack([sp.xform(sp.rot_y(-0.2), (0.0, 0.0, 0.1), about=cs), sp.xform(sp.rot_y(0.7), about=ct)])]
    return poses[k]


class Moved:
    """A context whose scene moved after its snapshot, with both scenes read back in original order."""

    def __init__(self, tr, pose):
        import torch
        self.tr = tr
        self.then = tr.scene_data()
        tr.motion_snapshot()
        pose()
        torch.cuda.synchronize()
        self.now = tr.scene_data()
        self.n = self.now["normals"].shape[0]
        assert tr.motion_info() == self.n
        assert not np.array_equal(_u32(self.now["vertices"]), _u32(self.then["vertices"]))

    def case(self, shape):
        """Spoiled elements on the live triangles in `shape`, and the restatement's answer."""
        count = int(np.prod(shape))
        prim, pos, nrm = mu.elements_on(self.now["vertices"], count, 40 + count)
        prim, pos, nrm = prim.reshape(shape), pos.reshape(shape + (4,)), nrm.reshape(shape + (4,))
        want = mu.motion(self.now["vertices"], self.then["vertices"], self.then["normals"], prim, pos, nrm)
        return (prim, pos, nrm), want


@pytest.fixture(scope="module")
def box_moved(scene):
    import torch
    tr = rt.RayTracer(abi.make_config(**KW), scene)
    tr.set_objects(RANGES)
    x = torch.from_numpy(_box_pose(scene)).cuda()
    yield Moved(tr, lambda: tr.pose_objects_device(x))
    tr.close()


@pytest.fixture(scope="module")
def mesh_moved(scene, tmp_path_factory):
    """Box + a 140-triangle sphere skinned to two bones: n > 64, so the context also keeps a tiled copy in another order."""
    import torch
    both, nf = su._mesh_scene(scene, tmp_path_factory.mktemp("motion"), 10, 8)
    assert len(both) > 64
    tr = rt.RayTracer(abi.make_config(**KW), both)
    skin, cm = sk.Skin(both, 26, nf, *sk.by_height(both, 26, nf), 2), sp.centre_of(both, 26, nf)
    skin.set(tr)
    bones = torch.from_numpy(np.stack([sp.IDENT, sp.xform(sp.rot_y(0.5), (0.15, -0.1, -0.1), about=cm)])).cuda()
    m = Moved(tr, lambda: tr.pose_skin_device(bones))
    data = tr.scene_data(tiled=True)
    assert not np.array_equal(_u32(data["vertices_m"]), _u32(data["vertices"]))      # the tiled copy is in another order
    yield m
    tr.close()


def _stats_equal(tr, stats):
    st = tr.motion_stats()
    assert {k: st[k] for k in stats} == stats
    assert st["reserved6"] == st["reserved7"] == 0


def _check_both_entries(m, shape):
    import torch
    (prim, pos, nrm), (want_p, want_n, stats) = m.case(shape)
    got_p, got_n = m.tr.motion_planes(prim, pos, nrm)
    assert got_p.shape == pos.shape
    assert np.array_equal(_u32(got_p), _u32(want_p)) and np.array_equal(_u32(got_n), _u32(want_n))
    _stats_equal(m.tr, stats)
    d = [torch.from_numpy(a.copy()).cuda() for a in (prim, pos, nrm)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out_p, out_n = m.tr.motion_planes_device(*d, stream=side)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out_p), _u32(want_p)) and np.array_equal(_bits(out_n), _u32(want_n))
    _stats_equal(m.tr, stats)
    return stats


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_box_objects_equal_the_restatement(box_moved, shape):
    stats = _check_both_entries(box_moved, shape)
    if shape == (37, 100):                                   # the 16 triangles of the blocks moved, the 10 of the walls did not
        assert stats["moved"] > 1000 and stats["unmoved"] > 500 and stats["copied"] > 100 and stats["prim_out_of_range"] > 50


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_skinned_mesh_equals_the_restatement(mesh_moved, shape):
    stats = _check_both_entries(mesh_moved, shape)
    if shape == (37, 100):
        assert stats["moved"] > 1000 and stats["unmoved"] > 100


def test_a_grid_that_continues_in_a_second_dimension(scene, monkeypatch):
    """UOB_RT_MOTION_BLOCKS_X = 2: the 15 workgroups of 3 700 elements lie in grid.y rows of two, the last row half empty."""
    import torch
    monkeypatch.setenv("UOB_RT_MOTION_BLOCKS_X", "2")
    tr = rt.RayTracer(abi.make_config(**KW), scene)
    monkeypatch.delenv("UOB_RT_MOTION_BLOCKS_X")
    try:
        tr.set_objects(RANGES)
        m = Moved(tr, lambda: tr.pose_objects(_box_pose(scene)))
        _check_both_entries(m, (37, 100))
        _check_both_entries(m, (513,))
    finally:
        tr.close()


def test_an_unmoved_context_returns_its_inputs(box_moved, scene):
    tr = box_moved.tr
    tr.motion_snapshot()                                     # of the posed scene: now nothing has moved since
    try:
        prim, pos, nrm = mu.elements_on(box_moved.now["vertices"], 3700, 8, spoil=False)
        got_p, got_n = tr.motion_planes(prim, pos, nrm)
        assert np.array_equal(_u32(got_p), _u32(pos)) and np.array_equal(_u32(got_n), _u32(nrm))
        st = tr.motion_stats()
        assert st["unmoved"] == 3700 == st["valid_elements"] and st["moved"] == 0
    finally:                                                 # the module's snapshot again: the scene before the pose
        import torch
        tr.pose_objects(np.stack([sp.IDENT, sp.IDENT]))
        box_moved.then = tr.scene_data()
        tr.motion_snapshot()
        tr.pose_objects(_box_pose(scene))
        torch.cuda.synchronize()
        box_moved.now = tr.scene_data()
    _check_both_entries(box_moved, (257,))


# ---- the moving accumulate ----------------------------------------------------------------------------------------------
def _acc_stats_equal(tr, stats):
    st = tr.accumulate_stats()
    assert {k: st[k] for k in stats} == stats
    assert st["reserved5"] == st["reserved6"] == st["reserved7"] == 0


_MOVING_REF = {}


def _moving_reference(h, w, param_set):
    key = (h, w, param_set)
    if key not in _MOVING_REF:
        planes, kw = au.call_args(h, w, param_set)
        rpos, rnrm = mu.moving_planes(h, w)
        nxt, mean, var, stats, _ = mu.accumulate_moving(*planes[:4], rpos, rnrm, planes[4], prev_focal_px=F32(w), **kw)
        _MOVING_REF[key] = (planes, kw, rpos, rnrm, _u32(nxt), _u32(mean), _u32(var), stats)
    return _MOVING_REF[key]


@pytest.mark.parametrize("param_set", ["defaults", "no_prim", "no_prev", "max_history_4"])
@pytest.mark.parametrize("size", au.SIZES + au.TILE_SIZES, ids=lambda s: "%dx%d" % s)
def test_moving_accumulate_equals_the_restatement(box_moved, size, param_set):
    import torch
    tr = box_moved.tr
    h, w = size
    planes, kw, rpos, rnrm, want_next, want_mean, want_var, stats = _moving_reference(h, w, param_set)
    nxt, mean, var = tr.accumulate_plane(*planes, reproj_position4=rpos, reproj_normal4=rnrm, prev_focal=w, **kw)
    assert np.array_equal(_u32(nxt), want_next) and np.array_equal(_u32(mean), want_mean) and np.array_equal(_u32(var), want_var)
    _acc_stats_equal(tr, stats)
    d = [torch.from_numpy(a.copy()).cuda() if a is not None else None for a in planes + (rpos, rnrm)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for want_m, want_v in ((True, True), (False, True), (True, False), (False, False)):
        got = tr.accumulate_plane_device(d[0], d[1], d[2], prim=d[3], prev=d[4], reproj_position4=d[5], reproj_normal4=d[6], stream=side,
                                         want_mean=want_m, want_variance=want_v, prev_focal=w, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got[0]), want_next)
        assert (got[1] is not None) == want_m and (got[2] is not None) == want_v
        assert got[1] is None or np.array_equal(_bits(got[1]), want_mean)
        assert got[2] is None or np.array_equal(_bits(got[2]), want_var)
        _acc_stats_equal(tr, stats)


@pytest.mark.parametrize("size", [(37, 100), (2 * au.TILE_TY + 1, 2 * au.TILE_TX + 1)], ids=lambda s: "%dx%d" % s)
def test_moving_entry_without_planes_is_the_plain_entry(box_moved, size):
    import ctypes as C
    import torch
    tr = box_moved.tr
    h, w = size
    planes, kw = au.call_args(h, w, "defaults")
    want = au.reference(h, w, "defaults")
    d = [torch.from_numpy(a.copy()).cuda() for a in planes]
    plain = tr.accumulate_plane_device(d[0], d[1], d[2], prim=d[3], prev=d[4], prev_focal=w, **kw)
    torch.cuda.synchronize()
    p = rt.accumulate_params(w, h, prev_focal=w, **kw)
    out = [torch.zeros((h, w, 12), device="cuda"), torch.zeros((h, w), device="cuda"), torch.zeros((h, w), device="cuda")]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    raw = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = rt.lib().rt_accumulate_plane_moving_device(tr._h, C.byref(p), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), None, None, ptr(d[4]),
                                                    ptr(out[0]), ptr(out[1]), ptr(out[2]), raw)
    assert rc == abi.RT_OK
    torch.cuda.synchronize()
    for a, b, ref in zip(out, plain, want[:3]):
        assert np.array_equal(_bits(a), ref) and np.array_equal(_bits(b), ref)
    _acc_stats_equal(tr, want[3])
    # and with the guides themselves as reprojection planes, through the kernel that reads them
    same = tr.accumulate_plane_device(d[0], d[1], d[2], prim=d[3], prev=d[4], reproj_position4=d[1], reproj_normal4=d[2], prev_focal=w, **kw)
    torch.cuda.synchronize()
    for a, ref in zip(same, want[:3]):
        assert np.array_equal(_bits(a), ref)


# ---- refusals and lifetime ----------------------------------------------------------------------------------------------
def test_refusals_and_the_snapshots_lifetime(scene):
    import torch
    torch.cuda.synchronize()
    before = rt.live_device_objects()
    tr = rt.RayTracer(abi.make_config(**KW), scene)
    n = len(scene)
    prim, pos, nrm = mu.elements_on(scene.packed()[0], 257, 3, spoil=False)
    with_ctx = rt.live_device_objects()
    tr.motion_snapshot()
    torch.cuda.synchronize()
    taken = rt.live_device_objects()
    assert tr.motion_info() == n
    # the two snapshot buffers, the family's counters and its event
    assert taken["allocations"] == with_ctx["allocations"] + 3 and taken["events"] == with_ctx["events"] + 1
    assert taken["bytes"] - with_ctx["bytes"] == 4 * n * 16 + _stats_bytes()
    tr.motion_planes(prim, pos, nrm)
    staged = rt.live_device_objects()
    # a replace to another count leaves a snapshot that no longer matches: refused until the next one
    smaller = rt.Scene(scene.aos[:n - 2].copy())
    tr.replace_scene(smaller)
    prim2 = np.minimum(prim, n - 3).astype(np.int32)
    for call in (lambda: tr.motion_planes(prim2, pos, nrm),
                 lambda: tr.motion_planes_device(*(torch.from_numpy(a).cuda() for a in (prim2, pos, nrm)))):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == abi.RT_E_INVALID and "%d triangles" % n in str(e.value) and "%d" % (n - 2) in str(e.value)
    assert tr.motion_info() == n
    tr.motion_snapshot()
    assert tr.motion_info() == n - 2
    got_p, got_n = tr.motion_planes(prim2, pos, nrm)
    assert np.array_equal(_u32(got_p), _u32(pos)) and np.array_equal(_u32(got_n), _u32(nrm))      # nothing moved since
    assert rt.live_device_objects()["bytes"] == staged["bytes"]                                   # the buffers only grow
    # release: the snapshot's two buffers go, the rest of the family stays until the context does
    tr.motion_release()
    gone = rt.live_device_objects()
    assert tr.motion_info() == 0
    assert gone["allocations"] == staged["allocations"] - 2 and gone["bytes"] == staged["bytes"] - 4 * n * 16
    with pytest.raises(rt.RtError) as e:
        tr.motion_planes(prim2, pos, nrm)
    assert "no snapshot" in str(e.value)
    tr.motion_snapshot()                                     # and a context closed with a snapshot frees it
    assert tr.motion_info() == n - 2
    tr.close()
    assert rt.live_device_objects() == before


def _stats_bytes():
    """The family's counters (made by the first snapshot, kept by a release): 8 exported words and 64 slots of 16."""
    return (8 + 64 * 16) * 8


# ---- ordering -----------------------------------------------------------------------------------------------------------
def test_a_device_pose_on_another_stream_waits_for_the_snapshot(scene):
    """Stream g: a gate, then the snapshot.  Stream b, no host synchronisation in between: a device pose, then the motion
    planes.  While the gate is closed the snapshot cannot have been taken, so a pose that did not wait for it would overwrite
    the scene first and the snapshot would hold the posed scene.  Observed: the event behind the pose stays unset for as long
    as the gate is closed; and the data: the motion planes are those of "snapshot = the scene before the pose"."""
    import torch
    tr = rt.RayTracer(abi.make_config(**KW), scene)
    try:
        tr.set_objects(RANGES)
        clock = ou.Clock.get()
        argb = torch.zeros((KW["height"], KW["width"]), dtype=torch.int32, device="cuda")
        rot, (_, _, cam, light) = rt.rotation_matrix(0.0, 0.0), su.VIEWS[0]
        from conftest import focal_for
        frame_on = lambda s: tr.render_device(rot, cam, light, focal_for(tr.cfg), argb.data_ptr(), stream=s.cuda_stream)
        g, _, b = ou.pick_streams(clock, frame_on, frame_as_b=False, report=print)
        x = torch.from_numpy(_box_pose(scene)).cuda()
        ident = np.stack([sp.IDENT, sp.IDENT])
        then = tr.scene_data()
        posed = scene.posed(RANGES, _box_pose(scene)).packed()[0]
        prim, pos, nrm = mu.elements_on(posed, 3700, 77)
        d = [torch.from_numpy(a).cuda() for a in (prim, pos, nrm)]
        out = [torch.zeros((3700, 4), device="cuda") for _ in range(2)]

        def sequence(gate_ms):
            tr.pose_objects(ident)
            for t in out:
                t.zero_()
            torch.cuda.synchronize()
            end = clock.gate(g, gate_ms) if gate_ms else None
            tr.motion_snapshot(stream=g)
            tr.pose_objects_device(x, stream=b)
            ev = torch.cuda.Event()
            ev.record(b)
            tr.motion_planes_device(*d, out_position4=out[0], out_normal4=out[1], stream=b)
            closed = end is not None and not end.query()
            result = ou.observe(end, ev, True) if end is not None else None
            torch.cuda.synchronize()
            return ou.VOID if (end is not None and not closed and result is None) else result

        for _ in range(2):                                   # the second round is timed: the first creates events and buffers
            dev_ms, host_ms = ou.device_ms(lambda: sequence(0), torch.cuda.current_stream())
        gate = ou.GATE_FACTOR * max(dev_ms, 0.05) + host_ms
        result = sequence(gate)
        if result == ou.VOID:
            print("void with a gate of %.2f ms, once more with %.2f ms" % (gate, ou.VOID_FACTOR * gate))
            result = sequence(ou.VOID_FACTOR * gate)
        print("pose behind a gated snapshot: gate %.2f ms, %s" % (gate, result or "the pose waited"))
        assert result is None, result
        now = tr.scene_data()
        assert np.array_equal(_u32(now["vertices"]), _u32(posed))
        want_p, want_n, stats = mu.motion(now["vertices"], then["vertices"], then["normals"], prim, pos, nrm)
        assert stats["moved"] > 1000
        assert np.array_equal(_bits(out[0]), _u32(want_p)) and np.array_equal(_bits(out[1]), _u32(want_n))
        _stats_equal(tr, stats)
    finally:
        torch.cuda.synchronize()
        tr.close()


def test_multi_device_context_answers_on_its_first_device(scene):
    import torch
    tr = rt.RayTracer(abi.make_config(devices=(0, 0), device_band_rows=8, **KW), scene)
    try:
        tr.set_objects(RANGES)
        m = Moved(tr, lambda: tr.pose_objects(_box_pose(scene, 1)))
        _check_both_entries(m, (37, 100))
        tr.motion_release()
        assert tr.motion_info() == 0
    finally:
        tr.close()
