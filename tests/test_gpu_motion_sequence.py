"""-m gpu: render_accumulated_light(moving=True) end to end, at 64 x 48, one sample per pixel, 4 shadow samples, a wide light
(the accumulate test's setting).  The tall block of the Cornell box is an object and turns about the vertical axis through its
centre by a fixed step per frame, seen from above so that its top face — which turns inside its own plane — is in view.
Frame by frame the device gives the bits of the restatement in tests/motion_util.py fed with the device's own AOV planes and
scene_data() read-backs: mean, variance, count and both families' counters.  The pixels that keep showing the same triangle of
the block find their history; without the motion planes (moving=False, a second context, the same sequence) fewer do, and
what they find is the record at the place where the point is now; the static walls have identical bits in both modes."""
import numpy as np
import pytest

import motion_util as mu
import test_gpu_scene_pose as sp
from conftest import DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu
F32 = np.float32
LIGHT_SPREAD = 0.3
FRAMES = 6
STEP = 0.1                             # radians per frame: the block's corners move about half a pixel's footprint
CAM, PITCH = [0.0, -1.0, -3.0], -0.3   # from the height of the ceiling, looking down: the top of the tall block is in view
BLOCK = range(sp.TALL_BLOCK[0], sp.TALL_BLOCK[0] + sp.TALL_BLOCK[1])
PLANE_EPS = 0.01                       # rt_accumulate_params_default


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(scene, moving):
    """The sequence on a fresh context -> per frame: (AOV planes, scene_data, parts, accumulate stats, motion stats or None)."""
    import torch
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=4, light_spread=LIGHT_SPREAD)
    tr = rt.RayTracer(cfg, scene)
    rot, focal = rt.rotation_matrix(0.0, PITCH), focal_for(cfg)
    ct = sp.centre_of(scene, *sp.TALL_BLOCK)
    frames = []
    try:
        tr.set_objects([sp.TALL_BLOCK])
        for k in range(FRAMES):
            if k:
                tr.pose_objects(sp.xform(sp.rot_y(k * STEP), about=ct)[None])
            data = tr.scene_data()
            planes = tr.render_aov(rot, CAM, focal, planes=("prim", "position", "normal"))
            parts = tr.render_accumulated_light(rot, CAM, DEFAULT_LIGHT, focal, want_parts=True, moving=moving)
            torch.cuda.synchronize()
            parts = [t.cpu().numpy().copy() for t in parts]
            frames.append((planes, data, parts, tr.accumulate_stats(), tr.motion_stats() if moving and k else None))
            assert tr.motion_info() == (len(scene) if moving else 0)
        tr.reset_history()
        assert tr.motion_info() == 0                          # reset_history releases the snapshot too
    finally:
        tr.close()
    return (rot, focal), frames


@pytest.fixture(scope="module")
def sequences(scene):
    return _run(scene, True), _run(scene, False)


def _restate(view, frames, moving):
    """The restatement over the sequence -> per frame: (next, mean, var, accumulate stats, motion stats, reproj planes, accepted)."""
    rot, focal = view
    kw = dict(prev_rot=rot, prev_cam=np.array(CAM, F32), prev_focal_px=F32(focal))
    prev, out = None, []
    for k, (planes, data, parts, _, _) in enumerate(frames):
        pos, nrm, prim, vis = planes["position"], planes["normal"], planes["prim"], parts[2]
        rp = rn = mstats = None
        if moving and k:
            then = frames[k - 1][1]
            rp, rn, mstats = mu.motion(data["vertices"], then["vertices"], then["normals"], prim, pos, nrm)
        accepted = []
        nxt, mean, var, stats, _ = mu.accumulate_moving(vis, pos, nrm, prim, rp, rn, prev, accepted=accepted, **kw)
        out.append((nxt, mean, var, stats, mstats, (rp, rn), accepted))
        prev = nxt
    return out


def _same_triangle_of_the_block(frames, k):
    """S of frame k: the pixels that show a triangle of the block which they also showed in frame k - 1."""
    prim, before = frames[k][0]["prim"], frames[k - 1][0]["prim"]
    return (prim >= BLOCK[0]) & (prim <= BLOCK[-1]) & (prim == before)


def test_moving_sequence_is_the_restatement_and_finds_the_blocks_history(sequences):
    (view, frames), _ = sequences
    want = _restate(view, frames, True)
    top = set()
    s_total = s_found = 0
    for k, ((planes, data, parts, astats, mstats), (nxt, mean, var, stats, mwant, (rp, rn), accepted)) in enumerate(zip(frames, want)):
        out, term, vis, vis_m, dvar, count = parts
        assert np.array_equal(_u32(vis_m), _u32(mean)), "frame %d: mean" % k
        assert np.array_equal(_u32(dvar), _u32(var)), "frame %d: variance" % k
        assert np.array_equal(_u32(count), _u32(nxt[..., mu.COUNT])), "frame %d: count" % k
        assert {key: astats[key] for key in stats} == stats, "frame %d: accumulate counters" % k
        if not k:
            continue
        assert {key: mstats[key] for key in mwant} == mwant, "frame %d: motion counters" % k
        assert mwant["moved"] > 100 and mwant["unmoved"] > 1000
        s = _same_triangle_of_the_block(frames, k)
        found = nxt[..., mu.COUNT] > 1
        print("frame %d: S holds %d pixels, %d found history; motion %s" % (k, s.sum(), (s & found).sum(), mwant))
        s_total, s_found = s_total + int(s.sum()), s_found + int((s & found).sum())
        # what was accepted on S lies on the record's plane: the carried point P', the snapshot's normal
        prev = want[k - 1][0]
        for cy, cx, acc, _ in accepted:
            r = prev[cy, cx]
            e = r[..., 0:3].astype(np.float64) - rp[..., 0:3]
            pd = np.abs((rn[..., 0:3] * e).sum(-1))
            nd = (rn[..., 0:3].astype(np.float64) * r[..., 4:7]).sum(-1)
            on = s & acc
            assert (pd[on] <= PLANE_EPS + 1e-6).all() and (nd[on] >= 0.9 - 1e-6).all()      # (float64 here, FP32 there)
        # the top face: its normal is the vertical, and it is in view
        nrm = planes["normal"]
        top |= set(np.unique(planes["prim"][s & (np.abs(nrm[..., 1]) > 0.99)]).tolist())
    print("S over the sequence: %d pixels, %d found history (moving=True)" % (s_total, s_found))
    assert s_total >= 100 and 2 * s_found > s_total
    assert top, "the top face of the block is not in view"


def test_without_motion_planes_the_block_loses_or_misplaces_its_history_and_the_walls_do_not_care(sequences):
    (view, frames), (view_s, static) = sequences
    want, want_s = _restate(view, frames, True), _restate(view_s, static, False)
    s_total = found_m = found_s = 0
    dist_m, dist_s = [], []
    for k in range(FRAMES):
        planes, planes_s = frames[k][0], static[k][0]
        for name in ("prim", "position", "normal"):            # the same sequence: the same views of the same scenes
            assert np.array_equal(_u32(planes[name]), _u32(planes_s[name]))
        prim = planes["prim"]
        parts, parts_s = frames[k][2], static[k][2]
        assert np.array_equal(_u32(parts[2]), _u32(parts_s[2]))                     # and the same samples of the visibility
        # moving=False is the plain call: the restatement without reprojection planes
        assert np.array_equal(_u32(parts_s[3]), _u32(want_s[k][1])) and np.array_equal(_u32(parts_s[5]), _u32(want_s[k][0][..., mu.COUNT]))
        walls = (prim < BLOCK[0]) | (prim > BLOCK[-1])          # the static triangles, the spheres, the misses
        for a, b in zip(parts, parts_s):
            assert np.array_equal(_u32(a)[walls], _u32(b)[walls]), "frame %d: a static pixel differs between the modes" % k
        if not k:
            continue
        s = _same_triangle_of_the_block(frames, k)
        s_total += int(s.sum())
        found_m += int((s & (want[k][0][..., mu.COUNT] > 1)).sum())
        found_s += int((s & (want_s[k][0][..., mu.COUNT] > 1)).sum())
        # on the top face, which turns inside its own plane: the history a pixel blends — the records it accepted, by their
        # weights — against the place P' where its own surface point was
        rp = want[k][5][0]
        top = s & (np.abs(planes["normal"][..., 1]) > 0.99)
        for w, dist in ((want, dist_m), (want_s, dist_s)):
            prev = w[k - 1][0]
            centre, weight = np.zeros(prim.shape + (3,)), np.zeros(prim.shape)
            for cy, cx, acc, wt in w[k][6]:
                centre += np.where(acc, wt, 0)[..., None] * prev[cy, cx][..., 0:3].astype(np.float64)
                weight += np.where(acc, wt, 0)
            on = top & (weight > 0)
            dist.extend(np.linalg.norm(centre[on] / weight[on][:, None] - rp[on][:, 0:3], axis=-1).tolist())
    print("S: %d pixels; found history with motion planes %d, without %d" % (s_total, found_m, found_s))
    print("top face, blended history against P': median distance with motion planes %.5f (%d pixels), without %.5f (%d pixels)"
          % (np.median(dist_m), len(dist_m), np.median(dist_s), len(dist_s)))
    assert found_m > found_s
    assert len(dist_s) >= 20 and len(dist_m) >= len(dist_s)  # the top face keeps finding history in both modes ...
    # ... and without the planes it is that of other surface points: a still camera reprojects a pixel of the face onto itself,
    # so it blends the record of its own place, while its surface point came from STEP * (its distance from the axis) away —
    # about 0.01 for a face 0.4 wide; only a pixel on the axis itself is its own history
    assert np.median(dist_s) > 1e-3
