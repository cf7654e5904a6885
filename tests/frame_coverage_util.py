"""What tests/test_gpu_frame_coverage.py shares: frames rendered into poisoned device tensors (a pixel no kernel wrote
keeps the poison, on the first frame of a context and on a static view alike), the wave kernel's job count for a forced job
size, and the scenes and views of the sequences.  The checks themselves are numpy (tests/test_frame_coverage_util_cpu.py
runs them without a device)."""
import os

import numpy as np

from uob_raytracer_amd import meshgen, runtime as rt

# ARGB poison: alpha byte 0, which no kernel stores (pack_argb sets alpha 0xFF); tap poison: NaN
SENTINEL = 0x00C0FFEE
BACKGROUND = 0xFF000000
TAP_W = 1.0        # the fourth tap component as stored: make_float4(c.x, c.y, c.z, 1.0f) in rt_kernel_wave.hip, rt_kernel_mesh.hip
#                    and rt_kernel_generic.hip alike


def owned_rows(cfg):
    """The rows of cfg's band partition, as rt_config_owned_rows counts them (rt_api.hip): global row numbers, in order."""
    br, bc = (cfg.band_rows if cfg.band_rows > 0 else cfg.height), max(cfg.band_count, 1)
    return [y for y in range(cfg.height) if (y // br) % bc == cfg.band_index]


def expected_jobs(cfg, job_tasks=None):
    """Jobs of one wave-kernel frame with UOB_RT_JOB_TASKS = job_tasks: ceil(W / job_pixels) * owned rows.  Restated from
    fill_params (rt_api.hip, "wave kernel: a job is a run of job_tasks 64-ray tasks"): a 64-ray task is 64 // aa pixels, a
    job is job_tasks of them within one row; with 65..256 AA samples a job is 16 pixels whatever the knob says.  The knob is
    honoured for certain only while the job stays within 64 pixels and does not fall below 16 (the conditions next to
    `c->tune.job_tasks` there); other values are refused here, not guessed at."""
    aa = cfg.aa_x * cfg.aa_y
    if aa > 64:
        job_pixels = 16
    else:
        pt = 64 // aa
        if job_tasks is None or job_tasks < 1 or not 16 <= job_tasks * pt <= 64:
            raise ValueError("a forced job of %r tasks of %d pixels is not one fill_params honours for certain" % (job_tasks, pt))
        job_pixels = job_tasks * pt
    return -(-cfg.width // job_pixels) * len(owned_rows(cfg))


def check_written(argb, tap=None, expected_tap=None):
    """The assertions of render_checked on host arrays: argb uint32 [rows, W] holds no SENTINEL word; tap float32
    [rows, W, 4] holds no NaN (where expected_tap [rows, W, 3 or 4] is given: none where that has none) and TAP_W in its
    fourth component."""
    argb = np.asarray(argb)
    bad = np.argwhere(argb.view(np.uint32) == np.uint32(SENTINEL))
    assert bad.size == 0, "%d of %d pixels were never written (ARGB sentinel), first at (row, x) = %s" % (len(bad), argb.size, bad[0])
    alpha = argb.view(np.uint32) >> np.uint32(24)
    assert (alpha == 0xFF).all(), "alpha byte other than 0xFF at %s" % (np.argwhere(alpha != 0xFF)[0],)
    if tap is None:
        return
    tap = np.asarray(tap)
    assert tap.shape == argb.shape + (4,)
    nan = np.isnan(tap[..., :3])
    if expected_tap is not None:
        nan &= ~np.isnan(np.asarray(expected_tap).reshape(argb.shape + (-1,))[..., :3])
    bad = np.argwhere(nan)
    assert bad.size == 0, "%d tap components are NaN (unwritten?), first at (row, x, channel) = %s" % (len(bad), bad[0])
    bad = np.argwhere(tap[..., 3].view(np.uint32) != np.float32(TAP_W).view(np.uint32))
    assert bad.size == 0, "%d taps do not hold w = %g, first at (row, x) = %s: %r" % (len(bad), TAP_W, bad[0], tap[tuple(bad[0])])


def render_checked(tr, rot, cam, light, focal, want_tap=True, expected_tap=None, to_host=True):
    """One frame of `tr` through RayTracer.render_device into tensors this call owns and has poisoned (ARGB int32 [rows, W]
    = SENTINEL, the tap float32 [rows, W, 4] = NaN), between two torch.cuda.synchronize(); check_written on the result.
    -> (argb uint32 [rows, W], tap float32 [rows, W, 4] or None) as numpy arrays, or with to_host=False the torch tensors
    (large frames: only the sentinel is looked for, on the device).  A context that owns no row gets one poisoned element
    (a pointer that is not NULL), which must come back untouched."""
    import torch
    dev = tr._torch_device()
    rows, w = tr.rows, tr.width
    flat_a = torch.full((max(rows * w, 1),), SENTINEL, dtype=torch.int32, device=dev)
    flat_t = torch.full((max(rows * w, 1), 4), float("nan"), dtype=torch.float32, device=dev) if want_tap else None
    torch.cuda.synchronize(dev)
    tr.render_device(rot, cam, light, focal, flat_a.data_ptr(), flat_t.data_ptr() if want_tap else None,
                     stream=tr._raw_stream(None, dev))
    torch.cuda.synchronize(dev)
    if rows == 0:
        assert int(flat_a[0]) == SENTINEL and (not want_tap or bool(torch.isnan(flat_t).all())), "a rank without rows wrote a pixel"
    argb = flat_a[:rows * w].reshape(rows, w)
    tap = flat_t[:rows * w].reshape(rows, w, 4) if want_tap else None
    if not to_host:
        n = int((argb == SENTINEL).sum())
        assert n == 0, "%d of %d pixels were never written (ARGB sentinel)" % (n, rows * w)
        return argb, tap
    argb = argb.cpu().numpy().view(np.uint32)
    tap = tap.cpu().numpy() if want_tap else None
    check_written(argb, tap, expected_tap)
    return argb, tap


def same_frame(got_argb, got_tap, want_argb, want_tap, what):
    """Bit for bit: ARGB words, and the first three tap components where want_tap (…, 3 or 4 channels) is given."""
    want_argb = np.asarray(want_argb).reshape(got_argb.shape)
    bad = np.argwhere(got_argb != want_argb)
    assert bad.size == 0, "%s: %d of %d pixels differ, first at (row, x) = %s: %08x, expected %08x" % (
        what, len(bad), got_argb.size, bad[0], got_argb[tuple(bad[0])], want_argb[tuple(bad[0])])
    if want_tap is not None and got_tap is not None:
        want = np.ascontiguousarray(np.asarray(want_tap).reshape(got_argb.shape + (-1,))[..., :3])
        got = np.ascontiguousarray(got_tap[..., :3])
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, "%s: %d tap components differ, first at (row, x, channel) = %s" % (what, len(bad), bad[0])


def mesh_scene(tmpdir, keep=44):
    """The box plus `keep` triangles of a bumpy sphere (n = 70: the mesh kernel, two tiles), cut to a count as
    walk_shapes_util.build_scene cuts it; the sphere hangs in the middle of the room, where EDGE_VIEWS look."""
    path = os.path.join(str(tmpdir), "coverage_%d.obj" % keep)
    assert meshgen.write_sphere_obj(path, 6, 5) >= keep
    sc = rt.Scene.cornell_box() + rt.Scene(rt.Scene.load_obj(path, translate=MESH_TRANSLATE).aos[:keep])
    assert len(sc) == 26 + keep
    return sc


def oracle_frame(oracle, cfg, scene, view, focal, pix=None):
    """The CPU oracle's (argb, rgb [.., 3]) of cfg's owned rows (or of the global pixel ids `pix`) under view = (yaw, pitch,
    cam, light)"""
    v, n, c = scene.packed()
    yaw, pitch, cam, light = view
    return oracle.render(cfg, v, n, c, rt.rotation_matrix(yaw, pitch), cam, light, focal, pix=pix, nthreads=8)


# ---- the sequences of section "the list on" -----------------------------------------------------------------------------
# Views (yaw, pitch, camera, light) on the box with light_spread 0.3.  The camera stands closer than the reference's and steps
# half a room to either side, turned back towards the middle: the CPU oracle finds 77, 81 and 83 % of a 256 x 96 frame's pixels
# on the scene (76 % and more at every case's shape; the tests assert half).  Between two views the room's image moves by a
# quarter of the frame's width and the light by 0.5 and more, so the blocks' penumbrae move by more than one 64-pixel job.
SEQ_SPREAD = 0.3
SEQ_VIEWS = (
    (0.0, 0.0, [0.0, 0.0, -2.4], [0.0, -0.5, -0.7]),
    (-0.2, 0.1, [0.5, 0.1, -2.2], [0.5, -0.6, -0.3]),
    (0.25, -0.05, [-0.6, 0.2, -2.1], [-0.5, -0.4, 0.1]),
)
SEQ_ORDER = (0, 0, 1, 2, 0, 1)


def seq_focal(cfg):
    """The sequences' focal length: the 1100-at-1024 of the reference scaled to the frame's WIDTH, halved: the wide frames of
    the cases (256 x 96) then see the room across their whole width."""
    return 0.5 * 1100.0 * cfg.width / 1024.0 * cfg.aa_x


# ---- the edge shapes ------------------------------------------------------------------------------------------------------
# The mesh's triangles lie within x -0.09 .. 0.29, y 0.03 .. 0.42, z 0.02 .. 0.38.  Both views stand INSIDE the room's open
# front and look at the mesh, past the glass sphere: every forward ray ends on the scene, so that even a 512 x 1 strip of a
# 64-pixel view is covered (the oracle finds 95 % and more at every shape), and the centre pixel of every shape is on the mesh.
MESH_TRANSLATE = (0.1, 0.6, 0.2)
EDGE_VIEWS = (
    (0.335, -0.102, [-0.3, 0.1, -0.95], [0.0, -0.5, -0.7]),
    (-0.4636, -0.681, [0.5, -0.5, -0.6], [0.4, -0.6, -0.2]),
)
LIMIT_VIEW = (0.1, 0.05, [0.1, 0.0, -3.0], [0.2, -0.5, -0.6])


def edge_focal(cfg):
    """The edge shapes' focal length: a tiny frame is the centre crop of a 64-pixel view"""
    return 1100.0 * 64 / 1024.0 * cfg.aa_x


def long_side_focal(cfg):
    """The limit shapes' focal length: scaled by the long side, so that the strip crosses the scene"""
    return 1100.0 * max(cfg.width, cfg.height) / 1024.0 * cfg.aa_x
