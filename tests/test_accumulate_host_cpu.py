"""CPU: the host statement of the temporal reprojection (rt_accumulate_plane_host, accumulate_host.cpp) gives the bits of the numpy
restatement in tests/accumulate_util.py on every word of the history and on both output planes, and has the properties the
header states: constant regions survive exactly, the history length climbs to max_history, a reprojection onto pixel centres
takes one tap, a previous camera that looks away leaves first frames, the variance is a variance, and noise averages out."""
import numpy as np
import pytest

import accumulate_util as au
from uob_raytracer_amd import runtime as rt

F32 = np.float32


def test_the_generator_is_sharp():
    stats = au.check_generator()
    assert stats["no_candidate"] > 0


@pytest.mark.parametrize("param_set", list(au.PARAM_SETS))
@pytest.mark.parametrize("size", au.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_equals_the_restatement(size, param_set):
    h, w = size
    planes, kw = au.call_args(h, w, param_set)
    want_next, want_mean, want_var, _ = au.reference(h, w, param_set)
    nxt, mean, var = rt.accumulate_plane_host(*planes, prev_focal=w, **kw)
    assert np.array_equal(nxt.view(np.uint32), want_next)
    assert np.array_equal(mean.view(np.uint32), want_mean)
    assert np.array_equal(var.view(np.uint32), want_var)
    # the variance is never negative or NaN, whatever the values (NaN and INF among them)
    assert (var >= 0).all()


def _still_view(h, w):
    rot, cam = au.yaw_matrix(0.0), np.array([0.0, 0.0, -2.0], F32)
    pos, nrm, prim = au.view_guides(h, w, rot, cam, w)
    return rot, cam, pos, nrm, prim


def test_a_constant_region_survives_and_the_history_length_climbs():
    h, w = 37, 100
    rot, cam, pos, nrm, prim = _still_view(h, w)
    valid = pos[..., 3] > 0
    assert valid.all()
    ones = np.ones((h, w), F32)
    prev = None
    for want in (1, 2, 3, 4, 4, 4):
        prev, mean, var = rt.accumulate_plane_host(ones, pos, nrm, prim, prev, prev_rot=rot, prev_cam=cam, prev_focal=w, max_history=4)
        assert (mean == F32(1)).all() and (prev[..., au.M2] == F32(1)).all() and (var == 0).all()
        assert (prev[..., au.COUNT] == F32(want)).all()
    zeros = np.zeros((h, w), F32)
    prev = None
    for _ in range(3):
        prev, mean, _ = rt.accumulate_plane_host(zeros, pos, nrm, prim, prev, prev_rot=rot, prev_cam=cam, prev_focal=w)
        assert (mean == 0).all() and (prev[..., au.M2] == 0).all()


def test_a_reprojection_onto_pixel_centres_takes_one_tap_of_weight_one():
    """Dyadic coordinates: the camera at the origin looks along z at the plane z = 2, focal = width = 16, so that every
    product and quotient of the projection is exact and fx, fy are the pixel's own integer coordinates."""
    h, w = 8, 16
    s = F32(0.125)
    pos = np.zeros((h, w, 4), F32)
    pos[..., 0] = (np.arange(w, dtype=F32) - F32(w / 2))[None, :] * s
    pos[..., 1] = (np.arange(h, dtype=F32) - F32(h / 2))[:, None] * s
    pos[..., 2] = F32(w) * s
    pos[..., 3] = 1
    nrm = np.zeros((h, w, 4), F32)
    nrm[..., 2] = -1
    rng = np.random.default_rng(5)
    first, second = rng.random((h, w), dtype=F32), rng.random((h, w), dtype=F32)
    view = dict(prev_rot=au.yaw_matrix(0.0), prev_cam=np.zeros(3, F32))
    prev, _, _ = rt.accumulate_plane_host(first, pos, nrm, None, None, prev_focal=w, **view)
    nxt, mean, _ = rt.accumulate_plane_host(second, pos, nrm, None, prev, prev_focal=w, **view)
    _, _, _, stats, taps = au.accumulate(second, pos, nrm, None, prev, prev_focal_px=w, **view)
    assert (taps == 1).all() and stats["accepted_taps"] == stats["found_history"] == h * w
    # one tap of weight 1: mp is the history's mean itself, and the blend factor is 1/2
    half = F32(0.5)
    assert np.array_equal(mean, first + half * (second - first))
    assert (nxt[..., au.COUNT] == 2).all()


def test_a_previous_camera_that_looks_away_leaves_first_frames():
    h, w = 37, 100
    planes, kw = au.call_args(h, w, "defaults")
    kw["prev_rot"] = au.yaw_matrix(np.pi)
    nxt, mean, _ = rt.accumulate_plane_host(*planes, prev_focal=w, **kw)
    want, _, _, stats, _ = au.accumulate(*planes, prev_focal_px=w, **kw)
    valid = planes[1][..., 3] > 0
    assert stats["no_candidate"] == stats["valid_pixels"] == valid.sum() and stats["found_history"] == 0
    assert np.array_equal(nxt.view(np.uint32), want.view(np.uint32))
    assert (nxt[..., au.COUNT][valid] == 1).all() and (nxt[..., au.COUNT][~valid] == 0).all()
    assert np.array_equal(mean.view(np.uint32), planes[0].view(np.uint32))         # every mean is the value's own bits


def test_eight_frames_of_noise_average_out():
    """Independent uniform noise on a still view: the mean of 8 frames has 1/sqrt(8) = 0.35 of a single frame's RMS error, and
    the test asks for less than half."""
    h, w = 37, 100
    rot, cam, pos, nrm, prim = _still_view(h, w)
    rng = np.random.default_rng(8)
    prev = None
    for _ in range(8):
        value = rng.random((h, w), dtype=F32)
        prev, mean, var = rt.accumulate_plane_host(value, pos, nrm, prim, prev, prev_rot=rot, prev_cam=cam, prev_focal=w)
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - 0.5) ** 2)))
    assert (prev[..., au.COUNT] == 8).all()
    print("rms of one frame %.4f, of the mean of eight %.4f" % (rms(value), rms(mean)))
    assert rms(mean) < 0.5 * rms(value)
    assert (var > 0).all()
