"""-m gpu: the temporal reprojection on the device (rt_accumulate_plane / rt_accumulate_plane_device, rt_accumulate.hip) gives the
bits of the numpy restatement in tests/accumulate_util.py on every word of the history and on both output planes — on the sizes
of the CPU comparison, on sizes just beyond a tile and beyond what one grid.y holds, through both entries, with and without the
optional planes; its counters are the restatement's counts; chained calls alternate two histories; calls on different streams
order themselves and leave frames alone; and render_accumulated_light accumulates the visibility of a still view as the
restatement does, lowers its error, keeps fully lit and fully shadowed regions exactly and restarts where a pan changes the
primitive."""
import numpy as np
import pytest

import accumulate_util as au
from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu
F32 = np.float32


def _cfg(**kw):
    return abi.make_config(width=64, height=48, shadow_samples=4, **kw)


@pytest.fixture(scope="module")
def tracer(scene):
    tr = rt.RayTracer(_cfg(), scene)
    yield tr
    tr.close()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _on_device(tr, planes, kw, focal, side, want_mean=True, want_variance=True):
    """The torch entry on a stream of its own, behind the uploads of torch's current stream -> bits of (next, mean, variance)."""
    import torch
    d = [torch.from_numpy(a.copy()).cuda() if a is not None else None for a in planes]
    side.wait_stream(torch.cuda.current_stream())
    nxt, mean, var = tr.accumulate_plane_device(d[0], d[1], d[2], prim=d[3], prev=d[4], stream=side, want_mean=want_mean,
                                                want_variance=want_variance, prev_focal=focal, **kw)
    torch.cuda.synchronize()
    assert (mean is not None) == want_mean and (var is not None) == want_variance
    return _bits(nxt), _bits(mean) if want_mean else None, _bits(var) if want_variance else None


def _stats_equal(tr, stats):
    st = tr.accumulate_stats()
    assert {k: st[k] for k in stats} == stats
    assert st["reserved5"] == st["reserved6"] == st["reserved7"] == 0


@pytest.mark.parametrize("param_set", list(au.PARAM_SETS))
@pytest.mark.parametrize("size", au.SIZES + au.TILE_SIZES, ids=lambda s: "%dx%d" % s)
def test_device_equals_the_restatement(tracer, size, param_set):
    import torch
    au.check_sizes()
    h, w = size
    planes, kw = au.call_args(h, w, param_set)
    want_next, want_mean, want_var, stats = au.reference(h, w, param_set)
    nxt, mean, var = tracer.accumulate_plane(*planes, prev_focal=w, **kw)
    assert np.array_equal(nxt.view(np.uint32), want_next)
    assert np.array_equal(mean.view(np.uint32), want_mean)
    assert np.array_equal(var.view(np.uint32), want_var)
    _stats_equal(tracer, stats)
    side = torch.cuda.Stream()
    for want_m, want_v in ((True, True), (False, True), (True, False), (False, False)):
        got = _on_device(tracer, planes, kw, w, side, want_m, want_v)
        assert np.array_equal(got[0], want_next)
        assert got[1] is None or np.array_equal(got[1], want_mean)
        assert got[2] is None or np.array_equal(got[2], want_var)
        _stats_equal(tracer, stats)


def test_more_row_groups_than_one_grid_y_holds(tracer):
    """A plane so tall that the row groups of the launch continue in grid.z."""
    import torch
    au.check_sizes()
    h, w = au.TALL_SIZE
    planes, kw = au.call_args(h, w, "defaults", h, au.TALL_VIEW)
    want_next, want_mean, want_var, stats = au.reference(h, w, "defaults", h, au.TALL_VIEW)
    assert stats["found_history"] > stats["valid_pixels"] // 2
    got = _on_device(tracer, planes, kw, h, torch.cuda.Stream())
    assert np.array_equal(got[0], want_next) and np.array_equal(got[1], want_mean) and np.array_equal(got[2], want_var)
    _stats_equal(tracer, stats)


def _sequence(h, w, frames):
    """Views that pan a little from frame to frame, with their guides and noisy values."""
    rng = np.random.default_rng(77)
    out = []
    for k in range(frames):
        rot, cam = au.yaw_matrix(0.02 * k), np.array([0.01 * k, 0.0, -2.0 + 0.01 * k], F32)
        pos, nrm, prim = au.view_guides(h, w, rot, cam, w)
        out.append((rot, cam, au.spoil(rng, pos), nrm, prim, au.noisy_values(rng, h, w)))
    return out


def test_three_chained_frames_alternate_two_histories(tracer):
    import torch
    h, w = 37, 100
    seq = _sequence(h, w, 3)
    hist = [torch.empty((h, w, 12), dtype=torch.float32, device="cuda") for _ in range(2)]
    want_prev, view = None, {}
    for k, (rot, cam, pos, nrm, prim, value) in enumerate(seq):
        want_next, want_mean, want_var, stats, _ = au.accumulate(value, pos, nrm, prim, want_prev, prev_focal_px=w, max_history=2,
                                                                 **(view or dict(prev_rot=rot, prev_cam=cam)))
        d = [torch.from_numpy(a).cuda() for a in (value, pos, nrm, prim)]
        nxt, mean, var = tracer.accumulate_plane_device(*d, prev=hist[(k + 1) & 1] if k else None, next=hist[k & 1], prev_focal=w,
                                                        max_history=2, **(view or dict(prev_rot=rot, prev_cam=cam)))
        assert nxt is hist[k & 1]
        torch.cuda.synchronize()
        assert np.array_equal(_bits(nxt), want_next.view(np.uint32))
        assert np.array_equal(_bits(mean), want_mean.view(np.uint32)) and np.array_equal(_bits(var), want_var.view(np.uint32))
        _stats_equal(tracer, stats)
        if k:
            assert stats["found_history"] > stats["valid_pixels"] // 2
        want_prev, view = want_next, dict(prev_rot=rot, prev_cam=cam)
    assert set(np.unique(want_next[..., au.COUNT])) == {0.0, 1.0, 2.0}


def test_two_calls_on_two_streams_and_a_frame_between_them(tracer):
    """Accumulate calls share the context's counters, so the second waits for the first on the device whatever its stream; a
    frame is no party to that: rendered between them it has the bits of a frame rendered alone."""
    import torch
    cfg = tracer.cfg
    rot = rt.rotation_matrix(0.0, 0.0)
    alone = tracer.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg)).copy()
    (ha, wa), (hb, wb) = (70, 200), (37, 100)
    (pa, ka), (pb, kb) = au.call_args(ha, wa, "defaults"), au.call_args(hb, wb, "max_history_4")
    a_in = [torch.from_numpy(x.copy()).cuda() for x in pa]
    b_in = [torch.from_numpy(x.copy()).cuda() for x in pb]
    d_argb = torch.zeros((cfg.height, cfg.width), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    out_a = tracer.accumulate_plane_device(*a_in[:3], prim=a_in[3], prev=a_in[4], stream=s1, prev_focal=wa, **ka)
    tracer.render_device(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg), d_argb.data_ptr(), stream=s3.cuda_stream)
    out_b = tracer.accumulate_plane_device(*b_in[:3], prim=b_in[3], prev=b_in[4], stream=s2, prev_focal=wb, **kb)
    torch.cuda.synchronize()
    for out, want in ((out_a, au.reference(ha, wa, "defaults")), (out_b, au.reference(hb, wb, "max_history_4"))):
        for got, ref in zip(out, want[:3]):
            assert np.array_equal(_bits(got), ref)
    _stats_equal(tracer, au.reference(hb, wb, "max_history_4")[3])
    assert np.array_equal(d_argb.cpu().numpy().view(np.uint32), alone)


def test_multi_device_context_accumulates_on_its_first_device(scene):
    import torch
    tr = rt.RayTracer(_cfg(devices=(0, 0), device_band_rows=8), scene)
    try:
        h, w = 37, 100
        planes, kw = au.call_args(h, w, "defaults")
        want_next, want_mean, want_var, stats = au.reference(h, w, "defaults")
        nxt, mean, var = tr.accumulate_plane(*planes, prev_focal=w, **kw)
        assert np.array_equal(nxt.view(np.uint32), want_next) and np.array_equal(mean.view(np.uint32), want_mean)
        assert np.array_equal(var.view(np.uint32), want_var)
        _stats_equal(tr, stats)
        got = _on_device(tr, planes, kw, w, torch.cuda.Stream())
        assert np.array_equal(got[0], want_next) and np.array_equal(got[1], want_mean) and np.array_equal(got[2], want_var)
    finally:
        tr.close()


# ---- end to end: the Cornell box at 64 x 48, one sample per pixel, 4 shadow samples, a wide light ---------------------------
LIGHT_SPREAD = 0.3       # the shipped 0.05 gives nearly hard shadows: a few pixels of penumbra at this size
FRAMES = 8
PAN = (0.05, [0.03, 0.0, -3.17])     # yaw, camera of the ninth frame


@pytest.fixture(scope="module")
def box(scene):
    import torch
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=4, light_spread=LIGHT_SPREAD)
    tr = rt.RayTracer(cfg, scene)
    ref = rt.RayTracer(abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=64, light_spread=LIGHT_SPREAD), scene)
    rot, focal = rt.rotation_matrix(0.0, 0.0), focal_for(cfg)
    planes = tr.render_aov(rot, DEFAULT_CAM, focal, planes=("prim", "position", "normal"))
    hit = planes["prim"] != -1
    k = cfg.width * cfg.height
    _, c64 = ref.shade_points(planes["position"][..., :3].reshape(k, 3), planes["normal"][..., :3].reshape(k, 3), DEFAULT_LIGHT,
                              seeds=np.arange(k, dtype=np.int32), want_counts=True)
    v64 = np.where(hit, c64.reshape(hit.shape).astype(F32) / F32(64), F32(0))
    ref.close()
    frames = []
    for _ in range(FRAMES):
        parts = tr.render_accumulated_light(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal, want_parts=True)
        frames.append([t.cpu().numpy().copy() for t in parts])
    pan_rot = rt.rotation_matrix(PAN[0], 0.0)
    pan_planes = tr.render_aov(pan_rot, PAN[1], focal, planes=("prim", "position", "normal"))
    pan = [t.cpu().numpy().copy() for t in tr.render_accumulated_light(pan_rot, PAN[1], DEFAULT_LIGHT, focal, want_parts=True)]
    pan_stats = tr.accumulate_stats()
    torch.cuda.synchronize()
    yield tr, (rot, focal), planes, hit, v64, frames, pan_planes, (pan, pan_stats)
    tr.close()


def test_accumulated_light_is_the_restatement_over_eight_frames(box):
    tr, (rot, focal), planes, hit, v64, frames, pan_planes, pan = box
    pos, nrm, prim = planes["position"], planes["normal"], planes["prim"]
    assert np.array_equal(hit, pos[..., 3] > 0)
    penumbra = hit & (v64 > 0) & (v64 < 1)
    print("penumbra pixels at 64 samples: %d of %d hits" % (penumbra.sum(), hit.sum()))
    assert penumbra.sum() >= 100
    view = dict(prev_rot=rot, prev_cam=np.array(DEFAULT_CAM, F32), prev_focal_px=F32(focal))
    prev, always, lit, dark = None, hit.copy(), None, None
    for k, (out, term, vis, vis_m, var, count) in enumerate(frames):
        assert set(np.unique(np.rint(vis * 4))) <= {0, 1, 2, 3, 4} and np.array_equal(np.rint(vis * 4) / F32(4), vis)
        if k:
            assert not np.array_equal(vis, frames[k - 1][2])                 # every frame draws another jitter stream
        taps = []
        prev, want_mean, want_var, stats, ntaps = au.accumulate(vis, pos, nrm, prim, prev, tap_list=taps, **view)
        assert np.array_equal(vis_m.view(np.uint32), want_mean.view(np.uint32))
        assert np.array_equal(var.view(np.uint32), want_var.view(np.uint32))
        assert np.array_equal(count.view(np.uint32), prev[..., au.COUNT].view(np.uint32))
        assert np.array_equal(out.view(np.uint32), (term * np.where(hit, vis_m, F32(0))).view(np.uint32))
        assert (out[~hit] == 0).all()
        if k:                                     # it found history, and so did every record it took, frame after frame
            always = au.exact_region(always, ntaps > 0, taps)
        lit = au.exact_region(lit, hit & (vis == 1), taps)
        dark = au.exact_region(dark, hit & (vis == 0), taps)
    # a still view reprojects every hit onto itself
    print("always found history: %d of %d hits; exactly lit %d, exactly dark %d" % (always.sum(), hit.sum(), lit.sum(), dark.sum()))
    assert always.sum() > 0.9 * hit.sum()
    assert (count[always] == FRAMES).all()
    assert lit.sum() > 100 and dark.sum() > 0
    assert (vis_m[lit] == F32(1)).all() and (vis_m[dark] == 0).all() and (var[lit] == 0).all() and (var[dark] == 0).all()
    assert np.array_equal(out[lit].view(np.uint32), term[lit].view(np.uint32))
    # and the accumulated visibility is nearer the 64-sample one than a single frame's, where it matters
    rms = lambda a: float(np.sqrt(np.mean((a[penumbra].astype(np.float64) - v64[penumbra]) ** 2)))
    print("penumbra RMS against 64 samples: frame eight alone %.4f, accumulated %.4f, ratio %.3f" % (rms(vis), rms(vis_m), rms(vis_m) / rms(vis)))
    assert rms(vis_m) < rms(vis)


def test_a_pan_restarts_the_pixels_whose_primitive_changed(box):
    tr, (rot, focal), planes, hit, v64, frames, pan_planes, pan = box
    pos, nrm, prim = pan_planes["position"], pan_planes["normal"], pan_planes["prim"]
    (out, term, vis, vis_m, var, count), pan_stats = pan
    # the history the ninth frame saw: the restatement's after eight frames (the previous test pins the device to it)
    view = dict(prev_rot=rot, prev_cam=np.array(DEFAULT_CAM, F32), prev_focal_px=F32(focal))
    prev = None
    for f in frames:
        prev = au.accumulate(f[2], planes["position"], planes["normal"], planes["prim"], prev, **view)[0]
    taps = []
    want_next, want_mean, _, stats, ntaps = au.accumulate(vis, pos, nrm, prim, prev, tap_list=taps, **view)
    assert np.array_equal(vis_m.view(np.uint32), want_mean.view(np.uint32))
    assert np.array_equal(count.view(np.uint32), want_next[..., au.COUNT].view(np.uint32))
    valid = pos[..., 3] > 0
    prev_prim = prev[..., au.PRIM].view(np.int32)
    changed, reprojected = valid.copy(), np.zeros_like(valid)   # it reprojects into the previous frame, onto other primitives only
    for qy, qx, _, inside in taps:
        changed &= ~inside | (prev_prim[qy, qx] != prim)
        reprojected |= inside
    changed &= reprojected
    print("pan: %d valid, %d found history, %d without a candidate, %d changed primitive" %
          (valid.sum(), stats["found_history"], stats["no_candidate"], changed.sum()))
    assert changed.sum() > 0 and (count[changed] == 1).all()
    assert stats["found_history"] > valid.sum() // 2 and (count[ntaps > 0] > 1).all()
    assert {k: pan_stats[k] for k in stats} == stats


def test_accumulated_light_refuses_bands_and_bad_samples_and_resets(scene, box):
    import torch
    tr, (rot, focal), *_ = box
    with pytest.raises(ValueError):
        tr.render_accumulated_light(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal, sample=1)          # 1 x 1 AA: only sample 0
    tr.reset_history()
    _, _, vis, vis_m, _, count = tr.render_accumulated_light(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal, want_parts=True)
    filtered = tr.render_accumulated_light(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal, filter=True)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(vis_m), _bits(vis)) and float(count.max()) == 1.0          # a first frame again
    assert np.array_equal(_bits(vis), box[5][0][2].view(np.uint32))                        # with the first frame's seeds
    assert tuple(filtered.shape) == (48, 64) and bool(torch.isfinite(filtered).all())
    bands = rt.RayTracer(abi.make_config(width=64, height=48, band_rows=8, band_index=0, band_count=2), scene)
    try:
        with pytest.raises(ValueError):
            bands.render_accumulated_light(rt.rotation_matrix(0.0, 0.0), DEFAULT_CAM, DEFAULT_LIGHT, focal_for(bands.cfg))
    finally:
        bands.close()
