"""-m gpu: the a-trous filter on the device (rt_filter_plane / rt_filter_plane_device, rt_filter.hip) gives the bits of the numpy
restatement in tests/filter_util.py — on the sizes of the CPU comparison, on sizes just beyond a tile and beyond what one
grid.y holds, through both entries, in place and out of place, in the built-in choice of kernel forms and with every pass in
the direct form; its counters are the restatement's counts; calls on different streams order themselves and leave frames
alone; and render_filtered_light keeps fully lit and fully shadowed regions exactly."""
import numpy as np
import pytest

import filter_util as fu
from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    return abi.make_config(width=64, height=48, shadow_samples=4, **kw)


@pytest.fixture(scope="module")
def tracer(scene):
    tr = rt.RayTracer(_cfg(), scene)
    yield tr
    tr.close()


@pytest.fixture(scope="module")
def direct_tracer(scene):
    """A context whose filter passes all take their taps from the caches (the knob is read once, at rt_init)."""
    import os
    os.environ["UOB_RT_FILTER_FORM"] = "direct"
    try:
        tr = rt.RayTracer(_cfg(), scene)
    finally:
        del os.environ["UOB_RT_FILTER_FORM"]
    yield tr
    tr.close()


def _params(passes, param_set):
    p = fu.full_params(fu.PARAM_SETS[param_set])
    p["passes"] = passes
    return p


def _on_device(tr, h, w, params, inplace, side):
    """The torch entry on a stream of its own, behind the uploads of torch's current stream."""
    import torch
    value, pos, nrm = (torch.from_numpy(a.copy()).cuda() for a in fu.planes(h, w))
    side.wait_stream(torch.cuda.current_stream())
    out = tr.filter_plane_device(value, pos, nrm, out=value if inplace else None, stream=side, **params)
    torch.cuda.synchronize()
    assert (out is value) == inplace
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("param_set", list(fu.PARAM_SETS))
@pytest.mark.parametrize("size", fu.SIZES + fu.TILE_SIZES, ids=lambda s: "%dx%d" % s)
def test_device_equals_the_restatement(tracer, direct_tracer, size, param_set):
    import torch
    fu.check_sizes()
    h, w = size
    value, pos, nrm = fu.planes(h, w)
    side = torch.cuda.Stream()
    for passes in (1, 5, 8):
        want, stats = fu.reference(h, w, passes, param_set)
        p = _params(passes, param_set)
        got = tracer.filter_plane(value, pos, nrm, **p)
        assert np.array_equal(got.view(np.uint32), want)
        st = tracer.filter_stats()
        assert (st["pixels"], st["passes"]) == (h * w, passes)
        assert {k: st[k] for k in stats} == stats
        assert st["reserved5"] == st["reserved6"] == st["reserved7"] == 0
        host_inplace = value.copy()
        tracer.filter_plane(host_inplace, pos, nrm, out=host_inplace, **p)
        assert np.array_equal(host_inplace.view(np.uint32), want)
        assert np.array_equal(_on_device(tracer, h, w, p, False, side), want)
        assert np.array_equal(_on_device(tracer, h, w, p, True, side), want)
        assert {k: tracer.filter_stats()[k] for k in stats} == stats
        # every pass in the direct form: the same bits and the same counts
        assert np.array_equal(_on_device(direct_tracer, h, w, p, passes == 1, side), want)
        assert {k: direct_tracer.filter_stats()[k] for k in stats} == stats


def test_more_row_groups_than_one_grid_y_holds(tracer):
    """A plane so tall that the row groups of a launch continue in grid.z, in the tiled form (passes 0 .. 5) and in the direct
    form (pass 6)."""
    import torch
    fu.check_sizes()
    (h, w), passes = fu.TALL_SIZE, fu.TALL_PASSES
    want, stats = fu.reference(h, w, passes, "defaults")
    got = _on_device(tracer, h, w, _params(passes, "defaults"), False, torch.cuda.Stream())
    assert np.array_equal(got, want)
    assert {k: tracer.filter_stats()[k] for k in stats} == stats


def test_two_calls_on_two_streams_and_a_frame_between_them(tracer):
    """Filter calls share the context's scratch, so the second waits for the first on the device whatever its stream; a frame
    is no party to that: rendered between them it has the bits of a frame rendered alone."""
    import torch
    cfg = tracer.cfg
    rot = rt.rotation_matrix(0.0, 0.0)
    alone = tracer.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg)).copy()
    (ha, wa), (hb, wb) = (70, 200), (37, 100)
    pa, pb = _params(8, "defaults"), _params(5, "value_0.25")
    a_in = [torch.from_numpy(x.copy()).cuda() for x in fu.planes(ha, wa)]
    b_in = [torch.from_numpy(x.copy()).cuda() for x in fu.planes(hb, wb)]
    d_argb = torch.zeros((cfg.height, cfg.width), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    out_a = tracer.filter_plane_device(*a_in, stream=s1, **pa)
    tracer.render_device(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg), d_argb.data_ptr(), stream=s3.cuda_stream)
    out_b = tracer.filter_plane_device(*b_in, stream=s2, **pb)
    torch.cuda.synchronize()
    assert np.array_equal(out_a.cpu().numpy().view(np.uint32), fu.reference(ha, wa, 8, "defaults")[0])
    assert np.array_equal(out_b.cpu().numpy().view(np.uint32), fu.reference(hb, wb, 5, "value_0.25")[0])
    assert np.array_equal(d_argb.cpu().numpy().view(np.uint32), alone)
    # and serially, through the blocking entry: the same bits again
    assert np.array_equal(tracer.filter_plane(*fu.planes(ha, wa), **pa).view(np.uint32), out_a.cpu().numpy().view(np.uint32))
    assert np.array_equal(tracer.filter_plane(*fu.planes(hb, wb), **pb).view(np.uint32), out_b.cpu().numpy().view(np.uint32))


def test_multi_device_context_filters_on_its_first_device(scene, tracer):
    tr = rt.RayTracer(_cfg(devices=(0, 0), device_band_rows=8), scene)
    try:
        h, w = 37, 100
        want, stats = fu.reference(h, w, 5, "defaults")
        assert np.array_equal(tr.filter_plane(*fu.planes(h, w)).view(np.uint32), want)
        assert {k: tr.filter_stats()[k] for k in stats} == stats
        import torch
        assert np.array_equal(_on_device(tr, h, w, _params(5, "defaults"), True, torch.cuda.Stream()), want)
    finally:
        tr.close()


# ---- real planes: the Cornell box at 128 x 128, one sample per pixel, 4 shadow samples ----------------------------------------
@pytest.fixture(scope="module")
def box128(scene):
    import torch
    cfg = abi.make_config(width=128, height=128, aa_x=1, aa_y=1, shadow_samples=4)
    tr = rt.RayTracer(cfg, scene)
    rot = rt.rotation_matrix(0.0, 0.0)
    view = (rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg))
    planes = tr.render_aov(rot, DEFAULT_CAM, focal_for(cfg), planes=("prim", "position", "normal"))
    filtered = [t.cpu().numpy() for t in tr.render_filtered_light(*view, want_parts=True)]
    unfiltered = [t.cpu().numpy() for t in tr.render_filtered_light(*view, want_parts=True, normal_min_dot=2.0)]
    torch.cuda.synchronize()
    yield tr, view, planes, filtered, unfiltered
    tr.close()


def test_filtered_light_without_accepted_taps_is_the_unfiltered_product(box128):
    tr, view, planes, _, (out, term, vis, vis_f) = box128
    assert np.array_equal(vis_f.view(np.uint32), vis.view(np.uint32))
    assert np.array_equal(out.view(np.uint32), (term * vis).view(np.uint32))
    hit = planes["prim"] != -1
    assert hit.any() and (~hit).any() and (out[~hit] == 0).all() and (out[hit] > 0).any()
    counts = np.rint(vis * 4)
    assert np.array_equal(counts / np.float32(4), vis) and set(np.unique(counts)) <= {0, 1, 2, 3, 4}
    assert 0 < (counts[hit] < 4).sum() and (counts[hit] == 4).sum() > 0          # there are penumbrae and lit floors


def test_filtered_light_keeps_lit_and_shadowed_regions_exactly(box128):
    tr, view, planes, (out, term, vis, vis_f), _ = box128
    pos, nrm = planes["position"], planes["normal"]
    hit = planes["prim"] != -1
    assert np.array_equal(hit, pos[..., 3] > 0)
    # the device's V_f is the restatement's on these planes too
    want, _ = fu.filter_plane(vis, pos, nrm, **fu.DEFAULTS)
    assert np.array_equal(vis_f.view(np.uint32), want.view(np.uint32))
    lit = fu.untouched_region(vis == 1.0, pos, nrm)
    dark = fu.untouched_region(hit & (vis == 0.0), pos, nrm)
    assert lit.sum() > 1000 and dark.sum() > 10
    assert (vis_f[lit] == np.float32(1.0)).all() and (vis_f[dark] == 0).all()
    assert np.array_equal(out[lit].view(np.uint32), term[lit].view(np.uint32))
    assert (vis_f[~hit] == 0).all() and (out[~hit] == 0).all()                  # misses stay 0
    assert not np.array_equal(vis_f, vis)                                       # and the penumbrae did change
    assert (vis_f[hit] >= 0).all() and (vis_f[hit] <= 1).all()


def test_filtered_light_refuses_bands_and_bad_samples(scene, box128):
    tr, view, *_ = box128
    with pytest.raises(ValueError):
        tr.render_filtered_light(*view, sample=1)                               # 1 x 1 AA: only sample 0
    bands = rt.RayTracer(abi.make_config(width=64, height=48, band_rows=8, band_index=0, band_count=2), scene)
    try:
        with pytest.raises(ValueError):
            bands.render_filtered_light(rt.rotation_matrix(0.0, 0.0), DEFAULT_CAM, DEFAULT_LIGHT, focal_for(bands.cfg))
    finally:
        bands.close()
