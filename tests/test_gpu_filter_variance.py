"""-m gpu: the variance-guided a-trous filter on the device (rt_filter_plane_variance / rt_filter_plane_variance_device,
rt_filter_variance.hip) gives the bits of the numpy restatement in tests/filter_variance_util.py on value and variance — on the
sizes of the CPU comparison, on sizes just beyond a tile and beyond what one grid.y holds, through both entries, in place and out
of place, in the built-in choice of kernel forms and with every pass in the direct form; its counters are the restatement's
counts; variance calls and plain calls share the scratch and order themselves, and leave frames alone; and
render_accumulated_light(filter="variance") is the restatement of its own parts."""
import numpy as np
import pytest

import filter_util as fu
import filter_variance_util as fv
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
    p = fv.full_params(fv.PARAM_SETS[param_set])
    p["passes"] = passes
    return p


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _on_device(tr, h, w, params, inplace, side, want_variance=True):
    """The torch entry on a stream of its own, behind the uploads of torch's current stream -> (value bits, variance bits)."""
    import torch
    value, var, pos, nrm = (torch.from_numpy(a.copy()).cuda() for a in fv.planes(h, w))
    side.wait_stream(torch.cuda.current_stream())
    out, ovar = tr.filter_plane_variance_device(value, var, pos, nrm, out=value if inplace else None,
                                                out_variance=var if inplace else None, want_variance=want_variance, stream=side,
                                                **params)
    torch.cuda.synchronize()
    assert (out is value) == inplace and (ovar is var) == inplace
    return _bits(out.cpu().numpy()), (_bits(ovar.cpu().numpy()) if ovar is not None else None)


def _same(got, want, vwant):
    return np.array_equal(got[0], want) and np.array_equal(got[1], vwant)


@pytest.mark.parametrize("param_set", ["defaults", "eps_0.05"])
@pytest.mark.parametrize("size", fu.SIZES + fu.TILE_SIZES, ids=lambda s: "%dx%d" % s)
def test_device_equals_the_restatement(tracer, direct_tracer, size, param_set):
    import torch
    fv.check_sizes()
    h, w = size
    value, var, pos, nrm = fv.planes(h, w)
    side = torch.cuda.Stream()
    for passes in (1, 5, 8):
        want, vwant, stats = fv.reference(h, w, passes, param_set)
        p = _params(passes, param_set)
        got = tracer.filter_plane_variance(value, var, pos, nrm, **p)
        assert _same((_bits(got[0]), _bits(got[1])), want, vwant)
        st = tracer.filter_variance_stats()
        assert (st["pixels"], st["passes"]) == (h * w, passes)
        assert {k: st[k] for k in stats} == stats
        assert st["reserved6"] == st["reserved7"] == 0
        v, r = value.copy(), var.copy()
        tracer.filter_plane_variance(v, r, pos, nrm, out=v, out_variance=r, **p)
        assert _same((_bits(v), _bits(r)), want, vwant)
        assert _same(_on_device(tracer, h, w, p, False, side), want, vwant)
        assert _same(_on_device(tracer, h, w, p, True, side), want, vwant)
        assert {k: tracer.filter_variance_stats()[k] for k in stats} == stats
        # without out_variance: the same value
        got, none = _on_device(tracer, h, w, p, False, side, want_variance=False)
        assert none is None and np.array_equal(got, want)
        # every pass in the direct form: the same bits and the same counts
        assert _same(_on_device(direct_tracer, h, w, p, passes == 1, side), want, vwant)
        assert {k: direct_tracer.filter_variance_stats()[k] for k in stats} == stats


def test_more_row_groups_than_one_grid_y_holds(tracer):
    """A plane so tall that the row groups of a launch continue in grid.z, in the threshold launch, in the tiled form (passes
    0 .. 5) and in the direct form (pass 6)."""
    import torch
    fv.check_sizes()
    (h, w), passes = fu.TALL_SIZE, fu.TALL_PASSES
    want, vwant, stats = fv.reference(h, w, passes, "defaults")
    assert _same(_on_device(tracer, h, w, _params(passes, "defaults"), False, torch.cuda.Stream()), want, vwant)
    assert {k: tracer.filter_variance_stats()[k] for k in stats} == stats


# (first variance call, plain call, second and larger variance call): the plain call smaller than both, and the plain call the
# one that grows the shared part of the scratch
ORDERS = {"variance_grows": ((37, 100), (5, 65), (70, 200)), "plain_grows": ((9, 129), (70, 200), (70, 200))}


@pytest.mark.parametrize("order", list(ORDERS))
def test_variance_and_plain_calls_share_the_scratch_on_three_streams(scene, order):
    """The calls of the filter family share the context's scratch, so each waits for the one before it on the device whatever
    its stream; a frame is no party to that.  All four have the bits of running alone."""
    import torch
    tr = rt.RayTracer(_cfg(), scene)
    try:
        cfg = tr.cfg
        rot = rt.rotation_matrix(0.0, 0.0)
        alone = tr.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg)).copy()
        (ha, wa), (hb, wb), (hc, wc) = ORDERS[order]
        a_in = [torch.from_numpy(x.copy()).cuda() for x in fv.planes(ha, wa)]
        b_in = [torch.from_numpy(x.copy()).cuda() for x in fu.planes(hb, wb)]
        c_in = [torch.from_numpy(x.copy()).cuda() for x in fv.planes(hc, wc)]
        d_argb = torch.zeros((cfg.height, cfg.width), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s1, s2, s3, s4 = (torch.cuda.Stream() for _ in range(4))
        out_a = tr.filter_plane_variance_device(*a_in, stream=s1, **_params(5, "defaults"))
        tr.render_device(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg), d_argb.data_ptr(), stream=s4.cuda_stream)
        out_b = tr.filter_plane_device(*b_in, stream=s2, passes=8)
        out_c = tr.filter_plane_variance_device(*c_in, stream=s3, **_params(8, "eps_0.05"))
        torch.cuda.synchronize()
        want_a = fv.reference(ha, wa, 5, "defaults")
        want_c = fv.reference(hc, wc, 8, "eps_0.05")
        assert _same([_bits(t.cpu().numpy()) for t in out_a], *want_a[:2])
        assert np.array_equal(_bits(out_b.cpu().numpy()), fu.reference(hb, wb, 8, "defaults")[0])
        assert _same([_bits(t.cpu().numpy()) for t in out_c], *want_c[:2])
        assert np.array_equal(d_argb.cpu().numpy().view(np.uint32), alone)
        assert {k: tr.filter_variance_stats()[k] for k in want_c[2]} == want_c[2]
        # a plain call reports no variance-stopped taps, also behind a variance call that counted some
        assert want_c[2]["variance_stopped"] > 0
        tr.filter_plane_device(*b_in, stream=s2, passes=8)
        plain_stats = fu.reference(hb, wb, 8, "defaults")[1]
        st = tr.filter_stats()
        assert {k: st[k] for k in plain_stats} == plain_stats and st["reserved5"] == 0
        assert tr.filter_variance_stats()["variance_stopped"] == 0
    finally:
        tr.close()


def test_multi_device_context_filters_on_its_first_device(scene):
    import torch
    tr = rt.RayTracer(_cfg(devices=(0, 0), device_band_rows=8), scene)
    try:
        h, w = 37, 100
        want, vwant, stats = fv.reference(h, w, 5, "defaults")
        got = tr.filter_plane_variance(*fv.planes(h, w))
        assert _same((_bits(got[0]), _bits(got[1])), want, vwant)
        assert {k: tr.filter_variance_stats()[k] for k in stats} == stats
        assert _same(_on_device(tr, h, w, _params(5, "defaults"), True, torch.cuda.Stream()), want, vwant)
    finally:
        tr.close()


# ---- real planes: the Cornell box at 128 x 128, one sample per pixel, 4 shadow samples, three accumulated frames -----------------
FRAMES = 3


@pytest.fixture(scope="module")
def box128(scene):
    import torch
    cfg = abi.make_config(width=128, height=128, aa_x=1, aa_y=1, shadow_samples=4)
    tr = rt.RayTracer(cfg, scene)
    rot = rt.rotation_matrix(0.0, 0.0)
    view = (rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg))
    planes = tr.render_aov(rot, DEFAULT_CAM, focal_for(cfg), planes=("prim", "position", "normal"))
    runs = {}
    for mode in ("variance", True, False):
        tr.reset_history()
        for _ in range(FRAMES):
            parts = tr.render_accumulated_light(*view, filter=mode, want_parts=True)
        torch.cuda.synchronize()
        runs[mode] = [t.cpu().numpy().copy() for t in parts]
    yield tr, view, planes, runs
    tr.close()


def test_accumulated_light_with_the_variance_filter_is_the_restatement_of_its_parts(box128):
    tr, view, planes, runs = box128
    pos, nrm = planes["position"], planes["normal"]
    hit = planes["prim"] != -1
    assert len(runs["variance"]) == 7 and len(runs[True]) == len(runs[False]) == 6
    out, term, vis, vis_m, var, count, var_f = runs["variance"]
    assert float(count.max()) == FRAMES and (var[hit] > 0).any() and (var >= 0).all()
    want, vwant, stats = fv.filter_plane_variance(vis_m, var, pos, nrm, **fv.full_params({}))
    assert stats["variance_stopped"] > 0 and stats["accepted_taps"] > 5 * stats["valid_pixels"]
    assert np.array_equal(_bits(var_f), _bits(vwant))
    light = term * np.where(hit, want, np.float32(0))
    assert np.array_equal(_bits(out), _bits(light))
    # the three sequences drew the same samples: the same accumulated parts
    for other in (runs[True], runs[False]):
        for k in (1, 2, 3, 4, 5):
            assert np.array_equal(_bits(other[k]), _bits(runs["variance"][k]))
    # fully lit and fully dark regions keep 1.0 / 0.0 exactly (their accumulated variance is +0)
    lit = fu.untouched_region(vis_m == 1.0, pos, nrm)
    dark = fu.untouched_region(hit & (vis_m == 0.0), pos, nrm)
    assert lit.sum() > 1000 and dark.sum() > 10
    assert (var[lit] == 0).all() and (var[dark] == 0).all()
    assert (want[lit] == np.float32(1.0)).all() and (want[dark] == 0).all()
    assert np.array_equal(_bits(out[lit]), _bits(term[lit])) and (out[dark] == 0).all()
    assert (var_f[lit] == 0).all() and (var_f[dark] == 0).all()
    assert (out[~hit] == 0).all()
    assert not np.array_equal(want, vis_m)                                      # and the penumbrae did change


def test_accumulated_light_with_the_plain_filter_keeps_its_bits(box128):
    tr, view, planes, runs = box128
    pos, nrm = planes["position"], planes["normal"]
    hit = planes["prim"] != -1
    out, term, vis, vis_m, var, count = runs[True]
    want, _ = fu.filter_plane(vis_m, pos, nrm, **fu.DEFAULTS)
    assert np.array_equal(_bits(out), _bits(term * np.where(hit, want, np.float32(0))))
    raw = runs[False]
    assert np.array_equal(_bits(raw[0]), _bits(raw[1] * np.where(hit, raw[3], np.float32(0))))
    with pytest.raises(ValueError):
        tr.render_accumulated_light(*view, filter="svgf")
    with pytest.raises(TypeError):
        tr.render_accumulated_light(*view, filter=True, sigma_value=2.0)        # the variance filter's parameter only
