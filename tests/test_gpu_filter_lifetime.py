"""-m gpu: what the filter calls take of the device and give back (rt_debug_live_device_objects): a context that
never filters holds nothing for them, only a call larger than any before it allocates, and rt_destroy returns everything."""
import gc

import numpy as np
import pytest

import filter_util as fu
from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu


def _live():
    gc.collect()
    return rt.live_device_objects()


def _cfg():
    return abi.make_config(width=64, height=48, shadow_samples=4)


def test_a_context_that_never_filters_allocates_nothing_for_the_family(scene):
    cfg = _cfg()
    start = _live()
    plain = rt.RayTracer(cfg, scene)
    plain.render(rt.rotation_matrix(0.0, 0.0), DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg))
    without = _live()
    plain.close()
    assert _live() == start
    tr = rt.RayTracer(cfg, scene)
    tr.render(rt.rotation_matrix(0.0, 0.0), DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg))
    assert _live() == without                                       # the same context again: nothing of the family yet
    h, w = 37, 100
    tr.filter_plane(*fu.planes(h, w))
    first = _live()
    # the event, the counters (8 exported words and 64 partial sums of a 128-byte line each), the staging of the blocking entry (40 bytes per pixel), the guides (32) and the two planes (8)
    assert first["events"] == without["events"] + 1 and first["streams"] == without["streams"]
    assert first["allocations"] == without["allocations"] + 4
    assert first["bytes"] == without["bytes"] + 8 * (8 + 64 * 16) + 80 * h * w
    tr.close()
    assert _live() == start


def test_only_a_larger_call_allocates_and_destroy_returns_everything(scene):
    import torch
    start = _live()
    tr = rt.RayTracer(_cfg(), scene)
    h, w = 37, 100
    want, _ = fu.reference(h, w, 5, "defaults")
    tr.filter_plane(*fu.planes(h, w))
    once = _live()
    assert np.array_equal(tr.filter_plane(*fu.planes(h, w)).view(np.uint32), want)
    assert np.array_equal(tr.filter_plane(*fu.planes(5, 5)).view(np.uint32), fu.reference(5, 5, 5, "defaults")[0])   # smaller
    assert _live() == once
    d = [torch.from_numpy(a.copy()).cuda() for a in fu.planes(h, w)]
    torch.cuda.synchronize()
    tr.filter_plane_device(*d)                                       # the device entry of that size: the scratch is there
    tr.filter_plane_device(d[0], d[1], d[2], out=d[0], passes=1)     # in place with one pass: through the scratch, not more of it
    torch.cuda.synchronize()
    assert _live() == once
    tr.filter_plane(*fu.planes(70, 200))                             # larger than any before: staging and scratch grow
    grown = _live()
    assert grown["allocations"] == once["allocations"] and grown["bytes"] == once["bytes"] + 80 * (70 * 200 - h * w)
    d = [torch.from_numpy(a.copy()).cuda() for a in fu.planes(70, 200)]
    torch.cuda.synchronize()
    tr.filter_plane_device(*d)                                       # a call is pending when the context goes
    tr.close()
    torch.cuda.synchronize()
    assert _live() == start
