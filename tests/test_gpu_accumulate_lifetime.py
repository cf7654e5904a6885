"""-m gpu: what the accumulate calls take of the device and give back (rt_debug_live_device_objects): a context
that never accumulates holds nothing for them, the blocking entry's staging only grows, the device entry needs no more than the
event and the counters, and rt_destroy returns everything."""
import gc

import numpy as np
import pytest

import accumulate_util as au
from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

COUNTER_BYTES = 8 * (8 + 64 * 16)      # 8 exported words and 64 partial sums of a 128-byte line each
STAGING_PER_PIXEL = 144                # guides 16 + 16, prev and next 48 + 48, value, prim, mean, variance 4 each


def _live():
    gc.collect()
    return rt.live_device_objects()


def _cfg():
    return abi.make_config(width=64, height=48, shadow_samples=4)


def _call(tr, h, w):
    planes, kw = au.call_args(h, w, "defaults")
    return tr.accumulate_plane(*planes, prev_focal=w, **kw)


def test_a_context_that_never_accumulates_allocates_nothing_for_the_family(scene):
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
    _call(tr, h, w)
    first = _live()
    # the event, the counters and the staging of the blocking entry
    assert first["events"] == without["events"] + 1 and first["streams"] == without["streams"]
    assert first["allocations"] == without["allocations"] + 2
    assert first["bytes"] == without["bytes"] + COUNTER_BYTES + STAGING_PER_PIXEL * h * w
    tr.close()
    assert _live() == start


def test_the_device_entry_needs_only_the_event_and_the_counters(scene):
    import torch
    start = _live()
    tr = rt.RayTracer(_cfg(), scene)
    before = _live()
    h, w = 37, 100
    planes, kw = au.call_args(h, w, "defaults")
    d = [torch.from_numpy(a.copy()).cuda() for a in planes]
    nxt = torch.empty((h, w, 12), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tr.accumulate_plane_device(*d[:3], prim=d[3], prev=d[4], next=nxt, prev_focal=w, **kw)
    torch.cuda.synchronize()
    once = _live()
    assert once["events"] == before["events"] + 1 and once["streams"] == before["streams"]
    assert once["allocations"] == before["allocations"] + 1 and once["bytes"] == before["bytes"] + COUNTER_BYTES
    assert np.array_equal(nxt.cpu().numpy().view(np.uint32), au.reference(h, w, "defaults")[0])
    tr.close()
    assert _live() == start


def test_only_a_larger_call_allocates_and_destroy_returns_everything(scene):
    import torch
    start = _live()
    tr = rt.RayTracer(_cfg(), scene)
    h, w = 37, 100
    _call(tr, h, w)
    once = _live()
    assert np.array_equal(_call(tr, h, w)[0].view(np.uint32), au.reference(h, w, "defaults")[0])
    assert np.array_equal(_call(tr, 5, 5)[0].view(np.uint32), au.reference(5, 5, "defaults")[0])          # smaller
    planes, kw = au.call_args(h, w, "no_prev")
    tr.accumulate_plane(*planes, prev_focal=w, **kw)                 # fewer planes: less of the staging
    assert _live() == once
    d = [torch.from_numpy(a.copy()).cuda() for a in au.call_args(h, w, "defaults")[0]]
    torch.cuda.synchronize()
    tr.accumulate_plane_device(*d[:3], prim=d[3], prev=d[4], prev_focal=w)     # the device entry: nothing of the context's
    torch.cuda.synchronize()
    assert _live() == once
    _call(tr, 70, 200)                                               # larger than any before: the staging grows
    grown = _live()
    assert grown["allocations"] == once["allocations"] and grown["bytes"] == once["bytes"] + STAGING_PER_PIXEL * (70 * 200 - h * w)
    planes, kw = au.call_args(70, 200, "defaults")
    d = [torch.from_numpy(a.copy()).cuda() for a in planes]
    torch.cuda.synchronize()
    out = tr.accumulate_plane_device(*d[:3], prim=d[3], prev=d[4], prev_focal=200, **kw)   # a call is pending when the context goes
    tr.close()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), au.reference(70, 200, "defaults")[0])
    assert _live() == start
