"""-m gpu: what the variance-guided filter calls take of the device and give back (rt_debug_live_device_objects):
a context that only makes plain filter calls holds what it held before this entry family existed, 40 bytes per pixel of scratch;
the first variance call adds 12; only a call larger than any before it allocates; and after close() nothing is left."""
import gc

import pytest

import filter_variance_util as fv
from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    return abi.make_config(width=64, height=48, shadow_samples=4, **kw)


def _live():
    gc.collect()
    return rt.live_device_objects()


def test_what_the_family_holds_and_gives_back(scene):
    """A context that made only plain calls holds 40 bytes per pixel of filter scratch, as before; the first variance call adds
    12 (two variance planes and the thresholds); only a larger call allocates; close() returns everything."""
    import torch
    d = [torch.from_numpy(a.copy()).cuda() for a in fv.planes(37, 100)]
    big = [torch.from_numpy(a.copy()).cuda() for a in fv.planes(70, 200)]
    torch.cuda.synchronize()
    start = _live()
    tr = rt.RayTracer(_cfg(), scene)
    tr.render(rt.rotation_matrix(0.0, 0.0), DEFAULT_CAM, DEFAULT_LIGHT, focal_for(tr.cfg))
    without = _live()
    h, w = 37, 100
    tr.filter_plane_device(d[0], d[2], d[3])
    tr.filter_plane_device(d[0], d[2], d[3], passes=8)
    torch.cuda.synchronize()
    plain = _live()
    # the event, the counters (8 exported words and 64 partial sums of a 128-byte line each), the guides (32) and two planes (8)
    assert plain["events"] == without["events"] + 1 and plain["streams"] == without["streams"]
    assert plain["allocations"] == without["allocations"] + 3
    assert plain["bytes"] == without["bytes"] + 8 * (8 + 64 * 16) + 40 * h * w
    tr.filter_plane_variance_device(*d)
    torch.cuda.synchronize()
    both = _live()
    assert both["allocations"] == plain["allocations"] + 1 and both["bytes"] == plain["bytes"] + 12 * h * w
    assert both["events"] == plain["events"]
    tr.filter_plane_variance_device(*d, passes=1, out=d[0], out_variance=d[1])      # in place with one pass: through the scratch
    tr.filter_plane_device(d[0], d[2], d[3])
    torch.cuda.synchronize()
    assert _live() == both
    tr.filter_plane_variance_device(*big)                                            # larger than any before: the scratch grows
    torch.cuda.synchronize()
    grown = _live()
    assert grown["allocations"] == both["allocations"] and grown["bytes"] == both["bytes"] + 52 * (70 * 200 - h * w)
    tr.filter_plane_variance(*fv.planes(37, 100))                                    # the blocking entry: its staging, 48 bytes per pixel
    staged = _live()
    assert staged["allocations"] == grown["allocations"] + 1 and staged["bytes"] == grown["bytes"] + 48 * h * w
    tr.filter_plane_variance_device(*big)                                            # a call is pending when the context goes
    tr.close()
    torch.cuda.synchronize()
    gone = _live()
    assert gone == start
    if not any(start.values()):                                                      # no other context of this process is open:
        assert gone == {key: 0 for key in rt.LIVE_OBJECT_KEYS}                       # all zeros
