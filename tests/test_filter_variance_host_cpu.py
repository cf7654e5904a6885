"""CPU: rt_filter_plane_variance_host, the host statement of the variance-guided a-trous filter, equals the numpy restatement of
tests/filter_variance_util.py bit for bit, on value and variance, on every size, pass count and parameter set of the
comparison, in place and out of place, with and without out_variance; what the header says follows exactly does follow; the
restatement's counters are hand counts on a small plane; and on a synthetic penumbra the filter beats the unfiltered estimate,
which beats the plain filter."""
import numpy as np
import pytest

import filter_util as fu
import filter_variance_util as fv
from uob_raytracer_amd import runtime as rt


def _params(passes, param_set):
    p = fv.full_params(fv.PARAM_SETS[param_set])
    p["passes"] = passes
    return p


def test_the_generator_keeps_the_comparison_sharp():
    per_pixel, stopped, changed, vchanged = fv.check_generator()
    print("accepted taps per valid pixel and pass %.1f, stopped by the variance alone %.1f %%, bits that depend on the tap order: "
          "value %.1f %%, variance %.1f %%" % (per_pixel, 100 * stopped, 100 * changed, 100 * vchanged))
    fv.check_sizes()


@pytest.mark.parametrize("param_set", list(fv.PARAM_SETS))
@pytest.mark.parametrize("passes", [1, 5, 8])
@pytest.mark.parametrize("size", fu.SIZES + fu.TILE_SIZES, ids=lambda s: "%dx%d" % s)
def test_host_statement_equals_the_restatement(size, passes, param_set):
    h, w = size
    value, var, pos, nrm = fv.planes(h, w)
    want, vwant, _ = fv.reference(h, w, passes, param_set)
    p = _params(passes, param_set)
    got, vgot = rt.filter_plane_variance_host(value, var, pos, nrm, **p)
    assert np.array_equal(got.view(np.uint32), want) and np.array_equal(vgot.view(np.uint32), vwant)
    if param_set == "reject_all":                                   # every tap rejected: both inputs, bit for bit
        assert np.array_equal(want, value.view(np.uint32)) and np.array_equal(vwant, var.view(np.uint32))
    # without out_variance
    got, none = rt.filter_plane_variance_host(value, var, pos, nrm, want_variance=False, **p)
    assert none is None and np.array_equal(got.view(np.uint32), want)
    # both in place; the value alone in place; the variance alone in place
    v, r = value.copy(), var.copy()
    a, b = rt.filter_plane_variance_host(v, r, pos, nrm, out=v, out_variance=r, **p)
    assert a is v and b is r
    assert np.array_equal(v.view(np.uint32), want) and np.array_equal(r.view(np.uint32), vwant)
    v = value.copy()
    _, vgot = rt.filter_plane_variance_host(v, var, pos, nrm, out=v, **p)
    assert np.array_equal(v.view(np.uint32), want) and np.array_equal(vgot.view(np.uint32), vwant)
    r = var.copy()
    got, _ = rt.filter_plane_variance_host(value, r, pos, nrm, out_variance=r, **p)
    assert np.array_equal(got.view(np.uint32), want) and np.array_equal(r.view(np.uint32), vwant)


@pytest.mark.parametrize("passes", [1, 5, 8])
@pytest.mark.parametrize("param_set", list(fu.PARAM_SETS))
def test_an_infinite_value_eps_gives_the_plain_filters_bits(param_set, passes):
    """value_eps = +INF with a finite sigma_value and finite non-negative variances: T is +INF, test 5 accepts what test 4 did."""
    h, w = 70, 200
    value, pos, nrm = fu.planes(h, w)
    var = np.abs(np.nan_to_num(fv.planes(h, w)[1], nan=0.03, posinf=0.07)).astype(np.float32)
    assert np.isfinite(var).all() and (var >= 0).all() and (var == 0).any()
    p = fu.full_params(fu.PARAM_SETS[param_set])
    p["passes"] = passes
    plain = rt.filter_plane_host(value, pos, nrm, **p)
    assert np.array_equal(plain.view(np.uint32), fu.reference(h, w, passes, param_set)[0])
    for sigma in (0.0, 4.0):
        got, _ = rt.filter_plane_variance_host(value, var, pos, nrm, value_eps=np.inf, sigma_value=sigma, **p)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))
        ref, _, stats = fv.filter_plane_variance(value, var, pos, nrm, value_eps=np.inf, sigma_value=sigma, **p)
        assert np.array_equal(ref.view(np.uint32), plain.view(np.uint32)) and stats["variance_stopped"] == 0


@pytest.mark.parametrize("passes", [1, 5, 8])
@pytest.mark.parametrize("fill", [1.0, 0.0])
def test_a_clean_plane_keeps_its_value_and_its_zero_variance(fill, passes):
    """Valid pixels of value 1.0f (or 0.0f) and variance +0 keep both at value_eps = 0: test 5 accepts a difference of 0."""
    _, pos, nrm = fu.planes(37, 100)
    value = np.full((37, 100), fill, np.float32)
    var = np.zeros((37, 100), np.float32)
    for name in ("defaults", "sigma_1", "value_0.25"):
        p = _params(passes, name)
        assert p["value_eps"] == 0.0
        out, ovar = rt.filter_plane_variance_host(value, var, pos, nrm, **p)
        assert np.array_equal(out.view(np.uint32), value.view(np.uint32))
        assert np.array_equal(ovar.view(np.uint32), var.view(np.uint32))
        ref, rvar, stats = fv.filter_plane_variance(value, var, pos, nrm, **p)
        assert fu.same_bits(ref, value.view(np.uint32)) and fu.same_bits(rvar, var.view(np.uint32))
        assert stats["variance_stopped"] == 0 and stats["accepted_taps"] > passes * stats["valid_pixels"]


def test_rejecting_every_tap_returns_both_inputs():
    value, var, pos, nrm = fv.planes(37, 100)
    unit = nrm.copy()
    unit[..., :3] = [0.0, 0.0, 1.0]
    out, ovar = rt.filter_plane_variance_host(value, var, pos, unit, normal_min_dot=2.0)
    assert np.array_equal(out.view(np.uint32), value.view(np.uint32)) and np.array_equal(ovar.view(np.uint32), var.view(np.uint32))


def test_counters_of_the_restatement_on_a_hand_counted_plane():
    """5 x 5, one plane, every pixel valid, one pass.  The left three columns hold 0, the right two hold 1; the variance is 0 but
    for 0.01 in column 2 of row 2, whose blur reaches the 3 x 3 block around it."""
    pos = np.zeros((5, 5, 4), np.float32)
    pos[..., 3] = 1.0
    nrm = np.zeros((5, 5, 4), np.float32)
    nrm[..., 2] = 1.0
    value = np.zeros((5, 5), np.float32)
    value[:, 3:] = 1.0
    var = np.zeros((5, 5), np.float32)
    var[2, 2] = 0.01
    # guides accept every tap inside the plane: per pixel (columns inside) x (rows inside)
    inside = np.array([3, 4, 5, 4, 3])
    four_taps = int(np.outer(inside, inside).sum())                               # 19 * 19 = 361, the centres included
    # sigma_value 4: T = 4 * sqrt(k * 0.01) is 0.2 at (2, 2), 0.141 beside it, 0.1 at the block's corners, 0 elsewhere: below 1
    # everywhere, so a tap is accepted iff its value equals the centre's: same side of the step
    same_side = np.array([min(x + 2, 2) - max(x - 2, 0) + 1 for x in range(3)] + [min(x + 2, 4) - max(x - 2, 3) + 1 for x in (3, 4)])
    assert list(same_side) == [3, 3, 3, 2, 2]                                     # tap columns of column x on its own side of the step
    accepted = int(np.outer(inside, same_side).sum())                             # rows inside x columns on the same side
    out, ovar, stats = fv.filter_plane_variance(value, var, pos, nrm, passes=1, sigma_value=4.0)
    assert stats == {"accepted_taps": accepted, "valid_pixels": 25, "kept": 0, "variance_stopped": four_taps - accepted}
    assert (accepted, four_taps - accepted) == (19 * 13, 19 * 6)
    assert np.array_equal(out, value)                                             # equal values average to themselves
    # sigma_value 100: T = 5 at (2, 2), 3.5 / 2.5 around it: those nine centres accept across the step, the others do not
    _, _, wide = fv.filter_plane_variance(value, var, pos, nrm, passes=1, sigma_value=100.0)
    block = sum(int(inside[y]) * int(inside[x] - same_side[x]) for y in (1, 2, 3) for x in (1, 2, 3))
    assert block == (4 + 5 + 4) * (1 + 2 + 2)
    assert wide["variance_stopped"] == four_taps - accepted - block and wide["accepted_taps"] == accepted + block
    # a NaN threshold (a negative variance under the blur) keeps the pixel: only (2, 2) sees g < 0 when its neighbours are invalid
    lone = pos.copy()
    lone[..., 3] = 0.0
    lone[2, 2, 3] = lone[2, 4, 3] = 1.0
    neg = np.full((5, 5), -0.01, np.float32)
    out, ovar, kept = fv.filter_plane_variance(value, neg, lone, nrm, passes=1)
    assert kept == {"accepted_taps": 2, "valid_pixels": 2, "kept": 2, "variance_stopped": 2}
    assert fu.same_bits(out, value.view(np.uint32)) and fu.same_bits(ovar, neg.view(np.uint32))
    host, hvar = rt.filter_plane_variance_host(value, neg, lone, nrm, passes=1)
    assert fu.same_bits(host, value.view(np.uint32)) and fu.same_bits(hvar, neg.view(np.uint32))


def test_the_filter_beats_the_unfiltered_estimate_on_a_synthetic_penumbra():
    """A planar wall with a slanted 6-pixel penumbra, the mean of 8 frames of 4 Bernoulli samples, the frames' variance:
    RMS(variance-guided, sigma_value 4) < RMS(unfiltered) < RMS(rt_filter_plane's defaults)."""
    truth, value, var, pos, nrm = fv.make_wall()
    new, nvar = rt.filter_plane_variance_host(value, var, pos, nrm, sigma_value=4.0)
    plain = rt.filter_plane_host(value, pos, nrm)
    e_new, e_raw, e_plain = fv.rms(new, truth), fv.rms(value, truth), fv.rms(plain, truth)
    print("RMS against the true ramp: variance-guided %.4f, unfiltered %.4f, rt_filter_plane defaults %.4f" % (e_new, e_raw, e_plain))
    assert e_new < e_raw < e_plain
    assert (nvar[np.isfinite(nvar)] >= 0).all() and nvar.mean() < var.mean()     # and the variance estimate shrinks with it


def test_a_wrong_tap_order_is_seen():
    value, var, pos, nrm = fv.planes(70, 200)
    want, vwant, _ = fv.reference(70, 200, 5, "defaults")
    rev, rvar, _ = fv.filter_plane_variance(value, var, pos, nrm, reverse=True, **fv.full_params({}))
    got, vgot = rt.filter_plane_variance_host(value, var, pos, nrm)
    assert np.array_equal(got.view(np.uint32), want) and not np.array_equal(rev.view(np.uint32), want)
    assert np.array_equal(vgot.view(np.uint32), vwant) and not np.array_equal(rvar.view(np.uint32), vwant)
