"""The variance-guided a-trous filter of include/uob_rt.h ("rt_filter_plane_variance") restated in numpy, one FP32 operation per
line of the definition, vectorised over the pixels (the taps stay a sequential loop: their order is part of the contract), on
top of tests/filter_util.py; a variance plane for filter_util's synthetic planes; the synthetic wall of the quality comparison;
and the constants of the device kernels, restated from uob_raytracer_amd/csrc/rt_host.h and rt_filter_variance.hip.  CPU only;
shared by the CPU and the GPU tests."""
import functools

import numpy as np

import filter_util as fu
from filter_util import F32, TAP, CENTRE_ONLY, QUIET_NAN, _shifted, guides_accept

BLUR = (F32(0.25), F32(0.125), F32(0.0625))          # the threshold's 3 x 3 kernel by |dx| + |dy|

# ---- the kernels' thresholds (rt_host.h kFilterVarianceMaxTiledSpacing, rt_filter_variance.hip TX / TY / kRowGroupsY) ---------
MAX_TILED_SPACING = 32              # variance passes of spacing <= 32 stage their taps in LDS, the others read the caches
ROW_GROUPS_Y = 32768                # row groups of a launch per grid.y; beyond that they continue in grid.z

PARAM_SETS = {
    "defaults": {},
    "sigma_1": {"sigma_value": 1.0},
    "eps_0.05": {"value_eps": 0.05},
    "reject_all": {"normal_min_dot": 2.0},
    "value_0.25": {"value_max_diff": 0.25},
}
DEFAULTS = dict(fu.DEFAULTS, sigma_value=4.0, value_eps=0.0)


def check_sizes():
    """filter_util's sizes lie where they claim to lie for the variance kernels too: the constants they are built from are
    the same.  (That the constants are the kernels' is tests/test_filter_variance_abi.py.)"""
    assert (MAX_TILED_SPACING, ROW_GROUPS_Y) == (fu.MAX_TILED_SPACING, fu.ROW_GROUPS_Y)
    fu.check_sizes()


def full_params(params):
    p = dict(DEFAULTS)
    p.update(params)
    return p


def thresholds(var, valid, sigma_value, value_eps):
    """T of one pass for every pixel (meaningful where valid)."""
    with np.errstate(all="ignore"):
        g = np.zeros_like(var)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                k = BLUR[abs(dx) + abs(dy)]
                vq, inside = _shifted(var, dy, dx, F32(0))
                okq, _ = _shifted(valid, dy, dx, False)
                c = np.where(inside & okq, vq, var)
                prod = k * c
                g = g + prod
        root = np.sqrt(g)
        scaled = F32(sigma_value) * root
        return scaled + F32(value_eps)


def filter_plane_variance(value, variance, position4, normal4, passes=5, normal_min_dot=0.9, plane_eps=0.01,
                          value_max_diff=float("inf"), sigma_value=4.0, value_eps=0.0, reverse=False):
    """-> (V_passes, Var_passes float32 [h, w], stats dict: accepted taps over valid centres and passes, valid pixels, (valid
    pixel, pass) pairs that kept their value, taps that passed tests 1 to 4 and failed test 5).  reverse visits the 25 taps in
    the opposite order (only to show that the order matters)."""
    v = np.ascontiguousarray(value, F32).copy()
    var = np.ascontiguousarray(variance, F32).copy()
    pos = np.ascontiguousarray(position4, F32)
    nrm = np.ascontiguousarray(normal4, F32)
    nmin, eps = F32(normal_min_dot), F32(plane_eps)
    with np.errstate(all="ignore"):
        valid = pos[..., 3] > F32(0)
        taps = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]
        if reverse:
            taps = taps[::-1]
        accepted_total = kept_total = stopped_total = 0
        for i in range(passes):
            s = 1 << i
            vmax = F32(value_max_diff) * F32(2.0 ** -i)
            T = thresholds(var, valid, sigma_value, value_eps)
            num = np.zeros_like(v)
            den = np.zeros_like(v)
            num2 = np.zeros_like(v)
            for dy, dx in taps:
                wt = TAP[abs(dx)] * TAP[abs(dy)]
                ww = wt * wt
                if dx == 0 and dy == 0:
                    vq, varq, acc = v, var, valid
                else:
                    vq, _ = _shifted(v, dy * s, dx * s, F32(0))
                    varq, _ = _shifted(var, dy * s, dx * s, F32(0))
                    four = guides_accept(pos, nrm, dy * s, dx * s, nmin, eps)
                    dv = vq - v
                    adv = np.abs(dv)
                    four = four & (adv <= vmax)
                    acc = four & (adv <= T)
                    stopped_total += int((four & ~acc).sum())
                prod = wt * vq
                prod2 = ww * varq
                num = np.where(acc, num + prod, num)
                den = np.where(acc, den + wt, den)
                num2 = np.where(acc, num2 + prod2, num2)
                accepted_total += int(acc.sum())
            kept = valid & (den == CENTRE_ONLY)
            kept_total += int(kept.sum())
            quot = num / den
            dd = den * den
            quot2 = num2 / dd
            quot_bits = np.where(np.isnan(quot), QUIET_NAN, quot.view(np.uint32))
            quot2_bits = np.where(np.isnan(quot2), QUIET_NAN, quot2.view(np.uint32))
            take = valid & ~kept
            v = np.where(take, quot_bits, v.view(np.uint32)).astype(np.uint32).view(F32)
            var = np.where(take, quot2_bits, var.view(np.uint32)).astype(np.uint32).view(F32)
    return v, var, {"accepted_taps": accepted_total, "valid_pixels": int(valid.sum()), "kept": kept_total,
                    "variance_stopped": stopped_total}


def make_variance(h, w, seed=0):
    """A variance plane for filter_util.planes(h, w): uniform in [0, 0.09) (standard deviations up to 0.3 for values in
    [0, 1)), 5 % exact zeros, about 0.5 % each of NaN and of -0.01, and a few +INF."""
    rng = np.random.default_rng(2000 + seed)
    var = (rng.random((h, w), dtype=F32) * F32(0.09)).astype(F32)
    r = rng.random((h, w))
    var[r < 0.05] = 0.0
    var[(r >= 0.05) & (r < 0.055)] = np.nan
    var[(r >= 0.055) & (r < 0.06)] = -0.01
    for _ in range(min(3, (h * w) // 40)):
        var.flat[int(rng.integers(h * w))] = np.inf
    return np.ascontiguousarray(var)


@functools.lru_cache(maxsize=None)
def planes(h, w):
    """(value, variance, position4, normal4), read-only and computed once per process."""
    value, pos, nrm = fu.planes(h, w)
    var = make_variance(h, w)
    var.setflags(write=False)
    return value, var, pos, nrm


@functools.lru_cache(maxsize=None)
def reference(h, w, passes, param_set):
    """The restatement on planes(h, w), computed once per process and left unchanged: (value bits, variance bits uint32 [h, w],
    stats)."""
    value, var, pos, nrm = planes(h, w)
    p = full_params(PARAM_SETS[param_set])
    p["passes"] = passes
    out, ovar, stats = filter_plane_variance(value, var, pos, nrm, **p)
    bits, vbits = out.view(np.uint32).copy(), ovar.view(np.uint32).copy()
    bits.setflags(write=False)
    vbits.setflags(write=False)
    return bits, vbits, stats


@functools.lru_cache(maxsize=None)
def check_generator():
    """The planes make the comparison sharp, at 70 x 200, 5 passes, sigma_value 4: more than 5 taps are accepted per valid pixel
    and pass, the variance stop alone rejects more than 20 % of the taps that pass tests 1 to 4, and reversing the tap order
    changes more than 20 % of the value bits and more than 5 % of the variance bits."""
    h, w = 70, 200
    value, var, pos, nrm = planes(h, w)
    bits, vbits, stats = reference(h, w, 5, "defaults")
    per_pixel = stats["accepted_taps"] / (5.0 * stats["valid_pixels"])
    assert per_pixel > 5.0, per_pixel
    # the taps that pass tests 1 to 4: the accepted ones without the centres, and the stopped ones
    four = stats["accepted_taps"] - 5 * stats["valid_pixels"] + stats["variance_stopped"]
    stopped = stats["variance_stopped"] / float(four)
    assert stopped > 0.20, stopped
    rev, rvar, _ = filter_plane_variance(value, var, pos, nrm, reverse=True, **full_params({}))
    changed = float(np.mean(rev.view(np.uint32) != bits))
    vchanged = float(np.mean(rvar.view(np.uint32) != vbits))
    assert changed > 0.20, changed
    assert vchanged > 0.05, vchanged
    assert np.isnan(var).mean() > 0.002 and (var < 0).mean() > 0.002 and np.isinf(var).any() and (var == 0).mean() > 0.03
    return per_pixel, stopped, changed, vchanged


def same_bits(a, b):
    return fu.same_bits(a, b)


# ---- the synthetic wall of the quality comparison ---------------------------------------------------------------------------
def make_wall(n=96, frames=8, samples=4, penumbra=6.0, seed=7):
    """A planar wall of n x n valid pixels with a slanted penumbra `penumbra` pixels wide: the true visibility ramp, the mean of
    `frames` frames of `samples` Bernoulli samples each, and the frames' variance m2 - mean^2 (what rt_accumulate_plane keeps).
    -> (truth, value, variance float32 [n, n], position4, normal4 float32 [n, n, 4])"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    edge = 0.35 * n + 0.3 * yy                                   # the slanted middle of the penumbra
    truth = np.clip((xx - edge) / penumbra + 0.5, 0.0, 1.0).astype(F32)
    per_frame = (rng.random((frames, samples, n, n)) < truth).mean(axis=1).astype(F32)
    mean = per_frame.mean(axis=0).astype(F32)
    m2 = (per_frame * per_frame).mean(axis=0).astype(F32)
    var = np.maximum(m2 - mean * mean, F32(0)).astype(F32)
    pos = np.zeros((n, n, 4), F32)
    pos[..., 0], pos[..., 1], pos[..., 3] = xx * 0.01, yy * 0.01, 1.0
    nrm = np.zeros((n, n, 4), F32)
    nrm[..., 2] = 1.0
    return truth, mean, var, pos, nrm


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
