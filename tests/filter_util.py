"""The a-trous filter of include/uob_rt.h ("rt_filter_plane") restated in numpy, one FP32 operation per line of the definition,
vectorised over the pixels (the 25 taps stay a sequential loop: their order is part of the contract); a generator of synthetic
planes that exercises every edge stop; and the sizes at which the device kernels take another path, restated from
uob_raytracer_amd/csrc/rt_host.h and rt_filter.hip.  CPU only; shared by the CPU and the GPU tests."""
import functools

import numpy as np

F32 = np.float32
TAP = (F32(0.375), F32(0.25), F32(0.0625))          # h[|d|]: 3/8, 1/4, 1/16
CENTRE_ONLY = F32(0.140625)                          # 9/64: the denominator when only the centre was accepted
QUIET_NAN = np.uint32(0x7FC00000)

# ---- the kernels' thresholds (rt_host.h kFilterTX / kFilterTY / kFilterMaxTiledSpacing, rt_filter.hip kRowGroupsY) ----------
FILTER_TX, FILTER_TY = 64, 4        # a tile: 64 contiguous pixels of 4 rows (tiled form: rows s apart)
MAX_TILED_SPACING = 32              # passes of spacing <= 32 stage their taps in LDS, the others read the caches
ROW_GROUPS_Y = 32768                # row groups of a launch per grid.y; beyond that they continue in grid.z

PARAM_SETS = {
    "defaults": {},
    "value_0.25": {"value_max_diff": 0.25},
    "reject_all": {"normal_min_dot": 2.0},
    "plane_eps_0": {"plane_eps": 0.0},
}
DEFAULTS = {"passes": 5, "normal_min_dot": 0.9, "plane_eps": 0.01, "value_max_diff": float("inf")}

# (height, width) of the CPU comparison: one pixel, every later tap outside, one row, one column, odd, the triage size
SIZES = [(1, 1), (5, 5), (1, 200), (200, 1), (37, 100), (70, 200)]
# beyond a tile by one pixel in each dimension; by one tile plus one
TILE_SIZES = [(FILTER_TY + 1, FILTER_TX + 1), (2 * FILTER_TY + 1, 2 * FILTER_TX + 1)]
# more row groups than one grid.y holds, in the tiled form (pass 0) and in the direct form (pass 6: spacing 64)
TALL_SIZE, TALL_PASSES = (FILTER_TY * ROW_GROUPS_Y + 2 * FILTER_TY + 1, 3), 7


def check_sizes():
    """The sizes above lie where they claim to lie, whatever the constants become.  (That the constants are the kernels' is
    tests/test_filter_abi.py::test_the_restated_thresholds_are_the_kernels.)"""
    for (h, w), k in zip(TILE_SIZES, (1, 2)):
        assert h == k * FILTER_TY + 1 and w == k * FILTER_TX + 1
    h, w = TALL_SIZE
    # row groups of a launch: the direct form takes FILTER_TY adjacent rows per group; the tiled form at spacing s has s
    # residue classes of ceil(ceil(h / s) / FILTER_TY) groups each, which at pass 0 (s = 1) is the same number
    groups_direct = -(-h // FILTER_TY)
    groups_tiled_pass0 = 1 * -(-(-(-h // 1)) // FILTER_TY)
    assert groups_direct > ROW_GROUPS_Y and groups_tiled_pass0 > ROW_GROUPS_Y
    assert MAX_TILED_SPACING >= 1                            # pass 0 of the tall plane runs in the tiled form
    assert (1 << (TALL_PASSES - 1)) > MAX_TILED_SPACING      # and its last pass in the direct form
    # 1, 5 and 8 passes: the first is tiled, the last of 8 is direct
    assert 1 <= MAX_TILED_SPACING < (1 << 7)
    # 37 x 100 and the smaller ones are narrower and lower than the halo of the largest spacing, 2 * 128 pixels
    assert all(max(size) < 2 * 128 for size in SIZES[:5])


def full_params(params):
    p = dict(DEFAULTS)
    p.update(params)
    return p


def _shifted(a, oy, ox, fill):
    """out[y, x] = a[y + oy, x + ox] where that lies inside the plane, else fill; and the mask of 'inside'."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    inside = np.zeros((h, w), bool)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return out, inside


def guides_accept(pos, nrm, oy, ox, nmin, eps):
    """Conditions 1 to 3 of the tap at offset (oy, ox) for every centre pixel: the mask of (valid centre, tap inside and valid,
    normals agree, tap on the centre's plane).  They depend on the guides alone, so they are the same in every pass that has
    this offset."""
    with np.errstate(all="ignore"):
        valid = pos[..., 3] > F32(0)
        pq, inside = _shifted(pos, oy, ox, F32(0))
        nq, _ = _shifted(nrm, oy, ox, F32(0))
        acc = valid & inside & (pq[..., 3] > F32(0))
        a = nrm[..., 0] * nq[..., 0]
        b = nrm[..., 1] * nq[..., 1]
        c = nrm[..., 2] * nq[..., 2]
        nd = (a + b) + c
        acc = acc & (nd >= nmin)
        d0 = pq[..., 0] - pos[..., 0]
        d1 = pq[..., 1] - pos[..., 1]
        d2 = pq[..., 2] - pos[..., 2]
        a = nrm[..., 0] * d0
        b = nrm[..., 1] * d1
        c = nrm[..., 2] * d2
        pd = (a + b) + c
        return acc & (np.abs(pd) <= eps)


def untouched_region(mask, pos, nrm, passes=5, normal_min_dot=0.9, plane_eps=0.01):
    """The valid pixels of `mask` all of whose guide-accepted taps, pass after pass, lie in the region too: where the values of
    `mask` are all 1.0f (or all 0.0f) and value_max_diff is +INF, the filter must leave exactly that value there."""
    region = mask & (pos[..., 3] > F32(0))
    for i in range(passes):
        s = 1 << i
        nxt = region.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx or dy:
                    acc = guides_accept(pos, nrm, dy * s, dx * s, F32(normal_min_dot), F32(plane_eps))
                    tap_in, _ = _shifted(region, dy * s, dx * s, False)
                    nxt &= ~acc | tap_in
        region = nxt
    return region


def filter_plane(value, position4, normal4, passes=5, normal_min_dot=0.9, plane_eps=0.01, value_max_diff=float("inf"),
                 reverse=False):
    """-> (V_passes float32 [h, w], stats dict: accepted taps over valid centres and passes, valid pixels, (valid pixel, pass)
    pairs that kept their value).  reverse visits the taps in the opposite order (only to show that the order matters)."""
    v = np.ascontiguousarray(value, F32).copy()
    pos = np.ascontiguousarray(position4, F32)
    nrm = np.ascontiguousarray(normal4, F32)
    nmin, eps = F32(normal_min_dot), F32(plane_eps)
    with np.errstate(all="ignore"):
        valid = pos[..., 3] > F32(0)
        taps = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]
        if reverse:
            taps = taps[::-1]
        accepted_total = kept_total = 0
        for i in range(passes):
            s = 1 << i
            vmax = F32(value_max_diff) * F32(2.0 ** -i)
            num = np.zeros_like(v)
            den = np.zeros_like(v)
            for dy, dx in taps:
                wt = TAP[abs(dx)] * TAP[abs(dy)]
                if dx == 0 and dy == 0:
                    vq, acc = v, valid
                else:
                    vq, _ = _shifted(v, dy * s, dx * s, F32(0))
                    acc = guides_accept(pos, nrm, dy * s, dx * s, nmin, eps)
                    dv = vq - v
                    acc = acc & (np.abs(dv) <= vmax)
                prod = wt * vq
                num = np.where(acc, num + prod, num)
                den = np.where(acc, den + wt, den)
                accepted_total += int(acc.sum())
            kept = valid & (den == CENTRE_ONLY)
            kept_total += int(kept.sum())
            quot = num / den
            quot_bits = np.where(np.isnan(quot), QUIET_NAN, quot.view(np.uint32))
            take = valid & ~kept
            v = np.where(take, quot_bits, v.view(np.uint32)).astype(np.uint32).view(F32)
    return v, {"accepted_taps": accepted_total, "valid_pixels": int(valid.sum()), "kept": kept_total}


def make_planes(h, w, seed=0):
    """Synthetic planes: three planar patches with different normals that meet at a straight and at a diagonal border (one of
    them with normals that are not unit length), positions a little off their planes, 3 % invalid pixels (w = 0, negative or
    NaN), values uniform in [0, 1) with 1 % NaN (two payloads) and a few +-INF in the corner patch.  -> value [h, w], position4, normal4 [h, w, 4]"""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u, t = (xx * 0.01).astype(F32), (yy * 0.01).astype(F32)
    patch = np.where(xx < 0.45 * w, 0, np.where((xx - 0.45 * w) + yy < 0.6 * max(h, w), 1, 2))
    normals = np.array([[0.6, 0.0, 0.8], [-1.0, 0.0, 0.0], [0.0, 1.25, 0.0]], F32)     # (the last: |N|^2 = 1.5625, above 0.9 and below 2)
    axis_u = np.array([[0.8, 0.0, -0.6], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], F32)
    axis_t = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], F32)
    # off the plane by up to 0.006 (so plane_eps = 0.01 rejects a few pairs), and exactly on it for half of the pixels (so
    # plane_eps = 0 accepts some pairs of the two axis-aligned patches)
    off = np.where(rng.random((h, w)) < 0.5, 0.0, rng.uniform(-0.006, 0.006, (h, w))).astype(F32)
    pos = np.zeros((h, w, 4), F32)
    nrm = np.zeros((h, w, 4), F32)
    for k in range(3):
        nrm[..., k] = normals[patch, k]
        unit = normals[patch, k] / np.linalg.norm(normals[patch], axis=-1).astype(F32)
        pos[..., k] = u * axis_u[patch, k] + t * axis_t[patch, k] + off * unit
    pos[..., 3] = 1.0
    nrm[..., 3] = rng.uniform(-5, 5, (h, w)).astype(F32)          # the pad of a guide is never looked at
    bad = rng.random((h, w)) < 0.03
    pos[..., 3] = np.where(bad, rng.choice(np.array([0.0, 0.0, -1.0, np.nan], F32), (h, w)), pos[..., 3])
    value = rng.random((h, w), dtype=F32)
    bits = value.view(np.uint32).copy()
    r = rng.random((h, w))
    bits[r < 0.005] = 0x7FC00123
    bits[(r >= 0.005) & (r < 0.01)] = 0xFFA00001
    value = bits.view(F32).copy()
    # (at value_max_diff = +INF an infinity is accepted by every neighbour of its patch and floods it pass by pass, so the
    # infinities go into the small corner patch where there is one: the other patches keep finite, order-sensitive sums)
    where = np.flatnonzero(patch == 2) if (patch == 2).any() else np.arange(h * w)
    for j in range(min(4, (h * w) // 40)):
        value.flat[int(rng.choice(where))] = np.inf if j % 2 == 0 else -np.inf
    return np.ascontiguousarray(value), np.ascontiguousarray(pos), np.ascontiguousarray(nrm)


@functools.lru_cache(maxsize=None)
def planes(h, w):
    value, pos, nrm = make_planes(h, w)
    for a in (value, pos, nrm):
        a.setflags(write=False)
    return value, pos, nrm


@functools.lru_cache(maxsize=None)
def reference(h, w, passes, param_set):
    """The restatement on planes(h, w), computed once per process and left unchanged: (bits uint32 [h, w], stats)."""
    value, pos, nrm = planes(h, w)
    p = full_params(PARAM_SETS[param_set])
    p["passes"] = passes
    out, stats = filter_plane(value, pos, nrm, **p)
    bits = out.view(np.uint32).copy()
    bits.setflags(write=False)
    return bits, stats


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@functools.lru_cache(maxsize=None)
def check_generator():
    """The generator's planes make the comparison sharp: at the defaults more than 10 taps are accepted per valid pixel and
    pass on average, and reversing the tap order changes the bits of more than 20 % of the pixels."""
    h, w = 70, 200
    value, pos, nrm = planes(h, w)
    bits, stats = reference(h, w, 5, "defaults")
    per_pixel = stats["accepted_taps"] / (5.0 * stats["valid_pixels"])
    assert per_pixel > 10.0, per_pixel
    rev, _ = filter_plane(value, pos, nrm, reverse=True, **DEFAULTS)
    changed = float(np.mean(rev.view(np.uint32) != bits))
    assert changed > 0.20, changed
    assert 0.01 < 1.0 - stats["valid_pixels"] / float(h * w) < 0.06
    assert np.isnan(value).mean() > 0.004 and np.isinf(value).any()
    return per_pixel, changed
