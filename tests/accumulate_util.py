"""The temporal reprojection of include/uob_rt.h ("rt_accumulate_plane") restated in numpy, one FP32 operation per line of the
definition, vectorised over the pixels (the four taps stay a sequential loop: their order is part of the contract); a generator
of synthetic view pairs that exercises every acceptance test; and the kernel's tile constants, restated from
uob_raytracer_amd/csrc/rt_host.h and rt_accumulate.hip.  CPU only; shared by the CPU and the GPU tests."""
import functools

import numpy as np

F32 = np.float32
QUIET_NAN = np.uint32(0x7FC00000)
WORDS = 12                                   # float32 words of one rt_history_texel
MEAN, M2, COUNT, PRIM = 3, 7, 8, 9           # position 0..2 | mean, normal 4..6 | m2, count, the int32 bits of prim, 0, 0

# ---- the kernel's thresholds (rt_host.h kFilterTX / kFilterTY, rt_accumulate.hip kRowGroupsY) ------------------------------
TILE_TX, TILE_TY = 64, 4            # a workgroup: 64 contiguous pixels of 4 adjacent rows
ROW_GROUPS_Y = 32768                # row groups of a launch per grid.y; beyond that they continue in grid.z

DEFAULTS = {"normal_min_dot": 0.9, "plane_eps": 0.01, "max_history": 32}
# name -> (overrides of DEFAULTS, with the prim plane, with a history)
PARAM_SETS = {
    "defaults": ({}, True, True),
    "reject_all": ({"normal_min_dot": 2.0}, True, True),
    "plane_eps_0": ({"plane_eps": 0.0}, True, True),
    "max_history_1": ({"max_history": 1}, True, True),
    "max_history_4": ({"max_history": 4}, True, True),
    "no_prim": ({}, False, True),
    "no_prev": ({}, True, False),
}

# (height, width) of the CPU comparison: one pixel, a few, one row, one column, odd, the triage size
SIZES = [(1, 1), (5, 5), (1, 200), (200, 1), (37, 100), (70, 200)]
# beyond a tile by one pixel in each dimension; by one tile plus one
TILE_SIZES = [(TILE_TY + 1, TILE_TX + 1), (2 * TILE_TY + 1, 2 * TILE_TX + 1)]
# more row groups than one grid.y holds
TALL_SIZE = (TILE_TY * ROW_GROUPS_Y + 2 * TILE_TY + 1, 3)


def check_sizes():
    """The sizes above lie where they claim to lie, whatever the constants become.  (That the constants are the kernel's is
    tests/test_accumulate_abi.py::test_the_restated_tile_is_the_kernels.)"""
    for (h, w), k in zip(TILE_SIZES, (1, 2)):
        assert h == k * TILE_TY + 1 and w == k * TILE_TX + 1
    assert -(-TALL_SIZE[0] // TILE_TY) > ROW_GROUPS_Y


def _quiet(a):
    """NaNs as the quiet NaN 0x7FC00000, everything else its own bits."""
    bits = a.view(np.uint32).copy()
    bits[a != a] = QUIET_NAN
    return bits.view(F32)


def accumulate(value, position4, normal4, prim, prev, prev_rot, prev_cam, prev_focal_px, normal_min_dot=0.9, plane_eps=0.01,
               max_history=32, reverse=False, tap_list=None):
    """-> (next float32 [h, w, 12], mean [h, w], variance [h, w], stats dict as rt_debug_accumulate_stats counts them, the
    accepted taps per pixel).  reverse visits the taps in the opposite order (only to show that the order matters); tap_list,
    a list, receives (row, column, accepted, inside) of each of the four taps: the coordinates clipped to the plane, and whether the
    pixel has a candidate and this tap of it lies inside the plane."""
    v = np.ascontiguousarray(value, F32)
    pos = np.ascontiguousarray(position4, F32)
    nrm = np.ascontiguousarray(normal4, F32)
    h, w = v.shape
    rot = np.asarray(prev_rot, F32)
    cam = np.asarray(prev_cam, F32)
    focal, nmin, eps = F32(prev_focal_px), F32(normal_min_dot), F32(plane_eps)
    valid = pos[..., 3] > F32(0)
    P = [pos[..., k] for k in range(3)]
    N = [nrm[..., k] for k in range(3)]
    with np.errstate(all="ignore"):
        vv = v * v
        num = np.zeros((h, w), F32)
        num2 = np.zeros((h, w), F32)
        den = np.zeros((h, w), F32)
        cmin = np.full((h, w), np.inf, F32)
        taps = np.zeros((h, w), np.int64)
        nocand = np.zeros((h, w), bool)
        if prev is not None:
            d = [P[k] - cam[k] for k in range(3)]
            q = []
            for j in range(3):
                a = d[0] * rot[j]
                b = d[1] * rot[4 + j]
                c = d[2] * rot[8 + j]
                q.append((a + b) + c)
            tx = q[0] * focal
            ty = q[1] * focal
            ux = tx / q[2]
            uy = ty / q[2]
            fx = ux + F32(0.5) * F32(w)
            fy = uy + F32(0.5) * F32(h)
            cand = valid & (q[2] > F32(0)) & (fx >= F32(-1)) & (fx < F32(w)) & (fy >= F32(-1)) & (fy < F32(h))
            nocand = valid & ~cand
            xf = np.floor(fx)
            yf = np.floor(fy)
            ax = fx - xf
            ay = fy - yf
            x0 = np.where(cand, xf, F32(0)).astype(np.int64)
            y0 = np.where(cand, yf, F32(0)).astype(np.int64)
            bx = F32(1) - ax
            by = F32(1) - ay
            order = [(0, 0), (0, 1), (1, 0), (1, 1)]            # (j, i): j outer, i inner, both ascending
            for j, i in (reversed(order) if reverse else order):
                qx, qy = x0 + i, y0 + j
                wt = (ax if i else bx) * (ay if j else by)
                inside = cand & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                acc = inside & (wt > F32(0))
                r = prev[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
                acc &= r[..., COUNT] > F32(0)
                if prim is not None:
                    acc &= r[..., PRIM].view(np.int32) == prim
                a = N[0] * r[..., 4]
                b = N[1] * r[..., 5]
                c = N[2] * r[..., 6]
                nd = (a + b) + c
                acc &= nd >= nmin
                e = [r[..., k] - P[k] for k in range(3)]
                a = N[0] * e[0]
                b = N[1] * e[1]
                c = N[2] * e[2]
                pd = (a + b) + c
                acc &= np.abs(pd) <= eps
                t = wt * r[..., MEAN]
                num = np.where(acc, num + t, num)
                t = wt * r[..., M2]
                num2 = np.where(acc, num2 + t, num2)
                den = np.where(acc, den + wt, den)
                cmin = np.where(acc & (r[..., COUNT] < cmin), r[..., COUNT], cmin)
                taps += acc
                if tap_list is not None:
                    tap_list.append((np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1), acc, inside))
        found = taps > 0
        mp = num / den
        sp = num2 / den
        nmax = F32(max_history - 1)
        n = np.where(cmin < nmax, cmin, nmax) + F32(1)
        a = F32(1) / n
        t = v - mp
        t = a * t
        mean5 = _quiet(mp + t)
        t = vv - sp
        t = a * t
        m25 = _quiet(sp + t)
        mean = np.where(found, mean5.view(np.uint32), v.view(np.uint32)).view(F32)       # a first frame: the value's own bits
        m2 = np.where(found, m25.view(np.uint32), _quiet(vv).view(np.uint32)).view(F32)
        count = np.where(found, n, np.where(valid, F32(1), F32(0))).astype(F32)
        t = mean * mean
        t = m2 - t
        var = np.where(t > F32(0), t, F32(0)).astype(F32)
    nxt = np.zeros((h, w, WORDS), F32)
    nxt[..., 0:3] = pos[..., 0:3]
    nxt[..., 4:7] = nrm[..., 0:3]
    out = nxt.view(np.uint32)
    out[..., MEAN] = mean.view(np.uint32)
    out[..., M2] = m2.view(np.uint32)
    out[..., COUNT] = count.view(np.uint32)
    out[..., PRIM] = (prim if prim is not None else np.full((h, w), -1, np.int32)).view(np.uint32)
    stats = {"pixels": h * w, "valid_pixels": int(valid.sum()), "found_history": int(found.sum()), "accepted_taps": int(taps.sum()),
             "no_candidate": int(nocand.sum())}
    return nxt, mean, var, stats, taps


# ---- synthetic view pairs -------------------------------------------------------------------------------------------------
def yaw_matrix(yaw):
    """rot[12] as rt_render takes it (rows of four, world = R * local) for a turn about the y axis."""
    c, s = F32(np.cos(yaw)), F32(np.sin(yaw))
    return np.array([c, 0, s, 0, 0, 1, 0, 0, -s, 0, c, 0], F32)


def view_guides(h, w, rot, cam, focal_px):
    """What a pinhole camera sees of three planes, intersected in FP32: a floor y = 0.4, a back wall z = 1.5, and the front
    z = 0.5 of a box (x in [-0.5, 0.2], y in [-0.3, 0.4]) that occludes part of the wall -> position4, normal4 [h, w, 4],
    prim int32 [h, w] (0 floor, 1 wall, 2 box).  The primary ray of pixel (x, y) is R * (x - w/2, y - h/2, focal)."""
    rot, cam, f = np.asarray(rot, F32), np.asarray(cam, F32), F32(focal_px)
    lx = (np.arange(w, dtype=F32) - F32(0.5) * F32(w))[None, :] + np.zeros((h, 1), F32)
    ly = (np.arange(h, dtype=F32) - F32(0.5) * F32(h))[:, None] + np.zeros((1, w), F32)
    with np.errstate(all="ignore"):
        d = [(rot[4 * k] * lx + rot[4 * k + 1] * ly) + rot[4 * k + 2] * f for k in range(3)]
        t_floor = (F32(0.4) - cam[1]) / d[1]
        t_wall = (F32(1.5) - cam[2]) / d[2]
        t_box = (F32(0.5) - cam[2]) / d[2]
        bx, by = cam[0] + t_box * d[0], cam[1] + t_box * d[1]
        on_box = (t_box > 0) & (bx >= F32(-0.5)) & (bx <= F32(0.2)) & (by >= F32(-0.3)) & (by <= F32(0.4))
        t = np.where(t_wall > 0, t_wall, F32(np.inf)).astype(F32)
        prim = np.where(t_wall > 0, 1, -1).astype(np.int32)
        nearer = on_box & (t_box < t)
        t, prim = np.where(nearer, t_box, t), np.where(nearer, 2, prim).astype(np.int32)
        nearer = (t_floor > 0) & (t_floor < t)
        t, prim = np.where(nearer, t_floor, t).astype(F32), np.where(nearer, 0, prim).astype(np.int32)
        hit = prim >= 0
        pos = np.zeros((h, w, 4), F32)
        for k in range(3):
            pos[..., k] = np.where(hit, cam[k] + t * d[k], F32(0))
        pos[..., 3] = np.where(hit, t, F32(0))
    nrm = np.zeros((h, w, 4), F32)
    nrm[..., 1] = np.where(prim == 0, F32(-1), F32(0))
    nrm[..., 2] = np.where(prim >= 1, F32(-1), F32(0))
    return pos, nrm, prim


def noisy_values(rng, h, w):
    """Uniform values with 1 % NaN of two payloads (a quiet one with a payload, a signalling one) and a few +-INF."""
    v = rng.random((h, w), dtype=F32)
    bits = v.view(np.uint32)
    u = rng.random((h, w))
    bits[u < 0.005] = 0x7FC12345
    bits[(u >= 0.005) & (u < 0.01)] = 0xFFA00001
    v[(u >= 0.01) & (u < 0.013)] = np.inf
    v[(u >= 0.013) & (u < 0.016)] = -np.inf
    return v


def spoil(rng, pos):
    """About 3 % of the pixels invalid: w = 0, negative, NaN."""
    u = rng.random(pos.shape[:2])
    pos[..., 3][u < 0.01] = 0
    pos[..., 3][(u >= 0.01) & (u < 0.02)] = -1
    pos[..., 3][(u >= 0.02) & (u < 0.03)] = np.nan
    return pos


PREV_VIEW = (0.0, (0.0, 0.0, -2.0))          # yaw, camera
CUR_VIEW = (0.05, (0.03, 0.01, -1.97))
# the tall plane is three pixels wide: its focal length is its height and its camera does not turn, or nothing would reproject
TALL_VIEW = (0.0, (0.0, 0.01, -1.97))


@functools.lru_cache(maxsize=None)
def view_pair(h, w, focal=None, cur=CUR_VIEW):
    """The planes of one call on a h x w plane, focal = width unless given: (value, position4, normal4, prim, prev, prev_rot, prev_cam,
    prev_focal_px).  The history is what a first frame of the previous view leaves, with history lengths 1 .. 6 and a few
    records of a foreign primitive.  The arrays are shared: do not write to them."""
    rng = np.random.default_rng(1000 * h + w)
    prev_rot, prev_cam = yaw_matrix(PREV_VIEW[0]), np.array(PREV_VIEW[1], F32)
    focal = F32(w if focal is None else focal)
    pos0, nrm0, prim0 = view_guides(h, w, prev_rot, prev_cam, focal)
    spoil(rng, pos0)
    prev, _, _, _, _ = accumulate(noisy_values(rng, h, w), pos0, nrm0, prim0, None, prev_rot, prev_cam, focal)
    lengths = rng.integers(1, 7, (h, w)).astype(F32)
    prev[..., COUNT] = np.where(prev[..., COUNT] > 0, lengths, F32(0))
    foreign = rng.random((h, w)) < 0.01
    prev[..., PRIM].view(np.int32)[foreign] = 7
    pos, nrm, prim = view_guides(h, w, yaw_matrix(cur[0]), np.array(cur[1], F32), focal)
    spoil(rng, pos)
    out = (noisy_values(rng, h, w), pos, nrm, prim, prev, prev_rot, prev_cam, focal)
    for a in out[:5]:
        a.setflags(write=False)
    return out


def call_args(h, w, param_set, focal=None, cur=CUR_VIEW):
    """(value, position4, normal4, prim or None, prev or None), and the keywords of accumulate() / runtime.accumulate_params
    apart from the view's focal, for a parameter set."""
    over, with_prim, with_prev = PARAM_SETS[param_set]
    value, pos, nrm, prim, prev, prev_rot, prev_cam, focal = view_pair(h, w, focal, cur)
    kw = dict(DEFAULTS)
    kw.update(over)
    kw.update(prev_rot=prev_rot, prev_cam=prev_cam)
    return (value, pos, nrm, prim if with_prim else None, prev if with_prev else None), kw


@functools.lru_cache(maxsize=None)
def reference(h, w, param_set, focal=None, cur=CUR_VIEW):
    """The restatement's (next bits, mean bits, variance bits, stats) of call_args(h, w, param_set); shared, do not write."""
    planes, kw = call_args(h, w, param_set, focal, cur)
    nxt, mean, var, stats, _ = accumulate(*planes, prev_focal_px=F32(w if focal is None else focal), **kw)
    return nxt.view(np.uint32), mean.view(np.uint32), var.view(np.uint32), stats


def check_generator():
    """The comparison is sharp: on the 70 x 200 pair most valid pixels find history, a good share does not, most of those
    that do blend all four taps, and the order of the taps shows in the bits."""
    h, w = 70, 200
    planes, kw = call_args(h, w, "defaults")
    nxt, mean, _, stats, taps = accumulate(*planes, prev_focal_px=F32(w), **kw)
    valid = stats["valid_pixels"]
    assert stats["found_history"] > 0.80 * valid
    assert valid - stats["found_history"] > 0.03 * valid
    assert (taps == 4).sum() > 0.5 * stats["found_history"]
    _, back, _, _, _ = accumulate(*planes, prev_focal_px=F32(w), reverse=True, **kw)
    assert (back.view(np.uint32) != mean.view(np.uint32)).sum() > 0.10 * h * w
    return stats


def exact_region(region_prev, value_is, tap_list):
    """The pixels whose mean is exactly a constant c (1.0f or 0.0f) after a call: their value is c and every tap they accepted
    had a mean of exactly c (region_prev, None before the first frame); then num == c * den and the blend returns c."""
    region = value_is.copy()
    if region_prev is not None:
        for qy, qx, acc, _ in tap_list:
            region &= ~acc | region_prev[qy, qx]
    return region
