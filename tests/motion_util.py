"""The motion planes of include/uob_rt.h ("rt_motion_planes") and the accumulate call that takes them
("rt_accumulate_plane_moving") restated in numpy, one FP32 operation per line of the definitions, vectorised over the elements
(the four taps of the accumulate stay a sequential loop: their order is part of the contract); and a generator of inputs that
reaches every case of the motion function.  CPU only; shared by the CPU and the GPU tests."""
import functools

import numpy as np

F32 = np.float32
QUIET_NAN = np.uint32(0x7FC00000)
WORDS, MEAN, M2, COUNT, PRIM = 12, 3, 7, 8, 9          # rt_history_texel as float32 words (accumulate_util has the same)
COUNTS = (1, 63, 64, 65, 257, 3700)                   # one element, around a wave, beyond a workgroup, the 37 x 100 plane
STATS_KEYS = ("elements", "valid_elements", "moved", "unmoved", "copied", "prim_out_of_range")


def _quiet(a):
    """NaNs as the quiet NaN 0x7FC00000, everything else its own bits."""
    bits = a.view(np.uint32).copy()
    bits[a != a] = QUIET_NAN
    return bits.view(F32)


def _dot(a, b):
    x = a[0] * b[0]
    y = a[1] * b[1]
    z = a[2] * b[2]
    return (x + y) + z


def motion(vertices_now, vertices_then, normals_then, prim, position4, normal4):
    """-> (prev_position4, prev_normal4 shaped like position4, stats dict as rt_debug_motion_stats counts them)."""
    vn = np.ascontiguousarray(vertices_now, F32).reshape(-1, 3, 4)
    vt = np.ascontiguousarray(vertices_then, F32).reshape(-1, 3, 4)
    nt = np.ascontiguousarray(normals_then, F32).reshape(-1, 4)
    n = nt.shape[0]
    assert vn.shape[0] == n and vt.shape[0] == n
    shape = np.shape(prim)
    prim = np.ascontiguousarray(prim, np.int32).reshape(-1)
    pos = np.ascontiguousarray(position4, F32).reshape(-1, 4)
    nrm = np.ascontiguousarray(normal4, F32).reshape(-1, 4)
    w_ok = pos[:, 3] > F32(0)
    in_range = (prim >= -2) & (prim < n)
    valid = w_ok & in_range
    copied = valid & (prim < 0)
    tri = valid & (prim >= 0)
    t = np.where(tri, prim, 0)
    if n == 0:
        vn, vt, nt = np.zeros((1, 3, 4), F32), np.zeros((1, 3, 4), F32), np.zeros((1, 4), F32)
    a, b, c = (vn[t, k, :3].T for k in range(3))          # [3, count] each
    a0, b0, c0 = (vt[t, k, :3].T for k in range(3))
    same = np.ones(prim.shape, bool)
    for now, then in ((a, a0), (b, b0), (c, c0)):
        for j in range(3):
            same &= now[j] == then[j]
    unmoved, moved = tri & same, tri & ~same
    with np.errstate(all="ignore"):
        e1 = [b[j] - a[j] for j in range(3)]
        e2 = [c[j] - a[j] for j in range(3)]
        d = [pos[:, j] - a[j] for j in range(3)]
        f1 = [b0[j] - a0[j] for j in range(3)]
        f2 = [c0[j] - a0[j] for j in range(3)]
        d11, d12, d22, p1, p2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(d, e1), _dot(d, e2)
        x = d11 * d22
        y = d12 * d12
        den = x - y
        x = d22 * p1
        y = d12 * p2
        u = (x - y) / den
        x = d11 * p2
        y = d12 * p1
        v = (x - y) / den
        carried = []
        for j in range(3):
            x = u * f1[j]
            x = a0[j] + x
            y = v * f2[j]
            carried.append(_quiet(x + y))
    out_p = np.zeros(pos.shape, np.uint32)
    out_n = np.zeros(pos.shape, np.uint32)
    keep = copied | unmoved
    out_p[keep] = pos.view(np.uint32)[keep]
    out_n[keep] = nrm.view(np.uint32)[keep]
    for j in range(3):
        out_p[moved, j] = carried[j].view(np.uint32)[moved]
    out_p[moved, 3] = F32(1).view(np.uint32)
    out_n[moved, :3] = nt.view(np.uint32)[t[moved], :3]
    stats = {"elements": int(prim.size), "valid_elements": int(valid.sum()), "moved": int(moved.sum()), "unmoved": int(unmoved.sum()),
             "copied": int(copied.sum()), "prim_out_of_range": int((w_ok & ~in_range).sum())}
    return out_p.view(F32).reshape(shape + (4,)), out_n.view(F32).reshape(shape + (4,)), stats


def accumulate_moving(value, position4, normal4, prim, reproj_position4, reproj_normal4, prev, prev_rot, prev_cam, prev_focal_px,
                      normal_min_dot=0.9, plane_eps=0.01, max_history=32, accepted=None):
    """rt_accumulate_plane_moving -> (next float32 [h, w, 12], mean [h, w], variance [h, w], stats dict as
    rt_debug_accumulate_stats counts them, the accepted taps per pixel).  reproj_* None: the guides themselves, which is
    rt_accumulate_plane.  accepted, a list, receives (row, column, accepted mask, weight) of each of the four taps."""
    v = np.ascontiguousarray(value, F32)
    pos = np.ascontiguousarray(position4, F32)
    nrm = np.ascontiguousarray(normal4, F32)
    rpos = pos if reproj_position4 is None else np.ascontiguousarray(reproj_position4, F32)
    rnrm = nrm if reproj_normal4 is None else np.ascontiguousarray(reproj_normal4, F32)
    h, w = v.shape
    rot, cam = np.asarray(prev_rot, F32), np.asarray(prev_cam, F32)
    focal, nmin, eps = F32(prev_focal_px), F32(normal_min_dot), F32(plane_eps)
    valid = pos[..., 3] > F32(0)
    Pr = [rpos[..., k] for k in range(3)]
    Nr = [rnrm[..., k] for k in range(3)]
    with np.errstate(all="ignore"):
        vv = v * v
        num, num2, den = np.zeros((h, w), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
        cmin = np.full((h, w), np.inf, F32)
        taps = np.zeros((h, w), np.int64)
        nocand = np.zeros((h, w), bool)
        if prev is not None:
            d = [Pr[k] - cam[k] for k in range(3)]
            q = []
            for j in range(3):
                x = d[0] * rot[j]
                y = d[1] * rot[4 + j]
                z = d[2] * rot[8 + j]
                q.append((x + y) + z)
            x = q[0] * focal
            y = q[1] * focal
            x = x / q[2]
            y = y / q[2]
            fx = x + F32(0.5) * F32(w)
            fy = y + F32(0.5) * F32(h)
            cand = valid & (rpos[..., 3] > F32(0)) & (q[2] > F32(0)) & (fx >= F32(-1)) & (fx < F32(w)) & (fy >= F32(-1)) & (fy < F32(h))
            nocand = valid & ~cand
            xf, yf = np.floor(fx), np.floor(fy)
            ax, ay = fx - xf, fy - yf
            x0 = np.where(cand, xf, F32(0)).astype(np.int64)
            y0 = np.where(cand, yf, F32(0)).astype(np.int64)
            bx, by = F32(1) - ax, F32(1) - ay
            for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)):          # j outer, i inner, both ascending
                qx, qy = x0 + i, y0 + j
                wt = (ax if i else bx) * (ay if j else by)
                acc = cand & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (wt > F32(0))
                cy, cx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                r = prev[cy, cx]
                acc &= r[..., COUNT] > F32(0)
                if prim is not None:
                    acc &= r[..., PRIM].view(np.int32) == prim
                x = Nr[0] * r[..., 4]
                y = Nr[1] * r[..., 5]
                z = Nr[2] * r[..., 6]
                acc &= (x + y) + z >= nmin
                e = [r[..., k] - Pr[k] for k in range(3)]
                x = Nr[0] * e[0]
                y = Nr[1] * e[1]
                z = Nr[2] * e[2]
                acc &= np.abs((x + y) + z) <= eps
                x = wt * r[..., MEAN]
                num = np.where(acc, num + x, num)
                x = wt * r[..., M2]
                num2 = np.where(acc, num2 + x, num2)
                den = np.where(acc, den + wt, den)
                cmin = np.where(acc & (r[..., COUNT] < cmin), r[..., COUNT], cmin)
                taps += acc
                if accepted is not None:
                    accepted.append((cy, cx, acc, wt))
        found = taps > 0
        mp = num / den
        sp = num2 / den
        nmax = F32(max_history - 1)
        n = np.where(cmin < nmax, cmin, nmax) + F32(1)
        s = F32(1) / n
        x = v - mp
        x = s * x
        mean5 = _quiet(mp + x)
        x = vv - sp
        x = s * x
        m25 = _quiet(sp + x)
        mean = np.where(found, mean5.view(np.uint32), v.view(np.uint32)).view(F32)
        m2 = np.where(found, m25.view(np.uint32), _quiet(vv).view(np.uint32)).view(F32)
        count = np.where(found, n, np.where(valid, F32(1), F32(0))).astype(F32)
        x = mean * mean
        x = m2 - x
        var = np.where(x > F32(0), x, F32(0)).astype(F32)
    nxt = np.zeros((h, w, WORDS), F32)
    nxt[..., 0:3] = pos[..., 0:3]                          # step 7 stores the CURRENT guides
    nxt[..., 4:7] = nrm[..., 0:3]
    out = nxt.view(np.uint32)
    out[..., MEAN] = mean.view(np.uint32)
    out[..., M2] = m2.view(np.uint32)
    out[..., COUNT] = count.view(np.uint32)
    out[..., PRIM] = (prim if prim is not None else np.full((h, w), -1, np.int32)).view(np.uint32)
    stats = {"pixels": h * w, "valid_pixels": int(valid.sum()), "found_history": int(found.sum()), "accepted_taps": int(taps.sum()),
             "no_candidate": int(nocand.sum())}
    return nxt, mean, var, stats, taps


# ---- inputs of the motion function ------------------------------------------------------------------------------------------
def _rotation(rng):
    """A random rotation matrix (float64) from a random axis and angle."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-1.0, 1.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


@functools.lru_cache(maxsize=None)
def scenes(n=40, seed=5):
    """(vertices_now [3n, 4], vertices_then [3n, 4], normals_then [n, 4]): n random triangles then, and now a copy in which
    every third triangle is left unmoved and the others are moved rigidly in groups of four; triangle 1 is degenerate now
    (den == 0: two equal corners) and moved.  Shared: do not write."""
    rng = np.random.default_rng(seed)
    then = rng.uniform(-1.0, 1.0, size=(n, 3, 3))
    now = then.copy()
    for g in range(0, n, 4):
        R, off = _rotation(rng), rng.uniform(-0.3, 0.3, size=3)
        for t in range(g, min(g + 4, n)):
            if t % 3 != 0:
                now[t] = then[t] @ R.T + off
    vn, vt = np.zeros((n, 3, 4), F32), np.zeros((n, 3, 4), F32)
    vn[..., :3], vt[..., :3] = now, then
    vn[..., 3] = vt[..., 3] = 1
    vn[1, 2] = vn[1, 1]                                    # the degenerate one
    nt = np.zeros((n, 4), F32)
    nt[:, :3] = rng.normal(size=(n, 3))
    out = (np.ascontiguousarray(vn.reshape(3 * n, 4)), np.ascontiguousarray(vt.reshape(3 * n, 4)), nt)
    for a in out:
        a.setflags(write=False)
    return out


def elements_on(vertices_now, count, seed, spoil=True):
    """`count` elements at random barycentrics on the live triangles -> (prim int32 [count], position4, normal4 [count, 4]); with
    spoil, about a quarter of them are then spoiled: NaN positions and w, w = 0, w < 0, and prim of -1, -2, -3 and n."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices_now, F32).reshape(-1, 3, 4)
    n = v.shape[0]
    prim = rng.integers(0, n, count).astype(np.int32)
    bary = rng.dirichlet((1.0, 1.0, 1.0), count).astype(F32)
    pos = np.zeros((count, 4), F32)
    pos[:, :3] = (bary[:, 0, None] * v[prim, 0, :3] + bary[:, 1, None] * v[prim, 1, :3]) + bary[:, 2, None] * v[prim, 2, :3]
    pos[:, 3] = rng.uniform(0.5, 4.0, count)
    nrm = np.zeros((count, 4), F32)
    nrm[:, :3] = rng.normal(size=(count, 3))
    nrm[:, 3] = rng.uniform(-1, 1, count)                  # (w of the normal plane is carried through the copies)
    if spoil:
        u = rng.random(count)
        pos[u < 0.03, 0] = np.nan
        pos[(u >= 0.03) & (u < 0.06), 3] = np.nan
        pos[(u >= 0.06) & (u < 0.09), 3] = 0
        pos[(u >= 0.09) & (u < 0.11), 3] = -1
        for lo, code in ((0.11, -1), (0.15, -2), (0.19, -3), (0.22, n)):
            prim[(u >= lo) & (u < lo + 0.03)] = code
    return prim, pos, nrm


@functools.lru_cache(maxsize=None)
def case(count):
    """The scenes and `count` spoiled elements, with the restatement's answer -> (scene arrays, (prim, position4, normal4),
    (prev_position4 bits, prev_normal4 bits, stats)).  Shared: do not write."""
    sc = scenes()
    el = elements_on(sc[0], count, 900 + count)
    p, nr, stats = motion(*sc, *el)
    return sc, el, (p.view(np.uint32), nr.view(np.uint32), stats)


def check_generator():
    """The comparison is sharp: at 3 700 elements every case of the function is met, the degenerate triangle included, and the
    carried points differ from the inputs."""
    sc, (prim, pos, nrm), (p, nr, stats) = case(3700)
    assert stats["moved"] > 1500 and stats["unmoved"] > 500 and stats["copied"] > 100 and stats["prim_out_of_range"] > 50
    assert stats["valid_elements"] == stats["moved"] + stats["unmoved"] + stats["copied"] < stats["elements"]
    degenerate = (prim == 1) & (pos[:, 3] > 0)
    assert degenerate.any() and not np.isfinite(p.view(F32)[degenerate, :3]).all()
    moved = (p[:, 3] == F32(1).view(np.uint32)) & (nr[:, 3] == 0) & np.isfinite(p.view(F32)[:, :3]).all(1)
    assert (np.abs(p.view(F32)[moved, :3] - pos[moved, :3]).max(1) > 1e-3).sum() > 1000
    return stats


def moving_planes(h, w):
    """Reprojection planes for accumulate_util.view_pair(h, w): the guides themselves with, column by column, the position
    shifted a little along x (another tap, still on the planes z = const / off the floor's plane y = const by nothing), w = 0
    (no candidate) and a turned normal -> (reproj_position4, reproj_normal4)."""
    import accumulate_util as au
    _, pos, nrm, _, _, _, _, _ = au.view_pair(h, w)
    rng = np.random.default_rng(31 * h + w)
    rpos, rnrm = pos.copy(), nrm.copy()
    u = rng.random((h, w))
    rpos[..., 0] = np.where(u < 0.5, pos[..., 0] + F32(0.02), pos[..., 0])
    rpos[..., 3] = np.where((u >= 0.5) & (u < 0.6), F32(0), np.where((u >= 0.6) & (u < 0.63), F32(np.nan), F32(1)))
    turned = (u >= 0.7) & (u < 0.8)
    rnrm[..., 0] = np.where(turned, F32(0.6), nrm[..., 0])
    for k in (1, 2):
        rnrm[..., k] = np.where(turned, nrm[..., k] * F32(0.8), nrm[..., k])
    rnrm[..., 3] = 0
    return rpos, rnrm
