"""Helpers of the AOV tests: the frame's primary rays restated in numpy FP32 (draw_pixel, oracle/rt_oracle.c:241-255) and the
expected planes derived from a closest-hit answer.  tests/test_aov_abi.py checks the restatement against the oracle itself."""
import numpy as np

F = np.float32


def owned_rows(cfg):
    br = cfg.band_rows if cfg.band_rows > 0 else cfg.height
    bc = max(cfg.band_count, 1)
    return np.array([y for y in range(cfg.height) if (y // br) % bc == cfg.band_index], np.int64)


def primary_directions(cfg, rot, focal):
    """float32 [rows, W, aa, 3]: the normalised direction of AA sample dy*aa_x+dx of every owned pixel (global coordinates)."""
    rot = np.asarray(rot, F)
    rx, ry = cfg.aa_x, cfg.aa_y
    sy = F(rx) / F(ry)
    ys, xs = owned_rows(cfg), np.arange(cfg.width)
    bx = (xs * rx).astype(F) - (F(cfg.width) * F(rx)) / F(2.0)
    by = (ys * ry).astype(F) - (F(cfg.height) * F(ry)) / F(2.0)
    a = np.arange(rx * ry)
    dxs, dys = (a % rx).astype(F), (a // rx).astype(F)
    X = np.broadcast_to((bx[None, :, None] + dxs[None, None, :]).astype(F), (len(ys), len(xs), len(a)))
    Y = np.broadcast_to(((by[:, None, None] + dys[None, None, :]).astype(F) * sy).astype(F), X.shape)
    Z = F(focal) + F(0.0)
    v = [((rot[4 * k] * X).astype(F) + (rot[4 * k + 1] * Y).astype(F)).astype(F) + rot[4 * k + 2] * Z for k in range(3)]  # left to right
    dot = ((v[0] * v[0] + v[1] * v[1]).astype(F) + v[2] * v[2]).astype(F)
    nrm = np.sqrt(dot).astype(F)
    out = np.stack([(c / nrm).astype(F) for c in v], -1)
    assert out.dtype == F
    return np.ascontiguousarray(out)


def rays_of(cam, dirs):
    """[k, 6] = (cam, direction) for directions [..., 3]"""
    d = dirs.reshape(-1, 3)
    s = np.broadcast_to(np.asarray(cam, F)[:3], d.shape)
    return np.ascontiguousarray(np.concatenate([s, d], 1), F)


def expected_planes(cam, dirs, tri, out10):
    """The six planes from a closest-hit answer (tri [k], out10 [k, 10]) for rays (cam, dirs), shaped like dirs[..., 0]."""
    shape = dirs.shape[:-1]
    tri = tri.reshape(shape)
    out10 = out10.reshape(shape + (10,)).astype(F)
    hit = tri != -1
    z4 = np.zeros(shape + (4,), F)
    pos, nrm, alb, dr = z4.copy(), z4.copy(), z4.copy(), z4.copy()
    pos[..., :3] = out10[..., 0:3]; pos[..., 3] = 1.0
    nrm[..., :3] = out10[..., 3:6]
    alb[...] = out10[..., 6:10]
    pos[~hit] = 0; nrm[~hit] = 0; alb[~hit] = 0
    dr[..., :3] = dirs
    d = (out10[..., 0:3] - np.asarray(cam, F)[:3]).astype(F)
    depth = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F) + d[..., 2] * d[..., 2]).astype(F)).astype(F)
    depth = np.where(hit, depth, F(np.inf)).astype(F)
    return {"prim": tri.astype(np.int32), "depth": depth, "position": pos, "normal": nrm, "albedo": alb, "direction": dr}


def u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def assert_planes_equal(got, want, names=None):
    for name in (names or want):
        assert got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        bad = np.argwhere(u32(got[name]) != u32(want[name]))
        assert bad.size == 0, "plane %s: %d elements differ, first at %s" % (name, len(bad), bad[0])
