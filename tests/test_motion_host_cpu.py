"""CPU: rt_motion_planes_host and rt_accumulate_plane_moving_host against the numpy restatement in tests/motion_util.py, on
every output word; an unmoved scene returns its inputs; the moving accumulate with the guides as reprojection planes, and
with none, is rt_accumulate_plane_host; and a pixel without a previous place starts over."""
import numpy as np
import pytest

import accumulate_util as au
import motion_util as mu
from uob_raytracer_amd import abi, runtime as rt

F32 = np.float32


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_generator_reaches_every_case():
    print(mu.check_generator())


@pytest.mark.parametrize("count", mu.COUNTS)
def test_motion_host_equals_the_restatement(count):
    sc, el, (want_p, want_n, _) = mu.case(count)
    got_p, got_n = rt.motion_planes_host(*sc, *el)
    assert np.array_equal(_u32(got_p), want_p) and np.array_equal(_u32(got_n), want_n)


def test_motion_host_takes_planes_of_any_leading_shape():
    sc, (prim, pos, nrm), (want_p, want_n, _) = mu.case(3700)
    got_p, got_n = rt.motion_planes_host(*sc, prim.reshape(37, 100), pos.reshape(37, 100, 4), nrm.reshape(37, 100, 4))
    assert got_p.shape == (37, 100, 4)
    assert np.array_equal(_u32(got_p).reshape(-1, 4), want_p) and np.array_equal(_u32(got_n).reshape(-1, 4), want_n)


def test_an_unmoved_scene_returns_the_input_planes_bits():
    vn, _, nt = mu.scenes()
    prim, pos, nrm = mu.elements_on(vn, 3700, 12, spoil=False)
    prim[::7] = -1
    prim[1::7] = -2
    pos.view(np.uint32)[5::11, 0] = 0x7FC12345               # a NaN coordinate with a payload: copied, not computed
    got_p, got_n = rt.motion_planes_host(vn, vn, nt, prim, pos, nrm)
    assert np.array_equal(_u32(got_p), _u32(pos)) and np.array_equal(_u32(got_n), _u32(nrm))
    want_p, want_n, stats = mu.motion(vn, vn, nt, prim, pos, nrm)
    assert np.array_equal(_u32(want_p), _u32(pos)) and stats["moved"] == 0 and stats["valid_elements"] == 3700


def test_the_carried_point_lies_on_the_previous_triangle():
    """The restated accuracy for well-shaped triangles: rigidly moved triangles carry a point to the same barycentrics."""
    rng = np.random.default_rng(3)
    n = 500
    then = rng.uniform(-1, 1, size=(n, 3, 3))
    e1, e2 = then[:, 1] - then[:, 0], then[:, 2] - then[:, 0]
    cos = np.abs((e1 * e2).sum(1)) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    keep = (cos < 0.8) & (np.linalg.norm(e1, axis=1) > 0.3) & (np.linalg.norm(e2, axis=1) > 0.3)
    then = then[keep]
    n = then.shape[0]
    now = np.stack([t @ mu._rotation(rng).T + rng.uniform(-0.3, 0.3, 3) for t in then])
    bary = rng.dirichlet((1, 1, 1), n)
    vn, vt = np.ones((n, 3, 4), F32), np.ones((n, 3, 4), F32)
    vn[..., :3], vt[..., :3] = now, then
    pos = np.ones((n, 4), F32)
    pos[:, :3] = np.einsum("nk,nkc->nc", bary, vn[..., :3].astype(np.float64))
    got_p, _ = rt.motion_planes_host(vn.reshape(-1, 4), vt.reshape(-1, 4), np.zeros((n, 4), F32), np.arange(n, dtype=np.int32), pos,
                                     np.zeros((n, 4), F32))
    want = np.einsum("nk,nkc->nc", bary, vt[..., :3].astype(np.float64))
    err = np.abs(got_p[:, :3] - want).max()
    print("well-shaped triangles: max error of the carried point %.3g" % err)
    assert err < 1e-5 and (got_p[:, 3] == 1).all()


# ---- the moving accumulate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param_set", list(au.PARAM_SETS))
@pytest.mark.parametrize("size", au.SIZES, ids=lambda s: "%dx%d" % s)
def test_moving_accumulate_host_equals_the_restatement(size, param_set):
    h, w = size
    planes, kw = au.call_args(h, w, param_set)
    rpos, rnrm = mu.moving_planes(h, w)
    want_next, want_mean, want_var, stats, _ = mu.accumulate_moving(*planes[:4], rpos, rnrm, planes[4], prev_focal_px=F32(w), **kw)
    nxt, mean, var = rt.accumulate_plane_host(*planes, reproj_position4=rpos, reproj_normal4=rnrm, prev_focal=w, **kw)
    assert np.array_equal(_u32(nxt), _u32(want_next))
    assert np.array_equal(_u32(mean), _u32(want_mean)) and np.array_equal(_u32(var), _u32(want_var))
    if size == (70, 200) and param_set == "defaults":       # the planes matter: other bits than the static call's, and history found
        assert not np.array_equal(_u32(want_next), au.reference(h, w, param_set)[0])
        assert stats["found_history"] > 0.3 * stats["valid_pixels"] and stats["no_candidate"] > 0.1 * stats["valid_pixels"]


@pytest.mark.parametrize("param_set", ["defaults", "no_prim", "no_prev", "plane_eps_0"])
@pytest.mark.parametrize("size", [(37, 100), (70, 200)], ids=lambda s: "%dx%d" % s)
def test_guides_as_reprojection_planes_and_no_planes_are_the_static_call(size, param_set):
    h, w = size
    planes, kw = au.call_args(h, w, param_set)
    want = au.reference(h, w, param_set)
    static = rt.accumulate_plane_host(*planes, prev_focal=w, **kw)
    same = rt.accumulate_plane_host(*planes, reproj_position4=planes[1], reproj_normal4=planes[2], prev_focal=w, **kw)
    # NULL planes through the moving entry itself
    p = rt.accumulate_params(w, h, prev_focal=w, **kw)
    v, pos, nrm, prim, prev = (None if a is None else np.ascontiguousarray(a) for a in planes)
    nxt, mean, var = np.empty((h, w, 12), F32), np.empty((h, w), F32), np.empty((h, w), F32)
    import ctypes as C
    rc = rt.lib().rt_accumulate_plane_moving_host(C.byref(p), rt._fp(v), rt._fp(pos), rt._fp(nrm), rt._ip(prim), None, None,
                                                  rt._fp(prev) if prev is not None else None, rt._fp(nxt), rt._fp(mean), rt._fp(var))
    assert rc == abi.RT_OK
    for got in (static, same, (nxt, mean, var)):
        for g, ref in zip(got, want[:3]):
            assert np.array_equal(_u32(g), ref)
    # and the restatement of the moving call agrees with accumulate_util's in the no-motion case
    mine = mu.accumulate_moving(*planes[:4], None, None, planes[4], prev_focal_px=F32(w), **kw)
    assert np.array_equal(_u32(mine[0]), want[0]) and mine[3] == want[3]


def test_a_pixel_without_a_previous_place_starts_over():
    h, w = 37, 100
    planes, kw = au.call_args(h, w, "defaults")
    value, pos, nrm, prim, prev = planes
    rpos, rnrm = pos.copy(), nrm.copy()
    rpos[::2, :, 3] = 0                                      # every other row: no place in the previous scene
    nxt, mean, _ = rt.accumulate_plane_host(*planes, reproj_position4=rpos, reproj_normal4=rnrm, prev_focal=w, **kw)
    valid = pos[..., 3] > 0
    count = nxt[..., abi.HISTORY_COUNT]
    assert (count[::2][valid[::2]] == 1).all() and (count[~valid] == 0).all()
    assert np.array_equal(_u32(mean[::2]), _u32(value[::2]))
    static = au.reference(h, w, "defaults")[0]
    assert np.array_equal(_u32(nxt[1::2]), static[1::2]) and (count[1::2] > 1).sum() > 1000
