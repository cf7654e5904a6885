"""-m gpu: the device scene-edit kernels above their internal size thresholds — the radix
sort and scan of the device tile build beyond one scan step, rt_scene_check beyond its capped grid, rt_pose_triangles beyond
its capped grid and at the object limit.  Every case compares the edited context with a plain restatement (numpy, or
Scene.posed on the host) and with a fresh context of the same scene, bit for bit (the boxes' min / max up to the sign of a
zero).  Frames are 64 x 48, one sample per pixel, one shadow sample: the kernels under test do not depend on the frame."""
import numpy as np
import pytest

import scene_sizes_util as U
import test_gpu_scene_replace as sr
import test_gpu_scene_update as su
from conftest import focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

VIEW = su.VIEWS[0]
DEVICE_TILES = abi.RT_UPDATE_DEVICE_TILES


def _cfg():
    return abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=1)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frame(tr, cfg):
    argb, rgb = su._frame(tr, cfg, VIEW)
    return argb.copy(), rgb.copy()


def _to_device(packed):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in packed]
    torch.cuda.synchronize()
    return out


def _replace_device(tr, dev):
    import torch
    tr.replace_scene_device(*dev, stream=torch.cuda.Stream())
    torch.cuda.synchronize()


def _update_device(tr, dev, device_tiles=False):
    import torch
    tr.update_scene_device(*(t.data_ptr() for t in dev), dev[1].shape[0], stream=torch.cuda.Stream().cuda_stream,
                           device_tiles=device_tiles)
    torch.cuda.synchronize()


class Fresh:
    """What fresh contexts make of a scene: the default context's frame; the Morton context's order, tiles and frame."""

    def __init__(self, cfg, sc):
        tr = rt.RayTracer(cfg, sc)
        self.frame = _frame(tr, cfg)
        tr.close()
        tr = sr._fresh_morton(cfg, sc)
        self.orig, self.tiles = tr.tile_data()
        self.morton_frame = _frame(tr, cfg)
        tr.close()


def _assert_scene(d, packed):
    """scene_data()'s scene in original order is the packed scene, bit for bit."""
    for name, want in zip(("vertices", "normals", "colors"), packed):
        assert np.array_equal(_u32(d[name]), _u32(want)), name


def _assert_tiled_copy(d, orig):
    """The tiled copy is the gather of the original order: entry j is triangle orig[j], for every j."""
    n = len(orig)
    assert np.array_equal(_u32(d["vertices_m"]).reshape(n, 12), _u32(d["vertices"]).reshape(n, 12)[orig])
    assert np.array_equal(_u32(d["normals_m"]), _u32(d["normals"])[orig])
    assert np.array_equal(_u32(d["colors_m"]), _u32(d["colors"])[orig])


def _assert_sampled_tiles(tiles, v4, orig):
    """The tiles' data against the float64 numpy restatement, on a seeded sample of tiles (first, last and first all-small
    tile included)."""
    pick = U.sample_tiles(U.morton_keys_np(v4)[orig])
    assert sr._same_tiles(tiles[pick], U.tile_rows_np(su.tile_data_np, v4, orig, pick))


def _assert_device_build(tr, cfg, packed, fresh):
    """The context's tiles were built on the device for the scene `packed`: everything the issue lists for a size."""
    v4 = packed[0]
    n = packed[1].shape[0]
    orig, tiles = tr.tile_data()
    assert np.array_equal(np.sort(orig), np.arange(n))                       # a permutation
    assert np.array_equal(orig, U.morton_order_np(v4))                       # the restated Morton order
    assert np.array_equal(orig, fresh.orig)                                  # the host's
    assert tiles.shape == ((n + 63) // 64, 12) and sr._same_tiles(tiles, fresh.tiles)
    _assert_sampled_tiles(tiles, v4, orig)
    d = tr.scene_data(tiled=True)
    _assert_scene(d, packed)
    _assert_tiled_copy(d, orig)
    got = _frame(tr, cfg)
    assert sr._same_frame(got, fresh.morton_frame) and sr._same_frame(got, fresh.frame)
    return orig


# ---- the readback itself ------------------------------------------------------------------------------------------------
def test_scene_data_contract(scene):
    cfg = _cfg()
    tr = rt.RayTracer(cfg, scene)                                            # 26 triangles: no tiled copy, no box kept
    d = tr.scene_data()
    _assert_scene(d, scene.packed())
    assert d["n_shadow"] == 26 and not d["vbox_lo"].any() and not d["vbox_hi"].any()
    with pytest.raises(rt.RtError) as e:
        tr.scene_data(tiled=True)
    assert e.value.code == abi.RT_E_UNSUPPORTED and "no tiled copy" in str(e.value)
    f, nothing = rt.lib().rt_debug_scene_data, [None] * 9
    assert f(tr._h, *nothing, 0) == 26 and f(tr._h, *nothing, 26) == 26     # a count query; nothing asked for
    assert f(tr._h, *nothing, 25) == abi.RT_E_INVALID
    assert "room for 25 triangles, 26 needed" in rt.lib().rt_last_error().decode()
    sc = U.random_scene(scene, 1100, seed=2)                                 # tile masks: the box is kept
    tr.replace_scene(sc)
    d = tr.scene_data(tiled=True)
    _assert_scene(d, sc.packed())
    _assert_tiled_copy(d, tr.tile_data()[0])
    xyz = sc.packed()[0][:, :3]
    assert np.array_equal(d["vbox_lo"], xyz.min(axis=0)) and np.array_equal(d["vbox_hi"], xyz.max(axis=0))
    assert d["n_shadow"] == 1100
    tr.close()


# ---- a. radix sort and scan ---------------------------------------------------------------------------------------------
SORT_SIZES = {1024: (1, 1), 1025: (2, 1), 16384: (16, 1), 16385: (17, 2), 32769: (33, 3), 40000: (40, 3)}   # n: (chunks, scan steps)


@pytest.mark.parametrize("n", sorted(SORT_SIZES))
def test_sort_and_scan_sizes(n, scene):
    chunks, steps = SORT_SIZES[n]
    assert U.sort_chunks(n) == chunks and U.scan_steps(n) == steps
    if steps > 1:
        assert 256 * -(-n // 1024) > 4096                                    # the scan's loop takes another step
    if n == 32769:
        assert n - (chunks - 1) * U.SORT_CHUNK == 1                          # a last chunk of one element
    cfg = _cfg()
    sc = U.random_scene(scene, n, seed=n)
    tr = rt.RayTracer(cfg, scene)
    _replace_device(tr, _to_device(sc.packed()))
    _assert_device_build(tr, cfg, sc.packed(), Fresh(cfg, sc))
    if n == 16385:                                                           # and through rt_update_scene, for one size
        other = U.random_scene(scene, n, seed=n + 1)
        before = tr.tile_data()[0]
        tr.update_scene(other, device_tiles=True)
        after = _assert_device_build(tr, cfg, other.packed(), Fresh(cfg, other))
        assert not np.array_equal(before, after)
    tr.close()


KEY_M = 16385


@pytest.mark.parametrize("case", ["equal_keys", "top_byte", "bottom_byte", "hot_digit", "many_large"])
def test_sort_key_distributions(case, scene):
    n = U.N_BOX + KEY_M
    assert U.scan_steps(n) == 2 and U.sort_chunks(n) == 17 and 256 * -(-n // 1024) > 4096
    cfg = _cfg()
    sc = U.key_case(scene, case, KEY_M)
    packed = sc.packed()
    tr = rt.RayTracer(cfg, scene)
    _replace_device(tr, _to_device(packed))
    orig = _assert_device_build(tr, cfg, packed, Fresh(cfg, sc))
    keys = U.morton_keys_np(packed[0])
    if case == "equal_keys":                                                 # the index order, across 17 chunks
        assert len(set(keys[U.N_BOX:].tolist())) == 1
        assert np.array_equal(orig[orig >= U.N_BOX], np.arange(U.N_BOX, n))
    if case == "many_large":                                                 # key 0 first, in original order, over 46 tiles
        large = np.nonzero(keys == 0)[0]
        assert set((U.N_BOX + U.large_positions(KEY_M)).tolist()) <= set(large.tolist())
        assert len(large) >= U.N_LARGE > 2 * U.SORT_CHUNK and len(large) // 64 >= 46
        assert np.array_equal(orig[:len(large)], large)
    tr.close()


# ---- b. rt_scene_check beyond its grid cap ----------------------------------------------------------------------------------
CHECK_N = U.CHECK_GRID + U.N_BOX + 70


class BigCheck:
    def __init__(self, box, oracle):
        n = self.n = CHECK_N
        assert n > 1024 * 256 and n % 64 != 0                                # a second trip of the loop; a ragged last tile
        self.cfg = _cfg()
        self.scene = U.check_scene(box, n)
        self.base = U.check_scene(box, n, box_scale=0.9)                     # the same count, another box
        self.packed = self.scene.packed()
        self.dev = _to_device(self.packed)
        self.fresh = Fresh(self.cfg, self.scene)
        self.pix = np.sort(np.random.default_rng(17).choice(64 * 48, 256, replace=False)).astype(np.int32)
        yaw, pitch, cam, light = VIEW
        self.oracle = oracle.render(self.cfg, *self.packed, rt.rotation_matrix(yaw, pitch), cam, light, focal_for(self.cfg),
                                    pix=self.pix)


@pytest.fixture(scope="module")
def big_check(scene, oracle):
    return BigCheck(scene, oracle)


@pytest.mark.parametrize("entry", ["update", "update_device_tiles", "replace"])
def test_check_beyond_the_grid_cap(entry, big_check, scene):
    b = big_check
    cfg, n = b.cfg, b.n
    if entry == "replace":
        tr = rt.RayTracer(cfg, scene)
        _replace_device(tr, b.dev)
    else:
        tr = rt.RayTracer(cfg, b.base)
        kept = tr.tile_data()[0]
        _update_device(tr, b.dev, device_tiles=entry == "update_device_tiles")
    d = tr.scene_data(tiled=True)
    xyz = b.packed[0][:, :3]
    assert np.array_equal(d["vbox_lo"], xyz.min(axis=0)) and np.array_equal(d["vbox_hi"], xyz.max(axis=0))
    assert np.array_equal(d["vbox_lo"], [-1, -1, -1]) and np.array_equal(d["vbox_hi"], [1, 1, 1])
    glass = int((b.packed[2][:, 3] == -1.0).sum())
    assert glass == 4 and d["n_shadow"] == n - glass
    if entry == "update":                                                    # a refit: rt_init's order of the old scene stays
        orig, tiles = tr.tile_data()
        assert np.array_equal(orig, kept)
        _assert_scene(d, b.packed)
        _assert_tiled_copy(d, orig)
        _assert_sampled_tiles(tiles, b.packed[0], orig)
        got = _frame(tr, cfg)
        assert sr._same_frame(got, b.fresh.frame)
    else:                                                                    # the Morton order depends on that box
        _assert_device_build(tr, cfg, b.packed, b.fresh)
        got = _frame(tr, cfg)
    o_argb, o_rgb = b.oracle
    assert np.array_equal(got[0].ravel()[b.pix], o_argb)
    assert np.array_equal(_u32(got[1][..., :3].reshape(-1, 3)[b.pix]), _u32(o_rgb))
    tr.close()


def _snapshot(tr, cfg):
    d = tr.scene_data(tiled=True)
    orig, tiles = tr.tile_data()
    argb, rgb = _frame(tr, cfg)
    return [_u32(d[k]) for k in ("vertices", "normals", "colors", "vertices_m", "normals_m", "colors_m", "vbox_lo", "vbox_hi")] + \
           [np.int64(d["n_shadow"]), orig, _u32(tiles), argb, _u32(rgb)]


@pytest.mark.parametrize("entry", ["update", "replace"])
def test_check_rejects_beyond_the_grid_cap(entry, big_check):
    import torch
    b = big_check
    cfg, n = b.cfg, b.n
    tr = rt.RayTracer(cfg, b.scene)
    before = _snapshot(tr, cfg)
    bad = _to_device(b.base.packed())                                        # another scene: an edit that got through would show
    for tri in (U.CHECK_GRID - 1, U.CHECK_GRID, n - 1):                      # the last lane of the first trip, the second trip
        for value in (float("nan"), float("inf"), 2.0 ** 17):
            row = 3 * tri + 1                                                # the triangle's second vertex
            old = bad[0][row].clone()
            bad[0][row, 1] = value
            torch.cuda.synchronize()
            with pytest.raises(rt.RtError) as e:
                if entry == "update":
                    _update_device(tr, bad)
                else:
                    _replace_device(tr, bad)
            assert e.value.code == abi.RT_E_INVALID, (tri, value)
            bad[0][row] = old
            after = _snapshot(tr, cfg)
            for k, (x, y) in enumerate(zip(before, after)):
                assert np.array_equal(x, y), (tri, value, k)
    _update_device(tr, bad)                                                  # the mended scene passes
    tr.close()


# ---- c. rt_pose_triangles beyond its grid cap and at the object limit --------------------------------------------------------
class BigPose:
    def __init__(self, box):
        nobj = self.nobj = U.MAX_OBJECTS
        self.cfg = _cfg()
        self.rest, self.ranges, self.centres = U.pose_scene(box, nobj)
        n = self.n = len(self.rest)
        assert nobj == 65535 and n == 26 + 65535 * 8 == 524306 and n > 2048 * 256
        assert self.ranges[-1] == (n - 8, 8) and n - U.POSE_GRID == 18        # 18 triangles in the loop's second trip
        self.xf = U.pose_xforms(self.centres)
        self.other = U.pose_xforms(self.centres, seed=10)
        self.posed = self.rest.posed(self.ranges, self.xf)
        self.packed = self.posed.packed()
        self.rest_packed = self.rest.packed()
        tr = rt.RayTracer(self.cfg, self.posed)
        self.fresh_frame = _frame(tr, self.cfg)
        tr.close()
        # a context given the same posed arrays through rt_update_scene, with the same flags
        tr = rt.RayTracer(self.cfg, self.rest)
        tr.update_scene(self.posed)
        self.ref = {0: tr.tile_data()}
        tr.update_scene(self.posed, device_tiles=True)
        self.ref[DEVICE_TILES] = tr.tile_data()
        tr.close()


@pytest.fixture(scope="module")
def big_pose(scene):
    return BigPose(scene)


@pytest.fixture(scope="module")
def pose_ctx(big_pose):
    """One context with the 65 535 objects per flags value (a refit keeps the order a device build before it left)."""
    made = {}

    def get(flags):
        if flags not in made:
            made[flags] = rt.RayTracer(big_pose.cfg, big_pose.rest)
            made[flags].set_objects(big_pose.ranges)
        return made[flags]
    yield get
    for tr in made.values():
        tr.close()


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("flags", [0, DEVICE_TILES])
def test_pose_beyond_the_grid_cap(entry, flags, big_pose, pose_ctx):
    import torch
    b = big_pose
    tr = pose_ctx(flags)
    assert tr.object_count() == 65535
    kw = {"device_tiles": True} if flags else {}
    tr.pose_objects(b.other, **kw)                                           # (another pose first: the next one has work to do)
    assert not np.array_equal(_u32(tr.scene_data()["vertices"]), _u32(b.packed[0]))
    if entry == "host":
        tr.pose_objects(b.xf, **kw)
    else:
        d_xf = torch.from_numpy(b.xf).cuda()
        torch.cuda.synchronize()
        tr.pose_objects_device(d_xf, stream=torch.cuda.Stream(), **kw)
        torch.cuda.synchronize()
    d = tr.scene_data(tiled=True)
    v, nr, c = b.packed
    assert np.array_equal(_u32(d["vertices"]), _u32(v))                      # Scene.posed, all n, objects 0 and 65534 included
    assert np.array_equal(_u32(d["normals"]), _u32(nr))
    assert np.array_equal(_u32(d["colors"]), _u32(b.rest_packed[2]))
    zero = U.special_poses(b.nobj)["zero"]
    assert b.nobj - 2 in zero
    for k in zero:                                                           # the collapsed objects: the host's NaN
        first = b.ranges[k][0]
        assert (_u32(d["normals"])[first:first + 8, :3] == 0xffc00000).all()
    orig, tiles = tr.tile_data()
    assert np.array_equal(orig, b.ref[flags][0]) and np.array_equal(_u32(tiles), _u32(b.ref[flags][1]))
    _assert_tiled_copy(d, orig)
    if flags:
        assert np.array_equal(orig, U.morton_order_np(v))
    assert sr._same_frame(_frame(tr, b.cfg), b.fresh_frame)


def test_pose_leaves_the_static_tail(big_pose):
    b = big_pose
    n = b.n
    ranges = [(26, 8), (1000, 300000), (400000, U.POSE_GRID - 400000)]       # the triangles from 524 288 on are in no object
    assert ranges[-1][0] + ranges[-1][1] == 2048 * 256 < n
    c0 = b.rest.aos[26:34, :3, :3].reshape(-1, 3).mean(axis=0).astype(np.float64)
    ang = 0.1
    rot = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    half = np.diag([0.5, 0.5, 0.5])
    xf = np.stack([np.concatenate([half, (c0 - half @ c0)[:, None]], 1),
                   np.concatenate([rot, np.array([[0.01], [0.0], [-0.02]])], 1),
                   np.concatenate([np.diag([-1.0, 1.0, 1.0]), np.array([[0.0], [0.02], [0.0]])], 1)]).astype(np.float32)
    want = b.rest.posed(ranges, xf).packed()
    tr = rt.RayTracer(b.cfg, b.rest)
    tr.set_objects(ranges)
    tr.pose_objects(xf)
    d = tr.scene_data()
    _assert_scene(d, (want[0], want[1], b.rest_packed[2]))
    tail = slice(U.POSE_GRID, n)
    assert np.array_equal(_u32(d["vertices"]).reshape(n, 12)[tail], _u32(b.rest_packed[0]).reshape(n, 12)[tail])
    assert np.array_equal(_u32(d["normals"])[tail], _u32(b.rest_packed[1])[tail])
    assert not np.array_equal(_u32(d["vertices"]).reshape(n, 12)[400000:U.POSE_GRID],
                              _u32(b.rest_packed[0]).reshape(n, 12)[400000:U.POSE_GRID])
    fresh = rt.RayTracer(b.cfg, b.rest.posed(ranges, xf))
    assert sr._same_frame(_frame(tr, b.cfg), _frame(fresh, b.cfg))
    fresh.close()
    tr.close()
