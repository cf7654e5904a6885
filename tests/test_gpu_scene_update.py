"""-m gpu: animated geometry — rt_update_scene / rt_update_scene_device replace a context's triangles between frames.
Every frame after an update is checked bit for bit (ARGB and the float tap) against the CPU oracle and against a fresh
context rt_init'ed with the new scene; the refit tile data against a float64 numpy restatement of rt_init's formulas."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, focal_for
from uob_raytracer_amd import abi, meshgen, runtime as rt

pytestmark = pytest.mark.gpu

VIEWS = [(0.0, 0.0, [0.0, 0.0, -3.2], [0.0, -0.5, -0.7]), (0.3, 0.1, [0.3, 0.2, -2.6], [0.2, -0.6, -0.4])]
SHORT_BLOCK = list(range(10, 18))          # the red block of LoadTestModel
SQUASH = np.diag([1.0, 0.5, 1.0])


def _frame(tr, cfg, view):
    yaw, pitch, cam, light = view
    return tr.render(rt.rotation_matrix(yaw, pitch), cam, light, focal_for(cfg), want_rgb=True)


def _check(tr, cfg, scene, oracle, views=VIEWS):
    """tr renders `scene` exactly as the oracle and as a fresh context do; returns the frames."""
    v, n, c = scene.packed()
    fresh = rt.RayTracer(cfg, scene)
    frames = []
    for view in views:
        argb, rgb = _frame(tr, cfg, view)
        yaw, pitch, cam, light = view
        o_argb, o_rgb = oracle.render(cfg, v, n, c, rt.rotation_matrix(yaw, pitch), cam, light, focal_for(cfg))
        assert np.array_equal(argb.ravel(), o_argb)
        assert np.array_equal(rgb[..., :3].reshape(-1, 3).view(np.uint32), o_rgb.view(np.uint32))
        f_argb, f_rgb = _frame(fresh, cfg, view)
        assert np.array_equal(argb, f_argb) and np.array_equal(rgb.view(np.uint32), f_rgb.view(np.uint32))
        frames.append((argb, rgb))
    fresh.close()
    return frames


def _box_scenes(box):
    moved = box.transformed(SHORT_BLOCK, np.eye(3), (0.25, 0.0, -0.125))
    # a wall into a mirror, a face of the tall block into glass (n_shadow changes)
    recol = moved.with_color([2, 3], (0.25, 0.0, 0.25, 0.0)).with_color([20, 21], (0.0, 0.2, 0.5, -1.0))
    return box, moved, recol


@pytest.mark.parametrize("flags", [0, abi.RT_FLAG_NO_CULL, abi.RT_FLAG_GENERIC_KERNEL])
def test_box_update_wave_kernel(flags, scene, oracle):
    cfg = abi.make_config(width=64, height=48, aa_x=2, aa_y=1, shadow_samples=4, flags=flags)
    a, b, c = _box_scenes(scene)
    tr = rt.RayTracer(cfg, a)
    first = _check(tr, cfg, a, oracle)
    tr.update_scene(b)
    moved = _check(tr, cfg, b, oracle)
    assert not np.array_equal(first[0][0], moved[0][0])
    tr.update_scene(c)
    _check(tr, cfg, c, oracle)
    tr.close()


def _mesh_scene(box, tmp_path, n_lon, n_lat):
    path = str(tmp_path / ("mesh_%d_%d.obj" % (n_lon, n_lat)))
    nf = meshgen.write_sphere_obj(path, n_lon, n_lat)
    return box + rt.Scene.load_obj(path), nf


def _mesh_sequence(both, nf):
    mesh = slice(26, 26 + nf)
    b = both.transformed(mesh, np.eye(3), (0.2, -0.05, -0.1))                    # rigid
    half = list(range(26, 26 + nf // 2))
    centre = both.aos[26:, :3, :3].reshape(-1, 3).mean(axis=0).astype(np.float32)
    c = both.transformed(half, SQUASH, centre - SQUASH.astype(np.float32) @ centre)   # squash half the mesh
    return b, c


@pytest.mark.parametrize("n_lon,n_lat", [(10, 8), (40, 30)])      # 166: one LDS stage; 2346: HBM records, tile masks
@pytest.mark.parametrize("flags", [0, abi.RT_FLAG_NO_TILE_BINS, abi.RT_FLAG_GENERIC_KERNEL])
@pytest.mark.parametrize("reorder", [False, True])
def test_mesh_sequence(n_lon, n_lat, flags, reorder, scene, oracle, tmp_path):
    both, nf = _mesh_scene(scene, tmp_path, n_lon, n_lat)
    b, c = _mesh_sequence(both, nf)
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3, flags=flags)
    tr = rt.RayTracer(cfg, both)
    first = _check(tr, cfg, both, oracle, VIEWS[:1])
    for s in (b, c, both):
        tr.update_scene(s, reorder=reorder)
        last = _check(tr, cfg, s, oracle, VIEWS[:1])
    assert np.array_equal(first[0][0], last[0][0]) and np.array_equal(first[0][1].view(np.uint32), last[0][1].view(np.uint32))
    tr.close()


def test_mesh_leaves_the_old_scene_box(scene, oracle, tmp_path):
    both, nf = _mesh_scene(scene, tmp_path, 40, 30)
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)        # tile masks on (> 1024 triangles)
    lo = both.aos[:, :3, :3].reshape(-1, 3).min(axis=0)
    for cen, r2, _ in abi.REFERENCE_SPHERES:
        lo = np.minimum(lo, np.asarray(cen, np.float32) - np.float32(np.sqrt(r2)) * 1.01)
    moved = both.transformed(slice(26, 26 + nf), np.eye(3), (0.0, 0.0, -1.2))
    assert (moved.aos[26:, :3, 2] < lo[2]).any()           # part of the mesh outside the box captured at rt_init
    tr = rt.RayTracer(cfg, both)
    _check(tr, cfg, both, oracle, VIEWS[:1])
    tr.update_scene(moved)
    _check(tr, cfg, moved, oracle)
    tr.close()


def tile_data_np(v4, orig):
    """upload_tiled_scene's per-tile data (rt_tile_sort.hip tile_data_host) restated in numpy float64 for a given order."""
    n = len(orig)
    V = v4.reshape(n, 3, 4)[:, :, :3][orig]
    out = np.zeros(((n + 63) // 64, 12), np.float32)
    for t in range(out.shape[0]):
        T = V[64 * t:64 * t + 64]
        a = T.astype(np.float64)
        e1, e2 = a[:, 1] - a[:, 0], a[:, 2] - a[:, 0]
        cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        norm = lambda x: np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        l1, l2, lc, l3 = norm(e1), norm(e2), norm(cr), norm(e2 - e1)
        degenerate = (~(lc > 1e-30) | ~(l1 > 0) | ~(l2 > 0) | ~(lc >= 1e-9 * l1 * l2)).any()
        ax, eta, emax, chi = np.array([1.0, 0.0, 0.0]), 1e30, 1e30, 4.0
        if not degenerate:
            le = np.maximum(np.maximum(l1, l2), l3)
            q = cr / lc[:, None]
            dot = (q[:, 0] * q[0, 0] + q[:, 1] * q[0, 1]) + q[:, 2] * q[0, 2]
            q[1:][dot[1:] < 0] *= -1.0
            s = np.zeros(3)
            for m in range(len(q)):                   # in triangle order, as the host adds
                s = s + q[m]
            la = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
            if la > 1e-12:
                ax = s / la
                d = q - ax
                chi, eta, emax = norm(d).max(), (le / lc).max(), le.max()
        out[t, 0:3], out[t, 4:7] = T.min(axis=(0, 1)), T.max(axis=(0, 1))
        out[t, 3], out[t, 7] = np.float32(eta * 1.0001), np.float32(emax * 1.0001)
        out[t, 8:11], out[t, 11] = ax.astype(np.float32), np.float32(chi * 1.0001 + 1e-6)
    return out


def _same_tiles(got, want):
    """Bit for bit; the boxes' min / max only up to the sign of a zero (min(+0, -0) is either)."""
    box = [0, 1, 2, 4, 5, 6]
    rest = [3, 7, 8, 9, 10, 11]
    return np.array_equal(got[:, box], want[:, box]) and np.array_equal(got[:, rest].view(np.uint32), want[:, rest].view(np.uint32))


def test_tile_data_after_refit(scene, tmp_path):
    both, nf = _mesh_scene(scene, tmp_path, 40, 30)
    b, c = _mesh_sequence(both, nf)
    cfg = abi.make_config(width=32, height=32, aa_x=1, aa_y=1, shadow_samples=1)
    tr = rt.RayTracer(cfg, both)
    orig0, tiles0 = tr.tile_data()
    assert _same_tiles(tiles0, tile_data_np(both.packed()[0], orig0))       # rt_init's host path
    for s in (b, c):
        tr.update_scene(s)
        orig, tiles = tr.tile_data()
        assert np.array_equal(orig, orig0)
        v4 = s.packed()[0]
        assert _same_tiles(tiles, tile_data_np(v4, orig))
        V = v4.reshape(-1, 3, 4)[:, :, :3][orig]
        for t in range(tiles.shape[0]):
            T = V[64 * t:64 * t + 64].reshape(-1, 3)
            assert (T >= tiles[t, 0:3]).all() and (T <= tiles[t, 4:7]).all()
    # the reorder path is rt_init's: the same order and tiles as a fresh context
    tr.update_scene(c, reorder=True)
    fresh = rt.RayTracer(cfg, c)
    (o1, t1), (o2, t2) = tr.tile_data(), fresh.tile_data()
    assert np.array_equal(o1, o2) and np.array_equal(t1.view(np.uint32), t2.view(np.uint32))
    assert not np.array_equal(o1, orig0)
    fresh.close()
    tr.close()


def _cuda_scene(scene):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in scene.packed()]


def _oracle_frame(oracle, cfg, scene, view):
    v, n, c = scene.packed()
    yaw, pitch, cam, light = view
    return oracle.render(cfg, v, n, c, rt.rotation_matrix(yaw, pitch), cam, light, focal_for(cfg))


def _render_dev(tr, cfg, view, out, stream):
    yaw, pitch, cam, light = view
    tr.render_device(rt.rotation_matrix(yaw, pitch), cam, light, focal_for(cfg), out[0].data_ptr(), out[1].data_ptr(),
                     stream=stream.cuda_stream)


def _same_as_oracle(out, want):
    argb, rgb = out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy()
    return np.array_equal(argb.ravel(), want[0]) and np.array_equal(rgb[..., :3].reshape(-1, 3).view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("n_lon,n_lat", [(10, 8), (40, 30)])
def test_device_entry_ordering(n_lon, n_lat, scene, oracle, tmp_path):
    import torch
    both, nf = _mesh_scene(scene, tmp_path, n_lon, n_lat)
    b, c = _mesh_sequence(both, nf)
    b = b.transformed(slice(26, 26 + nf), np.eye(3), (0.0, 0.0, -1.2))          # and out of the old box
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    scenes = [both, b, c]
    dev = [_cuda_scene(s) for s in scenes]
    outs = [(torch.zeros((48, 64), dtype=torch.int32, device="cuda"), torch.zeros((48, 64, 4), device="cuda")) for _ in range(3)]
    torch.cuda.synchronize()
    tr = rt.RayTracer(cfg, both)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    view = VIEWS[0]
    # render(A) -> update(B) -> render(B) -> update(C) -> render(C) on one non-default stream, no host sync in between
    _render_dev(tr, cfg, view, outs[0], s1)
    for k in (1, 2):
        tr.update_scene_device(*(t.data_ptr() for t in dev[k]), len(scenes[k]), stream=s1.cuda_stream)
        _render_dev(tr, cfg, view, outs[k], s1)
    s1.synchronize()
    for k in range(3):
        assert _same_as_oracle(outs[k], _oracle_frame(oracle, cfg, scenes[k], view)), "frame %d" % k
    # the update on a second stream between two frames on the first
    for o in outs:
        o[0].zero_(); o[1].zero_()
    torch.cuda.synchronize()
    _render_dev(tr, cfg, view, outs[0], s1)
    tr.update_scene_device(*(t.data_ptr() for t in dev[0]), len(both), stream=s2.cuda_stream)
    _render_dev(tr, cfg, view, outs[1], s1)
    s1.synchronize()
    assert _same_as_oracle(outs[0], _oracle_frame(oracle, cfg, c, view))
    assert _same_as_oracle(outs[1], _oracle_frame(oracle, cfg, both, view))
    # the device entry with RT_UPDATE_REORDER renders what the host entry does
    tr.update_scene_device(*(t.data_ptr() for t in dev[1]), len(b), stream=s2.cuda_stream, reorder=True)
    _check(tr, cfg, b, oracle, [view])
    tr.close()


def _bad_scenes(good):
    nan = good.aos.copy(); nan[30, 1, 2] = np.nan
    big = good.aos.copy(); big[40, 2, 0] = 2.0 ** 17
    return [rt.Scene(nan), rt.Scene(big)]


@pytest.mark.parametrize("n_lon,n_lat", [(10, 8), (40, 30)])
def test_rejected_updates_keep_the_scene(n_lon, n_lat, scene, tmp_path):
    import torch
    both, nf = _mesh_scene(scene, tmp_path, n_lon, n_lat)
    b, _ = _mesh_sequence(both, nf)
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    tr = rt.RayTracer(cfg, both)
    tr.update_scene(b)
    want = _frame(tr, cfg, VIEWS[0])
    v, n, c = b.packed()
    # a wrong triangle count, through both entries
    assert rt.lib().rt_update_scene(tr._h, rt._fp(v), rt._fp(n), rt._fp(c), len(b) - 1, 0) == abi.RT_E_INVALID
    dv = _cuda_scene(b)
    torch.cuda.synchronize()
    assert rt.lib().rt_update_scene_device(tr._h, *(rt.C.c_void_p(t.data_ptr()) for t in dv), len(b) + 1, 0, None) == abi.RT_E_INVALID
    for bad in _bad_scenes(both):
        for reorder in (False, True):
            with pytest.raises(rt.RtError) as e:
                tr.update_scene(bad, reorder=reorder)
            assert e.value.code == abi.RT_E_INVALID
            db = _cuda_scene(bad)
            torch.cuda.synchronize()
            with pytest.raises(rt.RtError) as e:
                tr.update_scene_device(*(t.data_ptr() for t in db), len(bad), reorder=reorder)
            assert e.value.code == abi.RT_E_INVALID
            got = _frame(tr, cfg, VIEWS[0])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    tr.close()


def test_multi_device_context(scene, oracle, tmp_path):
    import torch
    both, nf = _mesh_scene(scene, tmp_path, 40, 30)
    b, c = _mesh_sequence(both, nf)
    kw = dict(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=3)
    multi = rt.RayTracer(abi.make_config(devices=(0, 0), device_band_rows=8, **kw), both)
    single = rt.RayTracer(abi.make_config(**kw), both)
    cfg = abi.make_config(**kw)
    multi.update_scene(b)
    single.update_scene(b)
    for view in VIEWS:
        m, s = _frame(multi, cfg, view), _frame(single, cfg, view)
        assert np.array_equal(m[0], s[0]) and np.array_equal(m[1].view(np.uint32), s[1].view(np.uint32))
    dc = _cuda_scene(c)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    multi.update_scene_device(*(t.data_ptr() for t in dc), len(c), stream=stream.cuda_stream)
    stream.synchronize()
    got = _frame(multi, cfg, VIEWS[0])
    want = _oracle_frame(oracle, cfg, c, VIEWS[0])
    assert np.array_equal(got[0].ravel(), want[0]) and np.array_equal(got[1][..., :3].reshape(-1, 3).view(np.uint32), want[1].view(np.uint32))
    multi.close(); single.close()


@pytest.mark.parametrize("flags", [0, abi.RT_FLAG_GENERIC_KERNEL])
def test_work_counters_and_closest_hit_after_update(flags, scene, oracle, tmp_path):
    both, nf = _mesh_scene(scene, tmp_path, 10, 8)
    _, c = _mesh_sequence(both, nf)
    c = c.transformed(SHORT_BLOCK, np.eye(3), (0.125, 0.0, 0.0))
    cfg = abi.make_config(width=48, height=32, shadow_samples=4, flags=flags)
    tr = rt.RayTracer(cfg, both)
    tr.update_scene(c)
    v, n, col = c.packed()
    yaw, pitch, cam, light = VIEWS[1]
    rot = rt.rotation_matrix(yaw, pitch)
    _, _, want = oracle.render(cfg, v, n, col, rot, cam, light, focal_for(cfg), want_work=True)
    assert tr.count_work(rot, cam, light, focal_for(cfg)) == want
    rng = np.random.default_rng(5)
    d = rng.normal(size=(3000, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    start = rng.uniform(-0.9, 0.9, size=(3000, 3)).astype(np.float32)
    aim = c.aos[26:, :3, :3].reshape(-1, 3).mean(axis=0) - start[:1000]            # a third of the rays at the mesh
    d[:1000] = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    rays = np.concatenate([start, d], axis=1)
    tri, out = tr.trace_closest_hit(rays)
    o_tri, o_out = oracle.closest_hit(cfg, v, n, col, rays)
    assert np.array_equal(tri, o_tri)
    hit = tri != -1
    assert np.array_equal(out[hit].view(np.uint32), o_out[hit].view(np.uint32))
    assert (tri >= 26).any()
    tr.close()


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0,0"]])
def test_main_loop_moves_the_mesh(extra, scene, oracle, tmp_path):
    from test_host_surface import read_bmp
    exe = os.path.join(ROOT, "uob_raytracer_amd", "uob_raytracer")
    obj = str(tmp_path / "m.obj")
    meshgen.write_sphere_obj(obj, 10, 8)
    out = str(tmp_path / "shot.bmp")
    move = (0.03125, 0.0, -0.015625)
    frames = 4
    res = subprocess.run([exe, "--size", "128", "--frames", str(frames), "--obj", obj, "--move", "%r,%r,%r" % move,
                          "--out", out] + extra, check=True, capture_output=True, text=True)
    assert res.stdout.count("Frame Rate:") == frames
    # replay: the light animation of update() (skeleton.cpp:290-298) and the float32 moves
    f32 = np.float32
    lx, lor = f32(0.0), True
    mesh = rt.Scene.load_obj(obj)
    aos = mesh.aos.copy()
    for _ in range(frames):
        if lor:
            diff = f32(-0.5) - lx
            if diff > f32(-0.001):
                lor = False
        else:
            diff = f32(0.5) - lx
            if diff < f32(0.001):
                lor = True
        lx = lx + diff / f32(20.0)
        aos[:, :3, :3] += np.asarray(move, np.float32)
    moved = scene + rt.Scene(aos)
    cfg = abi.make_config(width=128, height=128)
    v, n, c = moved.packed()
    want, _ = oracle.render(cfg, v, n, c, rt.rotation_matrix(0.0, 0.0), [0.0, 0.0, -3.2], [lx, -0.5, -0.7],
                            1100.0 * 128 / 1024 * 2)
    got = read_bmp(out)
    assert np.array_equal(got.ravel(), want)
    assert ("light_position.x %.9g" % lx) in res.stdout
