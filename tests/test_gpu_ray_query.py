"""-m gpu: ray queries (rt_trace_rays / rt_trace_rays_device, rt_ray_query.hip) against the brute-force diagnostic
rt_debug_trace_rays and the CPU oracle, bit for bit: tri, and out10 as uint32 on hits.  Golden vectors, camera-like,
shadow-from-hit and random rays on the box and box + meshes, directed cases where the tile certificates are tightest,
scene updates, context variants, queries between frames, and the culling counters."""
import os

import numpy as np
import pytest

from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, meshgen, runtime as rt

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
CFG = dict(width=64, height=64)
MESHES = {"166": (10, 8), "2346": (40, 30), "20000": (100, 101)}


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(G, "function_vectors.npz"))


@pytest.fixture(scope="module")
def meshes(scene, tmp_path_factory):
    d = tmp_path_factory.mktemp("meshes")
    out = {}
    for name, (lon, lat) in MESHES.items():
        path = str(d / ("m%s.obj" % name))
        meshgen.write_sphere_obj(path, lon, lat)
        out[name] = scene + rt.Scene.load_obj(path)
    return out


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def camera_rays(k, seed=0, cam=DEFAULT_CAM, step=3):
    """k rays from the camera through pixels of a 1024^2 view at focal length 1100 (directions normalised in float32),
    jittered inside the pixel: every `step`-th pixel of a window around the meshes, rows of 64, row-major, so that a wave's
    64 rays are neighbours in a row as they are for a real camera."""
    rng = np.random.default_rng(seed)
    yy, xx = np.divmod(np.arange(k), 64)
    x = 336.0 - 32 * step + step * xx + rng.random(k)
    y = 853.0 - step * (k // 128) + step * yy + rng.random(k)
    d = np.stack([x - 512.0, y - 512.0, np.full(k, 1100.0)], 1).astype(np.float32)
    d /= np.sqrt((d * d).sum(1, keepdims=True)).astype(np.float32)
    s = np.broadcast_to(np.asarray(cam, np.float32), (k, 3))
    return np.ascontiguousarray(np.concatenate([s, d], 1), np.float32)


def random_rays(k, seed=1):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-0.99, 0.99, (k, 3)).astype(np.float32)
    d = rng.normal(size=(k, 3)).astype(np.float32)
    d /= np.sqrt((d * d).sum(1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([s, d], 1), np.float32)


def shadow_rays(tri, out, light=DEFAULT_LIGHT):
    """From each hit point towards the light, as direct_light sets them up (kernels.cl:323-326), in float32."""
    p = out[tri != -1, 0:3].astype(np.float32)
    d = (np.asarray(light, np.float32) - p).astype(np.float32)
    s = (p + np.float32(1e-4) * d).astype(np.float32)
    r2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([s, d], 1), np.float32), r2


def check_closest(tr, rays, want=None):
    """query == brute force (== want, e.g. the oracle's answer, when given); returns the query's (tri, out)."""
    tri, out = tr.query_closest_hit(rays)
    b_tri, b_out = tr.trace_closest_hit(rays)
    assert np.array_equal(tri, b_tri)
    hit = tri != -1
    assert np.array_equal(_u32(out[hit]), _u32(b_out[hit]))
    assert not out[~hit].any()
    if want is not None:
        assert np.array_equal(tri, want[0])
        assert np.array_equal(_u32(out[hit]), _u32(want[1][hit]))
    return tri, out


def check_shadow(tr, rays, r2, want=None):
    got = tr.query_in_shadow(rays, r2)
    assert np.array_equal(got, tr.trace_in_shadow(rays, r2))
    if want is not None:
        assert np.array_equal(got, want)
    return got


def check_with_oracle(tr, oracle, sc, rays, r2=None):
    cfg = tr.cfg
    v, n, c = sc.packed()
    if r2 is None:
        return check_closest(tr, rays, oracle.closest_hit(cfg, v, n, c, rays))
    return check_shadow(tr, rays, r2, oracle.in_shadow(cfg, v, c, rays, r2))


# ---- 1. the box with the reference's spheres: the reference's recorded outputs -------------------------------------------
def test_box_golden_vectors(scene, vectors):
    import torch
    tr = rt.RayTracer(abi.make_config(**CFG), scene)
    check_shadow(tr, vectors["rays"], vectors["radius_sq"], vectors["in_shadow"])
    check_closest(tr, vectors["rays_unit"], (vectors["hit_tri"], vectors["hit_out"]))
    # the device entry on torch tensors
    dev = torch.device("cuda", torch.cuda.current_device())
    rays = torch.from_numpy(np.ascontiguousarray(vectors["rays"], np.float32)).to(dev)
    r2 = torch.from_numpy(np.ascontiguousarray(vectors["radius_sq"], np.float32)).to(dev)
    sh = tr.query_device(abi.RT_TRACE_IN_SHADOW, rays, r2)
    unit = torch.from_numpy(np.ascontiguousarray(vectors["rays_unit"], np.float32)).to(dev)
    out10 = torch.full((unit.shape[0], 10), 7.0, device=dev)           # the device entry writes the zeros of a miss itself
    tri, out = tr.query_device(abi.RT_TRACE_CLOSEST_HIT, unit, out10=out10)
    torch.cuda.synchronize()
    assert out is out10
    assert np.array_equal(sh.cpu().numpy().astype(np.uint8), vectors["in_shadow"])
    tri, out = tri.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(tri, vectors["hit_tri"])
    hit = tri != -1
    assert np.array_equal(_u32(out[hit]), _u32(vectors["hit_out"][hit])) and not out[~hit].any()
    st = tr.trace_stats()
    assert st["rays"] == unit.shape[0] and st["tiles"] == 0 and st["unculled_rays"] == unit.shape[0]
    with pytest.raises(ValueError):
        tr.query_device(abi.RT_TRACE_CLOSEST_HIT, unit.double())
    with pytest.raises(ValueError):
        tr.query_device(abi.RT_TRACE_IN_SHADOW, rays)                  # radius_sq missing
    with pytest.raises(ValueError):
        tr.query_device(abi.RT_TRACE_CLOSEST_HIT, unit.cpu())
    tr.close()


# ---- 2. box + meshes: golden, camera-like, shadow-from-hit and random rays -------------------------------------------------
@pytest.mark.parametrize("name", ["166", "2346", "20000"])
def test_meshes_against_oracle_and_brute_force(name, meshes, oracle, vectors):
    sc = meshes[name]
    tr = rt.RayTracer(abi.make_config(**CFG), sc)
    k = 3000
    check_with_oracle(tr, oracle, sc, vectors["rays"][:k], vectors["radius_sq"][:k])
    check_with_oracle(tr, oracle, sc, vectors["rays_unit"][:k])
    cam = camera_rays(k)
    tri, out = check_with_oracle(tr, oracle, sc, cam)
    assert (tri >= 26).sum() > k // 10                                  # the mesh is in view
    srays, r2 = shadow_rays(tri, out)
    blocked = check_with_oracle(tr, oracle, sc, srays, r2)
    assert 0 < blocked.sum() < len(blocked)
    rnd = random_rays(k)
    check_with_oracle(tr, oracle, sc, rnd)
    check_with_oracle(tr, oracle, sc, rnd, np.full(k, 0.5, np.float32))
    tr.close()


def test_100k_mesh_against_brute_force(scene, tmp_path):
    path = str(tmp_path / "m100k.obj")
    assert meshgen.write_sphere_obj(path, 256, 196) + len(scene) == 99866
    tr = rt.RayTracer(abi.make_config(**CFG), scene + rt.Scene.load_obj(path))
    tri, out = check_closest(tr, camera_rays(4096, seed=3))
    assert (tri >= 26).any()
    srays, r2 = shadow_rays(tri, out)
    check_shadow(tr, srays, r2)
    check_closest(tr, random_rays(2048, seed=4))
    st = tr.trace_stats()
    assert st["tiles"] == (99866 + 26 + 63) // 64 and st["tested_tiles"] < st["waves"] * st["tiles"]
    tr.close()


# ---- 3. directed cases on a tiled mesh ----------------------------------------------------------------------------------
def _ulp_steps(a, steps):
    """Every row of a [k, 6] float32 array with its start and direction moved by each of `steps` ulps (through the bits)."""
    out = [a]
    for s in steps:
        b = a.copy().view(np.int32)
        b += np.int32(s) * np.sign(b + (b == 0)).astype(np.int32)
        out.append(b.view(np.float32))
    return np.ascontiguousarray(np.concatenate(out, 0), np.float32)


def test_directed_cases(meshes, oracle, vectors):
    sc = meshes["2346"]
    tr = rt.RayTracer(abi.make_config(**CFG), sc)
    aos = sc.aos
    idx = np.arange(26, len(sc), 37)
    v0, v1, v2 = aos[idx, 0, :3], aos[idx, 1, :3], aos[idx, 2, :3]
    e1, e2 = (v1 - v0).astype(np.float32), (v2 - v0).astype(np.float32)
    steps = [1, -1, 2, -2, 8, -8, 64, -64]
    # in a triangle's plane: along an edge from outside it, and inside the plane through the triangle
    inplane = np.concatenate([np.concatenate([v0 - 0.5 * e1, e1], 1), np.concatenate([v0 - 0.25 * (e1 + e2), e1 + e2], 1),
                              np.concatenate([v0 + 0.5 * e1 - e2, e2 - 0.25 * e1], 1)]).astype(np.float32)
    check_with_oracle(tr, oracle, sc, _ulp_steps(inplane, steps))
    check_with_oracle(tr, oracle, sc, _ulp_steps(inplane, steps), np.full(len(inplane) * 9, 4.0, np.float32))
    # through shared vertices and edge midpoints (equal t on neighbouring triangles: the lowest original index wins)
    cam = np.asarray(DEFAULT_CAM, np.float32)
    targets = np.concatenate([v0, v1, (0.5 * (v0 + v1)).astype(np.float32), (0.5 * (v1 + v2)).astype(np.float32)])
    d = (targets - cam).astype(np.float32)
    through = np.ascontiguousarray(np.concatenate([np.broadcast_to(cam, d.shape), d], 1), np.float32)
    tri, out = check_with_oracle(tr, oracle, sc, _ulp_steps(through, [1, -1]))
    # starting exactly on a surface (t = 0), moving on in the same direction and back out
    hit = tri != -1
    start = out[hit, 0:3]
    dirs = _ulp_steps(through, [1, -1])[hit, 3:6]
    on = np.ascontiguousarray(np.concatenate([np.concatenate([start, dirs], 1), np.concatenate([start, -dirs], 1)]), np.float32)
    check_with_oracle(tr, oracle, sc, on)
    check_with_oracle(tr, oracle, sc, on, np.full(len(on), 1.0, np.float32))
    # touching a tile box face: rays in the plane of a face, and one ulp either side of it
    _, tiles = tr.tile_data()
    lo, hi = tiles[:, 0:3], tiles[:, 4:7]
    mid = (0.5 * (lo + hi)).astype(np.float32)
    face = []
    for ax in range(3):
        o = mid.copy()
        o[:, ax] = lo[:, ax]
        o[:, (ax + 1) % 3] -= 3.0
        dd = np.zeros_like(o)
        dd[:, (ax + 1) % 3] = 1.0
        face.append(np.concatenate([o, dd], 1))
    check_with_oracle(tr, oracle, sc, _ulp_steps(np.concatenate(face).astype(np.float32), [1, -1, 4, -4]))
    # grazing the reference's spheres (discriminant near 0)
    graze = []
    for s in tr.cfg.spheres[:tr.cfg.num_spheres]:
        c = np.asarray(s.center, np.float32)
        r = np.float32(np.sqrt(np.float32(s.radius_sq)))
        for ax in range(3):
            o = c.copy()
            o[ax] += r
            o[(ax + 1) % 3] -= 2.0
            dd = np.zeros(3, np.float32)
            dd[(ax + 1) % 3] = 1.0
            graze.append(np.concatenate([o, dd]))
    graze = _ulp_steps(np.asarray(graze, np.float32), [1, -1, 2, -2, 16, -16])
    check_with_oracle(tr, oracle, sc, graze)
    check_with_oracle(tr, oracle, sc, graze, np.full(len(graze), 16.0, np.float32))
    # zero, tiny, NaN and infinite directions, starts beyond 2^16: outside the certificates' domain
    base = camera_rays(64, seed=5)
    odd = []
    for dvec in ([0, 0, 0], [2.0 ** -30, 0, 0], [2.0 ** -30, -(2.0 ** -31), 2.0 ** -30], [np.nan, 0, 1], [0, np.inf, 1],
                 [-np.inf, 0, 0], [2.0 ** 17, 1, 1]):
        r = base[:16].copy()
        r[:, 3:6] = np.asarray(dvec, np.float32)
        odd.append(r)
    far = base[:16].copy()
    far[:, 0:3] = np.float32(2.0 ** 17)
    far[:, 3:6] = -far[:, 0:3] / np.float32(2.0 ** 17)
    odd.append(far)
    nan_start = base[:16].copy()
    nan_start[:, 1] = np.nan
    odd.append(nan_start)
    odd = np.concatenate(odd + [base]).astype(np.float32)             # in-domain rays in the same waves
    check_with_oracle(tr, oracle, sc, odd)
    assert tr.trace_stats()["unculled_rays"] == len(odd) - 64            # every ray but the in-domain ones
    check_with_oracle(tr, oracle, sc, odd, np.full(len(odd), 9.0, np.float32))
    assert tr.trace_stats()["unculled_rays"] == len(odd) - 64
    tr.close()
    # glass mesh triangles cast no shadow
    mesh = list(range(26, len(sc)))
    glass = sc.with_color(mesh[::2], (0.1, 0.2, 0.3, -1.0))
    tg = rt.RayTracer(abi.make_config(**CFG), glass)
    tri, out = check_with_oracle(tg, oracle, glass, camera_rays(2000, seed=6))
    srays, r2 = shadow_rays(tri, out)
    check_with_oracle(tg, oracle, glass, srays, r2)
    check_with_oracle(tg, oracle, glass, random_rays(2000, seed=7), np.full(2000, 1.0, np.float32))
    tg.close()


# ---- 4. scene changes --------------------------------------------------------------------------------------------------
def _answers(tr, rays, r2):
    tri, out = tr.query_closest_hit(rays)
    return tri, _u32(out), tr.query_in_shadow(rays, r2)


def _same_answers(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_scene_updates(meshes):
    import torch
    a = meshes["2346"]
    nf = len(a) - 26
    b = a.transformed(slice(26, 26 + nf), np.eye(3), (0.2, -0.05, -0.1))
    c = a.transformed(list(range(26, 26 + nf // 2)), np.diag([1.0, 0.5, 1.0]))
    cfg = abi.make_config(**CFG)
    rays = np.concatenate([camera_rays(2000, seed=8), random_rays(2000, seed=9)])
    r2 = np.full(len(rays), 2.0, np.float32)
    fresh = {}
    for name, sc in (("a", a), ("b", b), ("c", c)):
        f = rt.RayTracer(cfg, sc)
        fresh[name] = _answers(f, rays, r2)
        f.close()
    tr = rt.RayTracer(cfg, a)
    tr.update_scene(b)                                      # refit
    _same_answers(_answers(tr, rays, r2), fresh["b"])
    tr.update_scene(c, reorder=True)
    _same_answers(_answers(tr, rays, r2), fresh["c"])
    dev = {k: [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in sc.packed()] for k, sc in (("a", a), ("b", b))}
    torch.cuda.synchronize()
    tr.update_scene_device(*(t.data_ptr() for t in dev["a"]), len(a))
    _same_answers(_answers(tr, rays, r2), fresh["a"])
    # a query on one stream after an update on another sees the new scene
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_rays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    tr.update_scene_device(*(t.data_ptr() for t in dev["b"]), len(b), stream=s1.cuda_stream)
    tri, out = tr.query_device(abi.RT_TRACE_CLOSEST_HIT, d_rays, stream=s2)
    s2.synchronize()
    assert np.array_equal(tri.cpu().numpy(), fresh["b"][0]) and np.array_equal(_u32(out.cpu().numpy()), fresh["b"][1])
    # a large query enqueued before a (blocking, host) update answers for the old scene
    torch.cuda.synchronize()
    big = torch.from_numpy(np.concatenate([random_rays(1 << 18, seed=10), rays])).cuda()
    torch.cuda.synchronize()
    tri, out = tr.query_device(abi.RT_TRACE_CLOSEST_HIT, big, stream=s1)
    tr.update_scene(a)
    s1.synchronize()
    tail = tri.cpu().numpy()[1 << 18:], _u32(out.cpu().numpy()[1 << 18:])
    assert np.array_equal(tail[0], fresh["b"][0]) and np.array_equal(tail[1], fresh["b"][1])
    _same_answers(_answers(tr, rays, r2), fresh["a"])
    tr.close()


# ---- 5. context variants ------------------------------------------------------------------------------------------------
def test_context_variants(scene, meshes, oracle, tmp_path):
    sc = meshes["2346"]
    rays = np.concatenate([camera_rays(1500, seed=11), random_rays(1500, seed=12)])
    r2 = np.full(len(rays), 3.0, np.float32)
    ref = rt.RayTracer(abi.make_config(**CFG), sc)
    want = _answers(ref, rays, r2)
    ref.close()
    for flags in (abi.RT_FLAG_GENERIC_KERNEL, abi.RT_FLAG_NO_TILE_BINS):        # n > 512 without tiles; tiles without masks
        tr = rt.RayTracer(abi.make_config(flags=flags, **CFG), sc)
        _same_answers(_answers(tr, rays, r2), want)
        assert (tr.trace_stats()["tiles"] == 0) == (flags == abi.RT_FLAG_GENERIC_KERNEL)
        tr.close()
    multi = rt.RayTracer(abi.make_config(devices=(0, 0), **CFG), sc)
    _same_answers(_answers(multi, rays, r2), want)
    multi.close()
    # around the tiling threshold: 64 triangles (no tiled copy) and 65 (one full tile and a tile of one)
    path = str(tmp_path / "small.obj")
    meshgen.write_sphere_obj(path, 20, 2)
    small = scene + rt.Scene.load_obj(path)
    for n in (64, 65):
        sn = rt.Scene(small.aos[:n])
        tr = rt.RayTracer(abi.make_config(**CFG), sn)
        check_with_oracle(tr, oracle, sn, rays)
        check_with_oracle(tr, oracle, sn, rays, r2)
        assert tr.trace_stats()["tiles"] == (0 if n == 64 else 2)
        tr.close()


# ---- 6. queries between frames ------------------------------------------------------------------------------------------
def test_queries_between_frames(meshes):
    import torch
    sc = meshes["2346"]
    cfg = abi.make_config(width=128, height=96, shadow_samples=4)
    view = (rt.rotation_matrix(0.1, 0.0), DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg))
    plain = rt.RayTracer(cfg, sc)
    want = plain.render(*view)
    plain.close()
    tr = rt.RayTracer(cfg, sc)
    rays = camera_rays(3000, seed=13)
    assert np.array_equal(tr.render(*view), want)
    tri, _ = tr.query_closest_hit(rays)
    assert np.array_equal(tr.render(*view), want)
    # device entries on two streams: frame, query, frame without a host synchronisation in between
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    frames = [torch.zeros((96, 128), dtype=torch.int32, device="cuda") for _ in range(2)]
    d_rays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    tr.render_device(*view, frames[0].data_ptr(), stream=s1.cuda_stream)
    q_tri, _ = tr.query_device(abi.RT_TRACE_CLOSEST_HIT, d_rays, stream=s2)
    tr.render_device(*view, frames[1].data_ptr(), stream=s1.cuda_stream)
    torch.cuda.synchronize()
    for f in frames:
        assert np.array_equal(f.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(q_tri.cpu().numpy(), tri)
    tr.close()


# ---- 7. the culling is real --------------------------------------------------------------------------------------------
def test_culling_counters(meshes):
    tr = rt.RayTracer(abi.make_config(**CFG), meshes["2346"])
    # 64 waves spread over the 1024^2 frame, each the 64 neighbouring pixels of a row segment (what a camera hands a wave)
    w = np.arange(4096) // 64
    x, y = 64 * (w % 16) + np.arange(4096) % 64 + 0.5, 16 * w + 8.5
    d = np.stack([x - 512.0, y - 512.0, np.full(4096, 1100.0)], 1).astype(np.float32)
    d /= np.sqrt((d * d).sum(1, keepdims=True)).astype(np.float32)
    rays = np.ascontiguousarray(np.concatenate([np.broadcast_to(np.float32(DEFAULT_CAM), d.shape), d], 1), np.float32)
    tri, _ = check_closest(tr, rays)
    assert (tri >= 26).any()
    tr.query_closest_hit(rays)
    st = tr.trace_stats()
    print("camera rays, 2346-triangle mesh:", st)
    assert st["rays"] == 4096 and st["waves"] == 64 and st["tiles"] == (2346 + 63) // 64 and st["unculled_rays"] == 0
    assert st["tested_tiles"] <= st["bundle_tiles"] <= st["waves"] * st["tiles"]
    assert st["tested_tiles"] < 0.5 * st["waves"] * st["tiles"]
    assert st["triangle_tests"] < 0.25 * 64 * st["waves"] * 2346
    assert st["tested_tiles"] <= 480 and st["triangle_tests"] <= 192000      # measured on an MI355X: 381 and 153 408
    tr.close()
