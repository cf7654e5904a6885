"""-m gpu: rt_radiance_rays / rt_radiance_rays_device (rt_radiance.hip) against the frame itself — with the AOV `direction`
plane as rays and the pixel ids as seeds the call must reproduce rt_render's float output and the oracle's on EVERY pixel,
mirror and glass included — and against tests/radiance_util.py, the bounce loop and colour rules restated in numpy FP32 with
hits and masks from the CPU oracle and from the brute-force diagnostic rt_debug_trace_rays.  Bit for bit (uint32 views)."""
import numpy as np
import pytest

import aov_util
import radiance_util as ru
import shade_util as su
from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, meshgen, runtime as rt

pytestmark = pytest.mark.gpu

F = np.float32
VIEWS = {"default": (0.0, 0.0), "yawed": (0.3, 0.0)}


@pytest.fixture(scope="module")
def meshes(scene, tmp_path_factory):
    d = tmp_path_factory.mktemp("radiance_meshes")
    small, big = str(d / "m2346.obj"), str(d / "m20000.obj")
    meshgen.write_sphere_obj(small, 40, 30)
    meshgen.write_sphere_obj(big, 100, 101)
    return {"box": scene,
            "2346": scene + rt.Scene.load_obj(small),
            "glass": scene + rt.Scene.load_obj(small, color=(0.9, 0.9, 0.9, -1.0)),
            "mirror": scene + rt.Scene.load_obj(small, color=(0.0, 0.0, 0.0, 0.0)),
            "20000": scene + rt.Scene.load_obj(big, color=(0.0, 0.0, 0.0, 0.0))}


def all_diffuse(sc):
    for i in np.flatnonzero(sc.aos[:, 4, 3] <= 0):
        sc = sc.with_color([int(i)], tuple(sc.aos[i, 4, :3]) + (0.5,))
    return sc


def oracle_calls(oracle, cfg, sc):
    v, n, c = sc.packed()
    return (lambda rays: oracle.closest_hit(cfg, v, n, c, rays)), (lambda rays, r2: oracle.in_shadow(cfg, v, c, rays, r2))


def restate(tr, rays, seeds, calls, light=DEFAULT_LIGHT):
    cfg = tr.cfg
    return ru.radiance(rays, seeds, light, cfg.shadow_samples, cfg.light_spread, cfg.max_bounces, *calls)


def assert_same(got, want, what):
    bad = np.argwhere(~su.same_bits(got, want))
    assert bad.size == 0, "%s: %d elements differ, first at %s: got %r, want %r" % (
        what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- a. the frame from public pieces, nothing excluded -------------------------------------------------------------------
def frame_identity(oracle, sc, cfg, view):
    rot, focal = rt.rotation_matrix(*VIEWS[view]), focal_for(cfg)
    aa = cfg.aa_x * cfg.aa_y
    tr = rt.RayTracer(cfg, sc)
    _, rgb = tr.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal, want_rgb=True)
    v, n, c = sc.packed()
    _, o_rgb = oracle.render(cfg, v, n, c, rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    o_rgb = o_rgb.reshape(cfg.height, cfg.width, 3)
    aov = tr.render_aov(rot, DEFAULT_CAM, focal, sample=None if aa > 1 else 0, planes=("prim", "albedo", "direction"))
    shape = aov["prim"].shape                                    # [H, W] or [H, W, aa]
    ids = su.pixel_ids(range(cfg.height), cfg.width)
    ids = np.broadcast_to(ids.reshape(ids.shape + (1,) * (len(shape) - 2)), shape)
    rays = aov_util.rays_of(DEFAULT_CAM, aov["direction"][..., :3])
    rgba, prim = tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=ids.reshape(-1), want_prim=True)
    st = tr.radiance_stats()
    col = rgba[:, :3].reshape(cfg.height, cfg.width, aa, 3)
    col = ru.pixel_colour(col)                                   # the pixel: float32 sum in sample order, / aa
    assert np.array_equal(su.u32(col), su.u32(rgb[..., :3]))     # every pixel
    assert np.array_equal(su.u32(col), su.u32(o_rgb))
    assert np.array_equal(prim.reshape(shape), aov["prim"])
    assert np.array_equal(rgba[:, 3], (prim != -1).astype(F))
    hit = aov["prim"] != -1
    specular = hit & (aov["albedo"][..., 3] <= 0)
    print("%s S=%d aa=%d bounces=%d: %d specular samples, stats %s" % (view, cfg.shadow_samples, aa, cfg.max_bounces, specular.sum(), st))
    assert specular.sum() > 0 and st["rays"] == rays.shape[0]
    # every specular first hit takes bounce 0; more bounce rays than that means some ray took two or more
    if cfg.max_bounces >= 2:
        assert st["bounce_rays"] > specular.sum()
    else:
        assert st["bounce_rays"] == (specular.sum() if cfg.max_bounces == 1 else 0)
    assert st["shaded_points"] >= (hit & ~specular).sum()
    tr.close()


@pytest.mark.parametrize("view", ["default", "yawed"])
@pytest.mark.parametrize("samples", [1, 10, 64, 100])
@pytest.mark.parametrize("name", ["box", "2346"])
def test_frame_identity(name, samples, view, meshes, oracle):
    frame_identity(oracle, meshes[name], abi.make_config(width=96, height=96, aa_x=1, aa_y=1, shadow_samples=samples), view)


@pytest.mark.parametrize("name", ["box", "2346"])
def test_frame_identity_2x2(name, meshes, oracle):
    frame_identity(oracle, meshes[name], abi.make_config(width=64, height=64, aa_x=2, aa_y=2, shadow_samples=10), "default")


@pytest.mark.parametrize("max_bounces", [0, 1, 10])
@pytest.mark.parametrize("name", ["box", "2346"])
def test_frame_identity_max_bounces(name, max_bounces, meshes, oracle):
    cfg = abi.make_config(width=96, height=96, aa_x=1, aa_y=1, shadow_samples=10, max_bounces=max_bounces)
    frame_identity(oracle, meshes[name], cfg, "default")


@pytest.mark.parametrize("name", ["glass", "mirror"])
def test_frame_identity_specular_mesh(name, meshes, oracle):
    """The bounce rays of a glass / mirror mesh go through the tiled walk"""
    frame_identity(oracle, meshes[name], abi.make_config(width=96, height=96, aa_x=1, aa_y=1, shadow_samples=10), "default")


# ---- b. arbitrary rays -----------------------------------------------------------------------------------------------------
def random_rays(k, seed):
    """Origins uniform in the box, directions random and NOT normalised (lengths over twelve octaves), seeds over the whole
    domain with 0 and 2^24 present; then NaN, infinite and out-of-domain rays in fixed rows"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.99, 0.99, (k, 3)).astype(F)
    d = rng.normal(size=(k, 3)).astype(F)
    d = (d * np.exp2(rng.uniform(-6.0, 6.0, (k, 1))).astype(F)).astype(F)
    seeds = rng.integers(0, (1 << 24) + 1, k).astype(np.int32)
    seeds[0], seeds[1] = 0, 1 << 24
    rays = np.ascontiguousarray(np.concatenate([o, d], 1), F)
    if k >= 64:
        rays[5, 4] = np.nan                                      # NaN direction
        rays[6, 0] = np.nan                                      # NaN start
        rays[7, 3] = np.inf                                      # infinite direction
        rays[8, 1] = -np.inf                                     # infinite start
        rays[9, 3:6] = 0.0                                       # no direction at all
        rays[10:14, 3:6] *= F(2.0 ** -30)                        # below 2^-20: outside the culls' domain
        rays[14:18, 3:6] *= F(2.0 ** 24)                         # above 2^16
        rays[18:22, 0:3] = (rays[18:22, 0:3] - rays[18:22, 3:6] / np.abs(rays[18:22, 3:6]).max(1, keepdims=True) * F(2.0 ** 17)).astype(F)
    return rays, seeds


@pytest.mark.parametrize("name", ["box", "glass", "mirror", "diffuse_box"])
def test_arbitrary_rays(name, meshes, oracle):
    sc = all_diffuse(meshes["box"]) if name == "diffuse_box" else meshes[name]
    cfg = abi.make_config(width=64, height=64, shadow_samples=10, spheres=() if name == "diffuse_box" else abi.REFERENCE_SPHERES)
    tr = rt.RayTracer(cfg, sc)
    rays, seeds = random_rays(20000 + 37, seed=len(sc))
    got, prim = tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=seeds, want_prim=True)
    st = tr.radiance_stats()
    for label, calls in (("oracle", oracle_calls(oracle, cfg, sc)), ("brute force", (tr.trace_closest_hit, tr.trace_in_shadow))):
        want = restate(tr, rays, seeds, calls)
        assert_same(got, want["rgba"], "%s, %s" % (name, label))
        assert np.array_equal(prim, want["prim"])
    assert not got[5:10].any()                                   # NaN / infinite / degenerate rays hit nothing
    assert (st["rays"], st["bounce_rays"], st["shaded_points"]) == (len(rays), int(want["bounces"].sum()), int(want["diffuse"].sum()))
    # rays traced without culling: the caller's rays outside the domain, and NaN bounce rays behind a total internal reflection
    assert st["unculled_rays"] == want["unculled"] >= 12
    if name == "diffuse_box":
        assert not want["specular"].any() and st["bounce_rays"] == 0
    else:
        assert want["specular"].any() and (want["bounces"] >= 2).any()
    # any number of rays: a ray's result does not depend on its neighbours
    for m in (1, 63, 65, 1000):
        sub = tr.radiance_rays(rays[:m], DEFAULT_LIGHT, seeds=seeds[:m])
        assert_same(sub, want["rgba"][:m], "%s, first %d rays" % (name, m))
    tr.close()


@pytest.mark.parametrize("flags", [abi.RT_FLAG_GENERIC_KERNEL])
@pytest.mark.parametrize("samples", [10, 100])
def test_arbitrary_rays_without_a_tiled_copy(flags, samples, meshes, oracle):
    """RT_FLAG_GENERIC_KERNEL: the walks' BOXES = false form, on a mesh and on the box; and more than 64 samples"""
    for name in ("glass", "box"):
        sc = meshes[name]
        cfg = abi.make_config(width=64, height=64, shadow_samples=samples, flags=flags)
        tr = rt.RayTracer(cfg, sc)
        rays, seeds = random_rays(3000 if samples == 10 else 600, seed=samples)
        got = tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=seeds)
        want = restate(tr, rays, seeds, (tr.trace_closest_hit, tr.trace_in_shadow))
        assert_same(got, want["rgba"], "%s without a tiled copy" % name)
        tr.close()
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=samples), meshes["mirror"])      # tiled, S as given
    rays, seeds = random_rays(2000, seed=samples + 1)
    assert_same(tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=seeds),
                restate(tr, rays, seeds, oracle_calls(oracle, tr.cfg, meshes["mirror"]))["rgba"], "mirror mesh, S = %d" % samples)
    tr.close()


# ---- c. the entries ----------------------------------------------------------------------------------------------------------
def test_entries(meshes):
    import torch
    sc = meshes["glass"]
    cfg = abi.make_config(width=64, height=64, shadow_samples=10)
    tr = rt.RayTracer(cfg, sc)
    rays, _ = random_rays(5000 + 13, seed=3)
    host, hprim = tr.radiance_rays(rays, DEFAULT_LIGHT, want_prim=True)                  # seeds = None
    seeds = (np.arange(len(rays)) & 0xFFFFFF).astype(np.int32)
    assert_same(tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=seeds), host, "explicit k & 0xFFFFFF")
    d_rays, d_seeds = torch.from_numpy(rays).cuda(), torch.from_numpy(seeds).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    d_prim = torch.empty(len(rays), dtype=torch.int32, device="cuda")
    out, d_prim = tr.radiance_rays_device(d_rays, DEFAULT_LIGHT, seeds=d_seeds, out_prim=d_prim, stream=s)
    only = tr.radiance_rays_device(d_rays, DEFAULT_LIGHT, stream=s)                      # no seeds, no prim
    s.synchronize()
    assert_same(out.cpu().numpy(), host, "device entry")
    assert_same(only.cpu().numpy(), host, "device entry without seeds")
    assert np.array_equal(d_prim.cpu().numpy(), hprim)
    # nray == 0 is a no-op
    assert tr.radiance_rays(np.zeros((0, 6), F), DEFAULT_LIGHT).shape == (0, 4)
    assert tr.radiance_rays_device(d_rays[:0], DEFAULT_LIGHT).shape == (0, 4)
    # a seed outside the domain: rejected by the host entry, nothing written
    import ctypes as C
    bad = seeds[:8].copy()
    bad[3] = (1 << 24) + 1
    keep = np.full((8, 4), 7.0, F)
    light = np.asarray(DEFAULT_LIGHT, F)
    rc = rt.lib().rt_radiance_rays(tr._h, rt._fp(np.ascontiguousarray(rays[:8])), bad.ctypes.data_as(C.POINTER(C.c_int32)), 8,
                                   rt._fp(light), rt._fp(keep), None)
    assert rc == abi.RT_E_INVALID and (keep == 7.0).all()
    with pytest.raises(rt.RtError):
        tr.radiance_rays(rays[:8], DEFAULT_LIGHT, seeds=bad)
    with pytest.raises(ValueError):
        tr.radiance_rays_device(d_rays.double(), DEFAULT_LIGHT)
    with pytest.raises(ValueError):
        tr.radiance_rays_device(d_rays.cpu(), DEFAULT_LIGHT)
    with pytest.raises(ValueError):
        tr.radiance_rays_device(d_rays, DEFAULT_LIGHT, seeds=d_seeds[:-1])
    tr.close()


def test_scene_update_and_frames(meshes):
    a = meshes["glass"]
    b = a.transformed(slice(26, len(a)), np.eye(3), (0.2, -0.05, -0.1))
    cfg = abi.make_config(width=128, height=96, shadow_samples=4)
    rays, seeds = random_rays(4000, seed=6)
    fresh = rt.RayTracer(cfg, b)
    want = fresh.radiance_rays(rays, DEFAULT_LIGHT, seeds=seeds, want_prim=True)
    fresh.close()
    plain = rt.RayTracer(cfg, a)
    view = (rt.rotation_matrix(0.1, 0.0), DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg))
    frame_alone = plain.render(*view)
    plain.close()
    tr = rt.RayTracer(cfg, a)
    before = tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=seeds, want_prim=True)
    frame = tr.render(*view)
    assert np.array_equal(frame, frame_alone)                           # a frame after a radiance call: the same bits
    ms = tr.last_kernel_ms()
    again = tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=seeds, want_prim=True)
    # the frame's timing events are untouched: the same two events, whose elapsed time the runtime recomputes from tick counts
    # at every query (seen to differ in the seventh digit between two queries; a radiance call takes a different time altogether)
    assert ms > 0 and tr.last_kernel_ms() == pytest.approx(ms, rel=1e-5)
    assert np.array_equal(tr.render(*view), frame)
    assert_same(again[0], before[0], "repeated call")
    tr.update_scene(b)
    got = tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=seeds, want_prim=True)
    assert_same(got[0], want[0], "after update_scene")
    assert np.array_equal(got[1], want[1]) and not np.array_equal(got[1], before[1])
    tr.close()


def test_shade_points_unchanged_by_the_shared_body(meshes, oracle):
    """rt_shade_points runs the body it now shares with the radiance call: results, counts and counters as before"""
    sc = meshes["2346"]
    S = 10
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=S), sc)
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.99, 0.99, (3000, 3)).astype(F)
    n = rng.normal(size=(3000, 3)).astype(F)
    n /= np.sqrt((n * n).sum(1, keepdims=True)).astype(F)
    seeds = rng.integers(0, (1 << 24) + 1, 3000).astype(np.int32)
    v, _, c = sc.packed()
    want, wcnt, term = su.direct_light(p, n, seeds, DEFAULT_LIGHT, S, tr.cfg.light_spread,
                                       lambda rays, r2: oracle.in_shadow(tr.cfg, v, c, rays, r2))
    got, cnt = tr.shade_points(p, n, DEFAULT_LIGHT, seeds=seeds, want_counts=True)
    assert np.array_equal(su.u32(got), su.u32(want)) and np.array_equal(cnt, wcnt)
    st = tr.shade_stats()
    assert st["points"] == 3000 and st["sample_rays"] == 3000 * S and st["skipped_points"] == 0
    assert st["waves"] == (3000 + 5) // 6 and st["tiles"] == (len(sc) + 63) // 64
    assert np.array_equal(su.u32(tr.shade_points(p, n, DEFAULT_LIGHT, seeds=seeds)), su.u32(want))
    st = tr.shade_stats()
    zero = int((term == 0).sum())
    assert zero > 0 and st["skipped_points"] == zero and st["sample_rays"] == (3000 - zero) * S
    tr.close()


# ---- d. the counters -----------------------------------------------------------------------------------------------------------
def test_counters(meshes):
    sc = meshes["20000"]                                                # (a mirror: no bounce ray of it leaves the culls' domain)
    S = 10
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=S, spheres=()), sc)
    rays, seeds = random_rays(4000, seed=8)
    rays = rays[64:]                                                    # in-domain rays only
    seeds = seeds[64:]
    got = tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=seeds)
    st = tr.radiance_stats()
    print("20000-triangle mirror mesh, random rays:", st)
    want = restate(tr, rays, seeds, (tr.trace_closest_hit, tr.trace_in_shadow))
    assert_same(got, want["rgba"], "20000-triangle mesh")
    assert st["rays"] == len(rays) and st["bounce_rays"] == int(want["bounces"].sum()) and st["shaded_points"] == int(want["diffuse"].sum())
    assert st["bounce_rays"] > 0 and 0 < st["sample_rays"] <= st["shaded_points"] * S
    assert st["closest_triangle_tests"] + st["shadow_triangle_tests"] < (st["rays"] + st["bounce_rays"] + st["sample_rays"]) * len(sc)
    assert want["unculled"] == 0                                        # every ray of the call is in the domain
    assert st["closest_tested_tiles"] > 0 and st["unculled_rays"] == 0
    tr.close()
    fresh = rt.RayTracer(abi.make_config(width=64, height=64), meshes["box"])
    assert not any(fresh.radiance_stats().values())                     # zeros before the first call
    fresh.close()


# ---- e. the panorama ---------------------------------------------------------------------------------------------------------
def test_panorama(meshes):
    import math
    import torch
    # the reference's box has no front wall (the camera looks in through it): the back wall once more at z = -1 closes it
    box = meshes["box"]
    z = box.aos[:, 0:3, 2]
    back = [int(i) for i in np.flatnonzero((z == z.max()).all(1))]
    closed = box + rt.Scene(box.transformed(back, np.eye(3), (0.0, 0.0, -2.0)).aos[back])
    assert len(back) == 2 and len(closed) == len(box) + 2
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=10), closed)
    W, H, cam, yaw = 256, 128, [0.1, -0.2, -0.3], 0.4
    img = tr.render_panorama(W, H, cam, DEFAULT_LIGHT, yaw=yaw)
    torch.cuda.synchronize()
    assert tuple(img.shape) == (H, W, 4) and img.dtype == torch.float32
    # the rays rebuilt from the documented formula, float32 on the device
    f32 = dict(dtype=torch.float32, device=img.device)
    t = lambda x: torch.tensor(x, **f32)
    phi = t(yaw) + (torch.arange(W, **f32) + 0.5) * t(2.0 * math.pi) / t(float(W)) - t(math.pi)
    theta = (torch.arange(H, **f32) + 0.5) * t(math.pi) / t(float(H)) - t(math.pi / 2.0)
    d = torch.stack([torch.sin(phi)[None, :] * torch.cos(theta)[:, None], torch.sin(theta)[:, None].expand(H, W),
                     torch.cos(phi)[None, :] * torch.cos(theta)[:, None]], -1).cpu().numpy()
    rays = aov_util.rays_of(cam, d)
    want = tr.radiance_rays(rays, DEFAULT_LIGHT, seeds=np.arange(W * H, dtype=np.int32))
    got = img.cpu().numpy()
    assert_same(got.reshape(-1, 4), want, "panorama")
    assert (got[..., 3] == 1.0).all()                                   # inside the closed box every direction hits
    assert len(np.unique(su.u32(got[..., :3]).reshape(-1, 3), axis=0)) > 100
    tr.close()
    # the open box from the same place: the rays through the missing wall see nothing, coverage 0 and colour 0
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=10), box)
    img = tr.render_panorama(W, H, cam, DEFAULT_LIGHT, yaw=yaw).cpu().numpy().reshape(-1, 4)
    tri, _ = tr.trace_closest_hit(rays)
    assert np.array_equal(img[:, 3], (tri != -1).astype(F)) and 0 < (tri == -1).sum() < W * H and not img[tri == -1].any()
    tr.close()
