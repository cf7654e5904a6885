"""-m gpu: rt_shade_points / rt_shade_points_device (rt_shade.hip) against tests/shade_util.py — direct_light restated in
numpy FP32, its masks from the CPU oracle's in_shadow and from the brute-force diagnostic rt_debug_trace_rays — and against
the frame itself: with the AOV planes of a view, albedo * (0.5f + L) must be rt_render's and the oracle's colour of every
diffuse primary hit, bit for bit (uint32 views)."""
import numpy as np
import pytest

import shade_util as su
from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, meshgen, runtime as rt

pytestmark = pytest.mark.gpu

F = np.float32
MESHES = {"166": (10, 8), "2346": (40, 30), "20000": (100, 101)}
VIEWS = {"default": (0.0, 0.0), "yawed": (0.3, 0.0)}


@pytest.fixture(scope="module")
def meshes(scene, tmp_path_factory):
    d = tmp_path_factory.mktemp("shade_meshes")
    out = {"box": scene}
    for name, (lon, lat) in MESHES.items():
        path = str(d / ("m%s.obj" % name))
        meshgen.write_sphere_obj(path, lon, lat)
        out[name] = scene + rt.Scene.load_obj(path)
    return out


def all_diffuse(sc):
    """Every triangle with a diffuse material (colour w > 0), its rgb kept"""
    for i in np.flatnonzero(sc.aos[:, 4, 3] <= 0):
        sc = sc.with_color([int(i)], tuple(sc.aos[i, 4, :3]) + (0.5,))
    return sc


def oracle_masks(oracle, cfg, sc):
    v, _, c = sc.packed()
    return lambda rays, r2: oracle.in_shadow(cfg, v, c, rays, r2)


def random_points(k, seed, light=DEFAULT_LIGHT):
    """Positions in the box, unit normals of which half face away from the light, seeds over the whole domain"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.99, 0.99, (k, 3)).astype(F)
    n = rng.normal(size=(k, 3)).astype(F)
    n /= np.sqrt((n * n).sum(1, keepdims=True)).astype(F)
    facing = ((np.asarray(light, F) - p) * n).sum(1) > 0
    flip = facing != (np.arange(k) % 2 == 0)
    n[flip] = -n[flip]
    seeds = rng.integers(0, (1 << 24) + 1, k).astype(np.int32)
    return p, n, seeds


def check_points(tr, oracle, sc, p, n, seeds, light=DEFAULT_LIGHT):
    """host entry == helper with the oracle's masks == helper with the brute-force diagnostic's; returns (light, counts, term)"""
    cfg = tr.cfg
    got, cnt = tr.shade_points(p, n, light, seeds=seeds, want_counts=True)
    for masks in (oracle_masks(oracle, cfg, sc), tr.trace_in_shadow):
        want, wcnt, term = su.direct_light(p, n, seeds, light, cfg.shadow_samples, cfg.light_spread, masks)
        bad = np.flatnonzero(~su.same_bits(got, want) | (cnt != wcnt))
        assert bad.size == 0, "%d of %d points differ, first %d: got %r / %d, want %r / %d" % (
            len(bad), len(got), bad[0], got[bad[0]], cnt[bad[0]], want[bad[0]], wcnt[bad[0]])
    assert np.array_equal(su.u32(tr.shade_points(p, n, light, seeds=seeds)), su.u32(got))      # without counts: the same light
    return got, cnt, term


# ---- a. the frame from public pieces: AOV + shade == rt_render == oracle, 1x1 AA ------------------------------------------
def frame_identity(oracle, sc, cfg, view, max_excluded=0.10):
    rot, focal = rt.rotation_matrix(*VIEWS[view]), focal_for(cfg)
    S, aa = cfg.shadow_samples, cfg.aa_x * cfg.aa_y
    tr = rt.RayTracer(cfg, sc)
    _, rgb = tr.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal, want_rgb=True)
    v, n, c = sc.packed()
    _, o_rgb = oracle.render(cfg, v, n, c, rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    o_rgb = o_rgb.reshape(cfg.height, cfg.width, 3)
    aov = tr.render_aov(rot, DEFAULT_CAM, focal, sample=None if aa > 1 else 0, planes=("prim", "position", "normal", "albedo"))
    shape = aov["prim"].shape                                    # [H, W] or [H, W, aa]
    ids = su.pixel_ids(range(cfg.height), cfg.width)
    ids = np.broadcast_to(ids.reshape(ids.shape + (1,) * (len(shape) - 2)), shape)
    light, cnt = tr.shade_points(aov["position"][..., :3], aov["normal"][..., :3], DEFAULT_LIGHT, seeds=ids.reshape(-1), want_counts=True)
    light, cnt = light.reshape(shape), cnt.reshape(shape)
    hit = aov["prim"] != -1
    diffuse = hit & (aov["albedo"][..., 3] > 0)
    col = np.where(diffuse[..., None], (aov["albedo"][..., :3] * (F(0.5) + light)[..., None]).astype(F), F(0.0)).astype(F)
    if aa > 1:                                                   # the pixel: float32 sum in sample order, / aa
        ok = (diffuse | ~hit).all(-1)
        acc = np.zeros(shape[:2] + (3,), F)
        for a in range(aa):
            acc = (acc + col[:, :, a]).astype(F)
        col = (acc / F(aa)).astype(F)
        lit = ok & diffuse.any(-1)
        partial = ((cnt > 0) & (cnt < S) & diffuse & ok[..., None]).any()
    else:
        ok = diffuse | ~hit
        lit = diffuse
        partial = ((cnt > 0) & (cnt < S) & diffuse).any() if S > 1 else (cnt[diffuse].min() == 0 and cnt[diffuse].max() == 1)
    excluded = 1.0 - ok.mean()
    print("%s S=%d aa=%d: %d compared pixels (%d lit), %.1f %% excluded" % (view, S, aa, ok.sum(), lit.sum(), 100 * excluded))
    assert excluded <= max_excluded and lit.sum() > 0
    assert np.array_equal(su.u32(col[ok]), su.u32(rgb[..., :3][ok]))
    assert np.array_equal(su.u32(col[ok]), su.u32(o_rgb[ok]))
    # a case proves little unless some point is partially shadowed (S = 1 has no such point: both outcomes must occur)
    assert partial
    tr.close()


@pytest.mark.parametrize("view", ["default", "yawed"])
@pytest.mark.parametrize("samples", [1, 10, 64, 100])
@pytest.mark.parametrize("name", ["box", "2346"])
def test_frame_identity(name, samples, view, meshes, oracle):
    frame_identity(oracle, meshes[name], abi.make_config(width=96, height=96, aa_x=1, aa_y=1, shadow_samples=samples), view)


@pytest.mark.parametrize("name", ["box", "2346"])
def test_frame_identity_all_diffuse(name, meshes, oracle):
    cfg = abi.make_config(width=96, height=96, aa_x=1, aa_y=1, shadow_samples=10, spheres=())
    frame_identity(oracle, all_diffuse(meshes[name]), cfg, "default", max_excluded=0.0)


# ---- b. 2x2 AA from RT_AOV_ALL_SAMPLES -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "2346"])
def test_frame_identity_2x2(name, meshes, oracle):
    # (a pixel is excluded when ANY of its four samples is mirror or glass; the share is printed and held to the same 10 %)
    frame_identity(oracle, meshes[name], abi.make_config(width=64, height=64, aa_x=2, aa_y=2, shadow_samples=10), "default")


# ---- c. general points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", [("box", 0), ("166", 0), ("2346", 0), ("20000", 0), ("2346", abi.RT_FLAG_GENERIC_KERNEL),
                                        ("box", abi.RT_FLAG_GENERIC_KERNEL)])
@pytest.mark.parametrize("samples", [10, 100])
def test_general_points(name, flags, samples, meshes, oracle):
    sc = meshes[name]
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=samples, flags=flags), sc)
    p, n, seeds = random_points(1500 if samples == 10 else 300, seed=len(sc) + samples)
    _, cnt, term = check_points(tr, oracle, sc, p, n, seeds)
    assert ((cnt > 0) & (cnt < samples)).any() and (term == 0).sum() > len(p) // 4
    assert (tr.shade_stats()["tiles"] == 0) == (flags != 0 or len(sc) <= 64)
    tr.close()


# ---- d. the device entry ----------------------------------------------------------------------------------------------------
def test_device_entry(meshes):
    import torch
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=10), meshes["2346"])
    p, n, _ = random_points(5000, seed=5)
    host, hcnt = tr.shade_points(p, n, DEFAULT_LIGHT, want_counts=True)                  # seeds = None
    seeds = (np.arange(len(p)) & 0xFFFFFF).astype(np.int32)
    assert np.array_equal(su.u32(tr.shade_points(p, n, DEFAULT_LIGHT, seeds=seeds)), su.u32(host))
    p6 = torch.from_numpy(np.ascontiguousarray(np.concatenate([p, n], 1))).cuda()
    d_seeds = torch.from_numpy(seeds).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    light, cnt = tr.shade_points_device(p6, DEFAULT_LIGHT, seeds=d_seeds, want_counts=True, stream=s)
    only = tr.shade_points_device(p6, DEFAULT_LIGHT, stream=s)                           # no seeds, no counts
    s.synchronize()
    assert np.array_equal(su.u32(light.cpu().numpy()), su.u32(host)) and np.array_equal(cnt.cpu().numpy(), hcnt)
    assert np.array_equal(su.u32(only.cpu().numpy()), su.u32(host))
    with pytest.raises(ValueError):
        tr.shade_points_device(p6.double(), DEFAULT_LIGHT)
    with pytest.raises(ValueError):
        tr.shade_points_device(p6.cpu(), DEFAULT_LIGHT)
    with pytest.raises(ValueError):
        tr.shade_points_device(p6, DEFAULT_LIGHT, seeds=d_seeds[:-1])
    with pytest.raises(rt.RtError):
        tr.shade_points(p, n, DEFAULT_LIGHT, seeds=np.full(len(p), -1, np.int32))
    # the per-pixel light plane composed on the device
    cfg = tr.cfg
    rot, focal = rt.rotation_matrix(0.0, 0.0), focal_for(cfg)
    plane = tr.render_direct_light(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    torch.cuda.synchronize()
    aov = tr.render_aov(rot, DEFAULT_CAM, focal, planes=("prim", "position", "normal"))
    want = tr.shade_points(aov["position"][..., :3], aov["normal"][..., :3], DEFAULT_LIGHT, seeds=su.pixel_ids(range(64), 64).reshape(-1))
    want = np.where(aov["prim"] != -1, want.reshape(64, 64), F(0.0))
    assert np.array_equal(su.u32(plane.cpu().numpy()), su.u32(want))
    tr.close()


def test_direct_light_plane_of_a_band(meshes):
    """render_direct_light of a context that owns every other band of 16 rows: the seeds are the GLOBAL pixel ids"""
    import torch
    import aov_util
    cfg = abi.make_config(width=64, height=64, shadow_samples=10, band_rows=16, band_index=1, band_count=2)
    tr = rt.RayTracer(cfg, meshes["2346"])
    rot, focal = rt.rotation_matrix(0.0, 0.0), focal_for(cfg)
    plane = tr.render_direct_light(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    torch.cuda.synchronize()
    rows = aov_util.owned_rows(cfg)
    assert plane.shape == (len(rows), 64) and rows[0] == 16
    aov = tr.render_aov(rot, DEFAULT_CAM, focal, planes=("prim", "position", "normal"))
    want = tr.shade_points(aov["position"][..., :3], aov["normal"][..., :3], DEFAULT_LIGHT, seeds=su.pixel_ids(rows, 64).reshape(-1))
    want = np.where(aov["prim"] != -1, want.reshape(len(rows), 64), F(0.0))
    assert np.array_equal(su.u32(plane.cpu().numpy()), su.u32(want)) and (want > 0).any()
    with pytest.raises(ValueError):
        tr.render_direct_light(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal, sample=None)
    with pytest.raises(ValueError):
        tr.render_direct_light(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal, sample=abi.RT_AOV_ALL_SAMPLES)
    tr.close()
    # the whole frame of the same view holds the band's rows
    full = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=10), meshes["2346"])
    whole = full.render_direct_light(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    torch.cuda.synchronize()
    assert np.array_equal(su.u32(whole.cpu().numpy()[rows]), su.u32(want))
    full.close()


# ---- e. scene updates, and shade calls between frames ------------------------------------------------------------------------
def test_scene_update_and_frames(meshes):
    a = meshes["2346"]
    b = a.transformed(slice(26, len(a)), np.eye(3), (0.2, -0.05, -0.1))
    cfg = abi.make_config(width=128, height=96, shadow_samples=4)
    p, n, seeds = random_points(4000, seed=6)
    fresh = rt.RayTracer(cfg, b)
    want = fresh.shade_points(p, n, DEFAULT_LIGHT, seeds=seeds, want_counts=True)
    fresh.close()
    tr = rt.RayTracer(cfg, a)
    before = tr.shade_points(p, n, DEFAULT_LIGHT, seeds=seeds, want_counts=True)
    view = (rt.rotation_matrix(0.1, 0.0), DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg))
    frame = tr.render(*view)
    ms = tr.last_kernel_ms()
    again = tr.shade_points(p, n, DEFAULT_LIGHT, seeds=seeds, want_counts=True)
    assert tr.last_kernel_ms() == ms                                    # the frame's timing events are untouched
    assert np.array_equal(tr.render(*view), frame)
    assert np.array_equal(su.u32(again[0]), su.u32(before[0])) and np.array_equal(again[1], before[1])
    tr.update_scene(b)
    got = tr.shade_points(p, n, DEFAULT_LIGHT, seeds=seeds, want_counts=True)
    assert np.array_equal(su.u32(got[0]), su.u32(want[0])) and np.array_equal(got[1], want[1])
    assert not np.array_equal(got[1], before[1])
    tr.close()


# ---- f. degenerate inputs: ordinary arithmetic, defined results ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "2346"])
def test_degenerate_inputs(name, meshes, oracle):
    sc = meshes[name]
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=10), sc)
    p, n, seeds = random_points(256, seed=7)
    p[0:64:4] = np.asarray(DEFAULT_LIGHT, F)                            # P at the light: radius_sq = 0
    p[64:128:4, 1] = np.nan                                             # NaN position
    p[128:192:4] *= F(2.0 ** 17)                                        # beyond 2^16: outside the certificates' domain
    n[200:208] = F(np.inf)                                              # the term's dot product overflows
    got, _, _ = check_points(tr, oracle, sc, p, n, seeds)
    assert np.isnan(got[0]) and np.isnan(got[64])
    tr.close()


# ---- g. the counters --------------------------------------------------------------------------------------------------------
def test_counters(meshes):
    sc = meshes["20000"]
    S = 10
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=S), sc)
    # 1000 clusters of 6 neighbouring points: a wave's 6 points are neighbours, as they are for points taken from a G-buffer
    p, n, seeds = random_points(6000, seed=8)
    p = (np.repeat(p[::6], 6, axis=0) + F(1e-3) * p).astype(F)
    tr.shade_points(p, n, DEFAULT_LIGHT, seeds=seeds, want_counts=True)
    st = tr.shade_stats()
    print("20000-triangle mesh, random points, with counts:", st)
    assert st["points"] == len(p) and st["sample_rays"] == len(p) * S and st["skipped_points"] == 0
    assert st["waves"] == (len(p) + 5) // 6 and st["tiles"] == (len(sc) + 63) // 64
    assert st["triangle_tests"] < len(p) * S * len(sc)
    assert st["tested_tiles"] <= st["bundle_tiles"] < st["waves"] * st["tiles"]
    tr.shade_points(p, n, DEFAULT_LIGHT, seeds=seeds)
    st = tr.shade_stats()
    print("without counts:", st)
    _, _, _, num, den = su.setup(p, n, DEFAULT_LIGHT)
    zero = int(((num / den) == 0).sum())
    assert zero > len(p) // 4
    assert st["points"] == len(p) and st["skipped_points"] == zero and st["sample_rays"] == (len(p) - zero) * S
    tr.close()
    # more than 64 samples: a point takes two passes of one wave
    tr = rt.RayTracer(abi.make_config(width=64, height=64, shadow_samples=100), sc)
    tr.shade_points(p[:500], n[:500], DEFAULT_LIGHT, seeds=seeds[:500], want_counts=True)
    st = tr.shade_stats()
    assert st["points"] == 500 and st["sample_rays"] == 500 * 100 and st["waves"] == 1000
    tr.close()
