"""-m gpu: the AOV pass (rt_render_aov / rt_render_aov_device, rt_aov.hip).  Everything is compared as uint32 bit patterns:
against the CPU oracle's closest hit of the frame's own primary rays (restated in numpy FP32, tests/aov_util.py), against
the query path at full size, against the frame itself, over subsets of planes, scene updates and stream orderings, through
the culling counters and through the host program."""
import os
import subprocess

import numpy as np
import pytest

import aov_util
from aov_util import assert_planes_equal, u32
from conftest import DEFAULT_CAM, DEFAULT_LIGHT, ROOT, focal_for
from test_host_surface import read_bmp
from uob_raytracer_amd import abi, meshgen, runtime as rt

pytestmark = pytest.mark.gpu

ALL_PLANES = ("prim", "depth", "position", "normal", "albedo", "direction")
POSES = {"default": (0.0, 0.0, DEFAULT_CAM), "turned": (0.4, -0.15, [0.3, 0.1, -2.9])}
MESHES = {"166": (10, 8), "2346": (40, 30), "20000": (100, 101)}


@pytest.fixture(scope="module")
def meshes(scene, tmp_path_factory):
    d = tmp_path_factory.mktemp("aov_meshes")
    out = {}
    for name, (lon, lat) in MESHES.items():
        path = str(d / ("m%s.obj" % name))
        meshgen.write_sphere_obj(path, lon, lat)
        out[name] = scene + rt.Scene.load_obj(path)
    return out


def oracle_planes(oracle, cfg, sc, rot, cam, focal):
    """The six planes of every sample, [rows, W, aa(, 4)], from the oracle's closest hit of the helper's rays."""
    v, n, c = sc.packed()
    dirs = aov_util.primary_directions(cfg, rot, focal)
    tri, out10 = oracle.closest_hit(cfg, v, n, c, aov_util.rays_of(cam, dirs))
    return aov_util.expected_planes(cam, dirs, tri, out10)


def check_against_oracle(oracle, cfg, sc, pose="default", min_mesh=0):
    yaw, pitch, cam = POSES[pose]
    rot, focal = rt.rotation_matrix(yaw, pitch), focal_for(cfg)
    want = oracle_planes(oracle, cfg, sc, rot, cam, focal)
    aa = cfg.aa_x * cfg.aa_y
    tr = rt.RayTracer(cfg, sc)
    for sample in (0, aa - 1, None):
        got = tr.render_aov(rot, cam, focal, sample=sample)
        assert set(got) == set(ALL_PLANES)
        assert_planes_equal(got, want if sample is None else {k: w[:, :, sample] for k, w in want.items()})
        assert tr.aov_stats()["samples"] == tr.rows * cfg.width * (aa if sample is None else 1)
    tr.close()
    prim = want["prim"]
    assert (prim == -1).any() and (prim >= 0).any()              # hits and misses are in view
    assert np.isinf(want["depth"][prim == -1]).all() and np.isfinite(want["depth"][prim != -1]).all()
    assert (prim >= 26).sum() >= min_mesh
    return want


# ---- 1. against the CPU oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("aa", [(1, 1), (2, 2), (4, 2)])
def test_box_with_spheres_against_oracle(aa, pose, scene, oracle):
    want = check_against_oracle(oracle, abi.make_config(width=64, height=64, aa_x=aa[0], aa_y=aa[1]), scene, pose)
    assert (want["prim"] == -2).any()                            # a sphere is in view


def test_ragged_frame_against_oracle(scene, oracle):
    check_against_oracle(oracle, abi.make_config(width=100, height=37, aa_x=2, aa_y=2), scene)


@pytest.mark.parametrize("index", [0, 1, 2])
def test_banded_context_against_oracle(index, scene, oracle):
    cfg = abi.make_config(width=72, height=100, aa_x=2, aa_y=1, band_rows=16, band_index=index, band_count=3)
    check_against_oracle(oracle, cfg, scene, "turned")


@pytest.mark.parametrize("name", list(MESHES))
def test_meshes_against_oracle(name, meshes, oracle):
    check_against_oracle(oracle, abi.make_config(width=128, height=128, aa_x=2, aa_y=1), meshes[name], min_mesh=500)


@pytest.mark.parametrize("flags", [abi.RT_FLAG_GENERIC_KERNEL, abi.RT_FLAG_NO_TILE_BINS])
def test_mesh_context_variants_against_oracle(flags, meshes, oracle):
    cfg = abi.make_config(width=128, height=128, aa_x=2, aa_y=1, flags=flags)
    check_against_oracle(oracle, cfg, meshes["2346"], min_mesh=500)


# ---- 2. against the query path at full size -------------------------------------------------------------------------------
def test_full_size_equals_the_query_path(scene, tmp_path):
    import torch
    path = str(tmp_path / "mesh_100k.obj")
    assert meshgen.write_sphere_obj(path, 250, 201) == 100000
    both = scene + rt.Scene.load_obj(path)
    cfg = abi.make_config(width=2048, height=2048, aa_x=1, aa_y=1, shadow_samples=1, spheres=())
    tr = rt.RayTracer(cfg, both)
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"prim": torch.empty((2048, 2048), dtype=torch.int32, device=dev)}
    for name in ("position", "normal", "albedo", "direction"):
        out[name] = torch.empty((2048, 2048, 4), dtype=torch.float32, device=dev)
    rot = rt.rotation_matrix(0.0, 0.0)
    tr.render_aov_device(rot, DEFAULT_CAM, focal_for(cfg), sample=0, out=out)
    k = 2048 * 2048
    rays = torch.empty((k, 6), dtype=torch.float32, device=dev)
    rays[:, 0:3] = torch.tensor(DEFAULT_CAM, dtype=torch.float32, device=dev)
    rays[:, 3:6] = out["direction"].reshape(k, 4)[:, 0:3]
    tri, out10 = tr.query_device(abi.RT_TRACE_CLOSEST_HIT, rays)
    torch.cuda.synchronize()
    assert torch.equal(out["prim"].reshape(k), tri)
    assert int((tri >= 26).sum()) > k // 50 and int((tri == -1).sum()) > 0
    bits = out10.view(torch.int32)
    for name, lo in (("position", 0), ("normal", 3), ("albedo", 6)):
        n = 4 if name == "albedo" else 3
        assert torch.equal(out[name].reshape(k, 4)[:, 0:n].contiguous().view(torch.int32), bits[:, lo:lo + n].contiguous()), name
    hit = tri != -1
    assert torch.equal(out["position"].reshape(k, 4)[:, 3], hit.to(torch.float32))
    assert not bool(out["normal"].reshape(k, 4)[:, 3].any())
    st = tr.aov_stats()
    assert st["samples"] == k and st["tiles"] == 1563 and st["mask_tiles"] < st["waves"] * st["tiles"]
    tr.close()


# ---- 3. consistency with the frame ------------------------------------------------------------------------------------------
def test_misses_are_the_frames_black_pixels(meshes):
    aos = meshes["166"].aos.copy()
    aos[:, 4, 3] = np.where(aos[:, 4, 3] > 0, aos[:, 4, 3], 1.0)             # diffuse only
    sc = rt.Scene(aos)
    cfg = abi.make_config(width=128, height=128, aa_x=1, aa_y=1, spheres=())
    tr = rt.RayTracer(cfg, sc)
    rot = rt.rotation_matrix(0.0, 0.0)
    _, rgb = tr.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg), want_rgb=True)
    prim = tr.render_aov(rot, DEFAULT_CAM, focal_for(cfg), planes=("prim",))["prim"]
    tr.close()
    black = (rgb[..., :3] == 0).all(-1)
    assert np.array_equal(prim == -1, black) and 0 < black.sum() < black.size


def test_specular_samples_are_the_frames_bounce_rays(scene):
    sc = scene.with_color([8, 9], (1.0, 1.0, 1.0, 0.0))                      # mirror wall + the reference's two spheres
    cfg = abi.make_config(width=64, height=64, aa_x=2, aa_y=2, max_bounces=1)
    tr = rt.RayTracer(cfg, sc)
    rot = rt.rotation_matrix(0.0, 0.0)
    got = tr.render_aov(rot, DEFAULT_CAM, focal_for(cfg), sample=None, planes=("prim", "albedo"))
    work = tr.count_work(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg))
    tr.close()
    specular = (got["prim"] != -1) & (got["albedo"][..., 3] <= 0)
    assert specular.sum() == work["bounce_rays"] > 0


# ---- 4. selection of planes -----------------------------------------------------------------------------------------------
def test_any_subset_of_planes_gives_the_same_bits(meshes):
    import torch
    cfg = abi.make_config(width=96, height=64, aa_x=2, aa_y=1)
    tr = rt.RayTracer(cfg, meshes["2346"])
    yaw, pitch, cam = POSES["turned"]
    rot, focal = rt.rotation_matrix(yaw, pitch), focal_for(cfg)
    dev = torch.device("cuda", torch.cuda.current_device())
    pad, canary = 512, 0x5A5A5A5A
    for sample in (1, None):
        full = tr.render_aov(rot, cam, focal, sample=sample)
        subsets = [(p,) for p in ALL_PLANES] + [("prim", "depth"), ("normal", "direction"), ("depth", "albedo", "position")]
        for names in subsets:
            flat, out = {}, {}
            for name in names:
                shape = full[name].shape
                count = int(np.prod(shape))
                flat[name] = torch.full((count + 2 * pad,), canary, dtype=torch.int32, device=dev)
                body = flat[name][pad:pad + count]
                out[name] = (body if name == "prim" else body.view(torch.float32)).view(shape)
            tr.render_aov_device(rot, cam, focal, sample=sample, out=out)
            torch.cuda.synchronize()
            for name in names:
                host = flat[name].cpu().numpy().view(np.uint32)
                assert (host[:pad] == canary).all() and (host[-pad:] == canary).all(), (names, name)
                assert np.array_equal(host[pad:-pad], u32(full[name]).ravel()), (names, name)
            host_got = tr.render_aov(rot, cam, focal, sample=sample, planes=names)
            assert set(host_got) == set(names)
            assert_planes_equal(host_got, full, names)
    tr.close()


# ---- 5. scene updates and ordering ------------------------------------------------------------------------------------------
def test_scene_update_then_pass_equals_a_fresh_context(meshes):
    sc = meshes["2346"]
    moved = sc.transformed(slice(26, None), np.eye(3), (0.15, -0.1, 0.05))
    cfg = abi.make_config(width=128, height=128, aa_x=1, aa_y=1)
    rot, focal = rt.rotation_matrix(0.0, 0.0), focal_for(cfg)
    tr = rt.RayTracer(cfg, sc)
    before = tr.render_aov(rot, DEFAULT_CAM, focal)
    tr.update_scene(moved)
    after = tr.render_aov(rot, DEFAULT_CAM, focal)
    tr.close()
    fresh = rt.RayTracer(cfg, moved)
    want = fresh.render_aov(rot, DEFAULT_CAM, focal)
    fresh.close()
    assert_planes_equal(after, want)
    assert not np.array_equal(before["prim"], after["prim"])


def test_a_pass_leaves_the_frames_and_their_scheduling_alone(meshes):
    cfg = abi.make_config(width=256, height=256, aa_x=1, aa_y=1, shadow_samples=4)
    rot, focal = rt.rotation_matrix(0.0, 0.0), focal_for(cfg)
    plain = rt.RayTracer(cfg, meshes["2346"])
    a1 = plain.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    a2 = plain.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    plain.close()
    tr = rt.RayTracer(cfg, meshes["2346"])
    b1 = tr.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    ms = tr.last_kernel_ms()
    costs = tr.block_costs()
    tr.render_aov(rot, DEFAULT_CAM, focal)
    tr.render_aov(rt.rotation_matrix(0.3, 0.1), [0.2, 0.0, -3.0], focal, sample=None)
    assert np.array_equal(tr.block_costs(), costs)               # the scheduling state is the frame's, untouched
    assert tr.last_kernel_ms() == ms
    b2 = tr.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    tr.close()
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2) and np.array_equal(a1, a2)


def test_pass_and_frame_on_two_streams(meshes):
    import torch
    cfg = abi.make_config(width=256, height=256, aa_x=1, aa_y=1, shadow_samples=4)
    rot, focal = rt.rotation_matrix(0.0, 0.0), focal_for(cfg)
    tr = rt.RayTracer(cfg, meshes["2346"])
    want_aov = tr.render_aov(rot, DEFAULT_CAM, focal)
    want_argb = tr.render(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal)
    dev = torch.device("cuda", torch.cuda.current_device())
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for _ in range(3):
        out = {"prim": torch.zeros((256, 256), dtype=torch.int32, device=dev),
               "depth": torch.zeros((256, 256), dtype=torch.float32, device=dev),
               "normal": torch.zeros((256, 256, 4), dtype=torch.float32, device=dev)}
        argb = torch.zeros((256, 256), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        tr.render_aov_device(rot, DEFAULT_CAM, focal, sample=0, out=out, stream=s1)
        tr.render_device(rot, DEFAULT_CAM, DEFAULT_LIGHT, focal, argb.data_ptr(), stream=s2.cuda_stream)
        tr.render_aov_device(rot, DEFAULT_CAM, focal, sample=0, out=out, stream=s1)
        torch.cuda.synchronize()
        assert np.array_equal(argb.cpu().numpy().view(np.uint32), want_argb)
        assert_planes_equal({k: t.cpu().numpy() for k, t in out.items()}, want_aov, list(out))
    tr.close()


# ---- 6. culling did something -----------------------------------------------------------------------------------------------
def test_tile_bins_spare_triangle_tests(meshes):
    kw = dict(width=128, height=128, aa_x=2, aa_y=1)
    rot = rt.rotation_matrix(0.0, 0.0)
    stats = {}
    for flags in (0, abi.RT_FLAG_NO_TILE_BINS):
        cfg = abi.make_config(flags=flags, **kw)
        tr = rt.RayTracer(cfg, meshes["20000"])
        assert tr.aov_stats() == dict.fromkeys(rt.AOV_STATS_KEYS, 0)          # zeros before the first pass
        tr.render_aov(rot, DEFAULT_CAM, focal_for(cfg), sample=None, planes=("prim",))
        stats[flags] = tr.aov_stats()
        tr.close()
        print(flags, stats[flags])
    bins, plain = stats[0], stats[abi.RT_FLAG_NO_TILE_BINS]
    for st in (bins, plain):
        assert st["samples"] == 128 * 128 * 2 and st["waves"] == 128 * 128 * 2 // 64 and st["tiles"] == (20026 + 63) // 64
    assert plain["mask_tiles"] == plain["waves"] * plain["tiles"]
    assert bins["mask_tiles"] < plain["mask_tiles"]
    assert bins["triangle_tests"] < plain["triangle_tests"]


# ---- 7. the host program ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--devices", "0,0,0"]])
def test_host_program_writes_the_aov_images(extra, tmp_path, scene):
    exe = os.path.join(ROOT, "uob_raytracer_amd", "uob_raytracer")
    plain, shot, prefix = str(tmp_path / "plain.bmp"), str(tmp_path / "shot.bmp"), str(tmp_path / "view")
    base = [exe, "--size", "128", "--frames", "2", "--keys", "left i"] + extra
    subprocess.run(base + ["--out", plain], check=True, capture_output=True)
    subprocess.run(base + ["--out", shot, "--aov", prefix], check=True, capture_output=True)
    assert open(plain, "rb").read() == open(shot, "rb").read()
    assert sorted(os.listdir(str(tmp_path))) == ["plain.bmp", "shot.bmp", "view_depth.bmp", "view_id.bmp", "view_normal.bmp"]
    images = {k: read_bmp(prefix + "_%s.bmp" % k) for k in ("depth", "normal", "id")}
    for img in images.values():
        assert img.shape == (128, 128) and (img >> 24 == 255).all()
    # the same view through the binding: yaw 0.1 after "left", camera z -3.1 after "i" (float32 / double as the C++ does)
    cfg = rt.default_config()
    cfg.width = cfg.height = cfg.band_rows = 128
    tr = rt.RayTracer(cfg, scene)
    yaw = np.float32(np.float64(np.float32(0.0)) + 0.1)
    cam = [0.0, 0.0, float(np.float32(np.float64(np.float32(-3.2)) + 0.1))]
    got = tr.render_aov(rt.rotation_matrix(float(yaw), 0.0), cam, 1100.0 * 128 / 1024 * cfg.aa_x, planes=("prim", "depth"))
    tr.close()
    ids = np.unique(got["prim"])
    assert 3 <= len(ids) <= 30
    assert len(np.unique(images["id"])) == len(ids)
    for i in ids:                                                # one colour per id, the same wherever the id is seen
        assert len(np.unique(images["id"][got["prim"] == i])) == 1
    grey = images["depth"] & 0xFF
    assert (grey[got["prim"] == -1] == 0).all() and grey.max() == 255
    assert grey.ravel()[np.argmin(got["depth"])] == 255
