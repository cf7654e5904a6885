"""-m gpu: closest-hit ties.  The reference replaces a hit only for a strictly smaller t, visiting the triangles in their
original order (kernels.cl:120, :194): of several hits at bit-equal t the lowest ORIGINAL index wins, and a sphere must be
strictly nearer than the triangle hit.  Every kernel that walks triangles in an order of its own restates that rule: closer()
of rt_tiles.h, primary_tile / bounce_tile / merge_hits of rt_kernel_mesh.hip, the tiled walk behind the ray, AOV, shade and
radiance calls, the mask-ordered loops of rt_trace.h, the tie order of the host and device tile sorts.

The scenes are those of tests/ties_util.py — duplicated faces (same, reversed and rotated winding), decals lying exactly in a
wall, double-sided meshes, two objects that coincide after a refit — in which hundreds to thousands of rays per frame meet two
triangles at bit-equal t (tests/test_ties_util_cpu.py proves that of every scene, at these frame sizes and views, with the
oracle alone; tests/test_oracle_vs_ref.py pins the oracle's own tie rule to the reference kernel).  Every assertion is bit
equality against the CPU oracle; equality between device paths comes second."""
import numpy as np
import pytest

import aov_util
import radiance_util as ru
import shade_util as su
import ties_util as tu
import wave_masks_util as wm
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

F = np.float32
_REF = {}                                    # oracle frames: computed once, shared, never changed


@pytest.fixture(scope="module")
def meshes(tmp_path_factory):
    d = tmp_path_factory.mktemp("ties_meshes")
    return {size: tu.load_mesh(size[0], size[1], d) for size in tu.MESH_SIZES}


def pose(kw, vname):
    """-> (rot, cam, light, focal) of a ties_util view on a frame of config keywords kw"""
    yaw, pitch, cam, light, lens = tu.view(vname)
    return rt.rotation_matrix(yaw, pitch), cam, light, tu.focal_for(abi.make_config(**kw), lens)


def oracle_frame(oracle, key, kw, sc, vname):
    k = (key, tuple(sorted((a, repr(b)) for a, b in kw.items())), vname)
    if k not in _REF:
        v, n, c = sc.packed()
        _REF[k] = oracle.render(abi.make_config(**kw), v, n, c, *pose(kw, vname), nthreads=8)
    return _REF[k]


def same(got, want, what):
    a = got[0]
    wa = np.asarray(want[0]).reshape(a.shape)
    bad = np.argwhere(a != wa)
    assert bad.size == 0, "%s: %d pixels differ, first at %s" % (what, len(bad), bad[0])
    g = np.asarray(got[1], F).reshape(a.size, -1)[:, :3]
    w = np.asarray(want[1], F).reshape(a.size, -1)[:, :3]
    assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), what + ": float plane differs"


def frames_of(tr, kw, views):
    return [tr.render(*pose(kw, v), want_rgb=True) for v in views]


def render(kw, sc, views, flags=0, knobs=None):
    tr = wm.context(kw, knobs or {}, sc, flags)
    out = frames_of(tr, kw, views)
    tr.close()
    return out


# ---- 1. the wave kernel, n <= 64 ------------------------------------------------------------------------------------------

AAS = ((1, 1), (2, 2), (4, 2))
SAMPLES = (1, 16, 64)


def _box_cases():
    """(kind, order, material, aa, samples): every scene, the samplings spread over them (all nine pairs occur)"""
    out = []
    for kind in tu.BOX_KINDS:
        for order in tu.ORDERS:
            for material in (("diffuse", "mirror", "glass") if kind in ("same", "reversed", "decal_wall") else ("diffuse",)):
                i = len(out)
                out.append((kind, order, material, AAS[i % 3], SAMPLES[(i // 3) % 3]))
    return out


BOX_CASES = _box_cases()
assert {(c[3], c[4]) for c in BOX_CASES} == {(a, s) for a in AAS for s in SAMPLES}


@pytest.mark.parametrize("case", BOX_CASES, ids=lambda c: "%s-%s-%s-%dx%d-%d" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4]))
def test_box_frames(case, scene, oracle):
    """shipped == RT_FLAG_NO_CULL == RT_FLAG_GENERIC_KERNEL == oracle, ARGB and float planes, two views"""
    kind, order, material, (ax, ay), samples = case
    sc, _ = tu.box_scene(scene, kind, order, material)
    kw = dict(width=160, height=96, aa_x=ax, aa_y=ay, shadow_samples=samples)
    views = tu.views_of(kind)
    got = {"shipped": render(kw, sc, views), "RT_FLAG_NO_CULL": render(kw, sc, views, abi.RT_FLAG_NO_CULL),
           "RT_FLAG_GENERIC_KERNEL": render(kw, sc, views, abi.RT_FLAG_GENERIC_KERNEL)}
    for vi, vname in enumerate(views):
        want = oracle_frame(oracle, ("box",) + case[:3], kw, sc, vname)
        for what, frames in got.items():
            same(frames[vi], want, "%s, %s, %s against the oracle" % (case, vname, what))


def test_box_more_than_64_aa_samples(scene, oracle):
    """9x9 AA (two tasks per pixel) on the doubled floor, wall and block face, the copies first"""
    sc, _ = tu.box_scene(scene, "reversed", "first")
    kw = dict(width=96, height=64, aa_x=9, aa_y=9, shadow_samples=16)
    for flags in (0, abi.RT_FLAG_NO_CULL, abi.RT_FLAG_GENERIC_KERNEL):
        got = render(kw, sc, ("default",), flags)
        same(got[0], oracle_frame(oracle, "box9x9", kw, sc, "default"), "9x9 AA, flags %d" % flags)


# strips of 128x8 at the headline sampling under UOB_RT_JOB_TASKS=8, through a lens 8x the default: a job's 64-pixel tile lies
# on one duplicated face.  (yaw, pitch): the back wall right of and above the tall block; the floor in front of the tall block.
STRIP_VIEWS = {"wall": (0.05, 0.1), "floor": (-0.19, -0.36)}
STRIPS = [("reversed", "after", "wall"), ("reversed", "first", "floor"), ("same", "first", "wall"), ("same", "after", "floor"),
          ("rotated", "first", "wall"), ("decal_wall", "first", "wall"), ("decal_wall", "after", "wall")]
STRIP = dict(width=128, height=8, aa_x=4, aa_y=2, shadow_samples=64)
STRIP_FOCAL = 1100.0 * 128 / 1024.0 * 4 * 8.0


def strip_on_pair(oracle, sc, pairs, vname):
    """(pixels of the strip whose first AA sample's closest hit is a triangle of a pair, pixels) by the oracle"""
    cfg = abi.make_config(**STRIP)
    rot = rt.rotation_matrix(*STRIP_VIEWS[vname])
    dirs = aov_util.primary_directions(cfg, rot, STRIP_FOCAL)[:, :, 0]
    v, n, c = sc.packed()
    tri, _ = oracle.closest_hit(cfg, v, n, c, aov_util.rays_of(wm.DEFAULT_CAM, dirs))
    partner, _ = tu.pair_tables(len(sc), pairs)
    return int(((tri >= 0) & (partner[np.where(tri >= 0, tri, 0)] >= 0)).sum()), tri.size


@pytest.mark.parametrize("kind,order,vname", STRIPS)
def test_strip_seeded(kind, order, vname, scene, oracle, capsys):
    """seeded (1, 4 and 16 rows per tile) == UOB_RT_NO_SEED=1 == unculled == generic == oracle; a seed's record names what
    its tile shows (check_table of test_gpu_tile_seed.py and check_wide_table of test_gpu_tile_seed_wide.py: Kp holds the AOV
    pass's ids, which are the lower index of a pair, and h is the id at the tile's centre)"""
    from test_gpu_tile_seed import check_table
    from test_gpu_tile_seed_wide import DEFAULT, check_wide_table, wide_counters
    sc, pairs = tu.box_scene(scene, kind, order)
    on, of = strip_on_pair(oracle, sc, pairs, vname)
    assert 2 * on >= of, "the strip shows a pair on %d of %d pixels" % (on, of)
    rot, cam, light = rt.rotation_matrix(*STRIP_VIEWS[vname]), wm.DEFAULT_CAM, wm.DEFAULT_LIGHT
    v, n, c = sc.packed()
    want = oracle.render(abi.make_config(**STRIP), v, n, c, rot, cam, light, STRIP_FOCAL, nthreads=8)

    def one(knobs, flags=0, table=False):
        tr = wm.context(STRIP, dict(wm.KNOBS, **knobs), sc, flags)
        a, f = tr.render(rot, cam, light, STRIP_FOCAL, want_rgb=True)
        d = (tr.wave_seeds_wide(), tr.wave_seeds()) if table else None
        prim = tr.render_aov(rot, cam, STRIP_FOCAL, sample=None, planes=("prim",))["prim"] if table else None
        tr.close()
        return (a, f), d, prim

    for what, knobs, flags in (("UOB_RT_NO_SEED=1", {"UOB_RT_NO_SEED": "1"}, 0), ("unculled", {}, abi.RT_FLAG_NO_CULL),
                               ("generic", {}, abi.RT_FLAG_GENERIC_KERNEL)):
        same(one(knobs, flags)[0], want, "%s/%s %s, %s against the oracle" % (kind, order, vname, what))
    partner, lower = tu.pair_tables(len(sc), pairs)
    for rows in ("1", "4", "16"):
        got, (wide, strict), prim = one({"UOB_RT_SEED_ROWS": rows}, table=True)
        same(got, want, "%s/%s %s, seeded with %s rows per tile, against the oracle" % (kind, order, vname, rows))
        if kind in ("same", "reversed"):                         # the same three points: every hit on a pair is a tie
            assert np.array_equal(np.where(prim >= 0, lower[np.where(prim >= 0, prim, 0)], prim), prim), "an id that is not a pair's lower index"
        check_table(strict, prim, sc)
        if int(rows) <= STRIP["height"]:                         # (the helper reads the centre row of a whole tile)
            check_wide_table(wide, prim, sc, DEFAULT)
        with capsys.disabled():
            print("\n[ties] strip %s/%s %s R=%s: %d of %d pixels on a pair, %s" % (kind, order, vname, rows, on, of, wide_counters(wide)))
        assert wide["jobs_primary"] > 0, "no job of the strip started from a record"


# ---- 2. the mesh kernel, n > 64 -------------------------------------------------------------------------------------------

MESH_FLAGS = (0, abi.RT_FLAG_NO_TILE_BINS, abi.RT_FLAG_GENERIC_KERNEL)
MESH_SAMPLES = (2, 16, 17, 64)               # 16 and 17: the two lane mappings of level 3


def mesh_kw(samples, **extra):
    return dict(dict(width=96, height=64, aa_x=1, aa_y=1, shadow_samples=samples), **extra)


def samples_of(size, arrangement):
    return MESH_SAMPLES[(3 * tu.MESH_SIZES.index(size) + tu.ARRANGEMENTS.index(arrangement)) % 4]


@pytest.mark.parametrize("flags", MESH_FLAGS)
@pytest.mark.parametrize("arrangement", tu.ARRANGEMENTS)
@pytest.mark.parametrize("size", tu.MESH_SIZES, ids=lambda s: "%dx%d" % s)
def test_mesh_frames(size, arrangement, flags, scene, oracle, meshes):
    sc, _ = tu.mesh_scene(scene, meshes[size], arrangement)
    kw = mesh_kw(samples_of(size, arrangement))
    views = tu.views_of("mesh")
    got = render(kw, sc, views, flags)
    for vi, vname in enumerate(views):
        same(got[vi], oracle_frame(oracle, ("mesh", size, arrangement), kw, sc, vname),
             "%s %s flags %d %s against the oracle" % (size, arrangement, flags, vname))


@pytest.mark.parametrize("how", ["morton", "replace_scene_device", "RT_UPDATE_DEVICE_TILES", "RT_UPDATE_REORDER"])
@pytest.mark.parametrize("size", tu.MESH_SIZES, ids=lambda s: "%dx%d" % s)
def test_mesh_tile_orders(size, how, scene, oracle, meshes):
    """The shuffled double-sided mesh in tiles made four other ways than rt_init's kd order (test_mesh_frames)"""
    import torch
    sc, _ = tu.mesh_scene(scene, meshes[size], "shuffled")
    other, _ = tu.mesh_scene(scene, meshes[size], "mesh_copies")           # the same count in another order
    kw = mesh_kw(16)
    if how == "morton":
        tr = wm.context(kw, {"UOB_RT_TILE_ORDER": "morton"}, sc)
    elif how == "replace_scene_device":
        tr = rt.RayTracer(abi.make_config(**kw), scene + rt.Scene(meshes[size]))       # another count
        keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in sc.packed()]
        tr.replace_scene_device(*keep)
        torch.cuda.synchronize()
    else:
        tr = rt.RayTracer(abi.make_config(**kw), other)
        tr.update_scene(sc, device_tiles=how == "RT_UPDATE_DEVICE_TILES", reorder=how == "RT_UPDATE_REORDER")
    orig, _ = tr.tile_data()
    assert np.array_equal(np.sort(orig), np.arange(len(sc))), "the tiled order is no permutation"
    views = tu.views_of("mesh")
    got = frames_of(tr, kw, views)
    tr.close()
    for vi, vname in enumerate(views):
        same(got[vi], oracle_frame(oracle, ("mesh", size, "shuffled"), kw, sc, vname), "%s %s %s against the oracle" % (size, how, vname))


@pytest.mark.parametrize("size", tu.MESH_SIZES, ids=lambda s: "%dx%d" % s)
def test_mesh_cooperative_blocks(size, scene, oracle, meshes, monkeypatch):
    """Five frames of one context with UOB_RT_MASK_DEBUG=8: every block from frame 2 on is cooperative — the four waves
    share the tiles and merge_hits merges their closest hits per lane"""
    monkeypatch.setenv("UOB_RT_MASK_DEBUG", "8")                          # read once, in rt_init
    sc, _ = tu.mesh_scene(scene, meshes[size], "shuffled")
    kw = mesh_kw(16)
    tr = rt.RayTracer(abi.make_config(**kw), sc)
    for k, vname in enumerate(("mesh_front", "mesh_front", "mesh_side", "mesh_side", "mesh_front")):
        got = tr.render(*pose(kw, vname), want_rgb=True)
        same(got, oracle_frame(oracle, ("mesh", size, "shuffled"), kw, sc, vname), "%s frame %d (%s) against the oracle" % (size, k, vname))
    tr.close()


@pytest.mark.parametrize("max_bounces", [1, 10])
@pytest.mark.parametrize("variant", ["mirror_mesh", "mirror_wall"])
def test_mesh_bounces(variant, max_bounces, scene, oracle, meshes):
    """bounce_tile: a mirror mesh under diffuse copies (or the other way round, by the order), and a mirror wall whose bounce
    rays meet the tied mesh"""
    kw = mesh_kw(2, max_bounces=max_bounces)
    views = tu.views_of(variant)
    for arrangement in ("shuffled", "copies_mesh"):
        sc, _ = tu.mesh_scene(scene, meshes[(10, 8)], arrangement, variant)
        for flags in MESH_FLAGS:
            got = render(kw, sc, views, flags)
            for vi, vname in enumerate(views):
                same(got[vi], oracle_frame(oracle, ("mesh", variant, arrangement), kw, sc, vname),
                     "%s %s %d bounces flags %d %s against the oracle" % (variant, arrangement, max_bounces, flags, vname))


# ---- 3. the calls beside the frame ------------------------------------------------------------------------------------------

def check_calls(tr, kw, sc, pairs, oracle, vname, device_entry=False):
    """AOV, ray queries, radiance and shade of the context's scene `sc` against the oracle.  -> AOV pixels on a pair"""
    cfg = abi.make_config(**kw)
    assert cfg.aa_x * cfg.aa_y == 1
    rot, cam, light, focal = pose(kw, vname)
    v, n, c = sc.packed()
    partner, lower = tu.pair_tables(len(sc), pairs)
    # the AOV planes; the id of a pixel whose closest hit is a paired triangle is the pair's lower index
    dirs = aov_util.primary_directions(cfg, rot, focal)[:, :, 0]
    rays = aov_util.rays_of(cam, dirs)
    tri, out10 = oracle.closest_hit(cfg, v, n, c, rays)
    aov = tr.render_aov(rot, cam, focal, sample=0)
    aov_util.assert_planes_equal(aov, aov_util.expected_planes(cam, dirs, tri, out10))
    prim = aov["prim"].reshape(-1)
    paired = (tri >= 0) & (partner[np.where(tri >= 0, tri, 0)] >= 0)
    assert paired.sum() >= 200, "the view shows a pair on %d pixels" % paired.sum()
    assert np.array_equal(prim[paired], lower[prim[paired]]) and np.array_equal(prim[paired], lower[tri[paired]])
    # ray queries, host entries: the AOV's rays and 4 000 seeded ones aimed at the pairs
    q = np.ascontiguousarray(np.concatenate([aov_util.rays_of(cam, aov["direction"][..., :3]), tu.seeded_rays(4000, 99, sc, pairs)]), F)
    wt, wo = oracle.closest_hit(cfg, v, n, c, q)
    gt, go = tr.query_closest_hit(q)
    assert np.array_equal(gt, wt), "closest hit: %d winners differ" % (gt != wt).sum()
    hit = wt != -1
    assert np.array_equal(su.u32(go[hit]), su.u32(wo[hit]))
    sh = q.copy()                                                # through the hit and as far again: blocked by the pair itself
    sh[:, 3:6] = (F(2.0) * (wo[:, 0:3] - q[:, 0:3]).astype(F)).astype(F)
    sh = np.ascontiguousarray(sh[hit])
    r2 = (sh[:, 3:6] * sh[:, 3:6]).sum(1).astype(F)
    want_sh = oracle.in_shadow(cfg, v, c, sh, r2)
    assert want_sh.any()
    assert np.array_equal(tr.query_in_shadow(sh, r2), want_sh)
    if device_entry:                                             # the device entry, on a side stream
        import torch
        dev = tr._torch_device()
        d_rays = torch.from_numpy(q).to(dev)
        d_sh, d_r2 = torch.from_numpy(sh).to(dev), torch.from_numpy(r2).to(dev)
        torch.cuda.synchronize(dev)
        s = torch.cuda.Stream(dev)
        d_tri, d_out = tr.query_device(abi.RT_TRACE_CLOSEST_HIT, d_rays, stream=s)
        d_blocked = tr.query_device(abi.RT_TRACE_IN_SHADOW, d_sh, radius_sq=d_r2, stream=s)
        s.synchronize()
        assert np.array_equal(d_tri.cpu().numpy(), wt) and np.array_equal(su.u32(d_out.cpu().numpy()[hit]), su.u32(wo[hit]))
        assert np.array_equal(d_blocked.cpu().numpy().astype(np.uint8), want_sh)
    # radiance: one AA sample per pixel, so the call's colour is the frame's float output
    _, rgb = tr.render(rot, cam, light, focal, want_rgb=True)
    o_rgb = oracle.render(cfg, v, n, c, rot, cam, light, focal, nthreads=8)[1]
    ids = su.pixel_ids(range(cfg.height), cfg.width).reshape(-1)
    rgba, rprim = tr.radiance_rays(aov_util.rays_of(cam, aov["direction"][..., :3]), light, seeds=ids, want_prim=True)
    assert np.array_equal(su.u32(ru.pixel_colour(rgba[:, None, :3])), su.u32(rgb[..., :3].reshape(-1, 3)))
    assert np.array_equal(su.u32(ru.pixel_colour(rgba[:, None, :3])), su.u32(o_rgb))
    assert np.array_equal(rprim, prim)
    # shade: the AOV's points, seeded as the frame seeds them, with the oracle's shadow masks
    pts = tri >= 0
    p, nr = aov["position"].reshape(-1, 4)[pts, :3], aov["normal"].reshape(-1, 4)[pts, :3]
    got, cnt = tr.shade_points(p, nr, light, seeds=ids[pts], want_counts=True)
    want, wcnt, _ = su.direct_light(p, nr, ids[pts], light, cfg.shadow_samples, cfg.light_spread,
                                    lambda r, rr: oracle.in_shadow(cfg, v, c, r, rr))
    assert su.same_bits(got, want).all() and np.array_equal(cnt, wcnt)
    return int(paired.sum())


@pytest.mark.parametrize("which", ["box", "mesh"])
def test_calls_beside_the_frame(which, scene, oracle, meshes):
    kw = mesh_kw(16)
    if which == "box":
        sc, pairs = tu.box_scene(scene, "reversed", "first")
        vname = "default"
    else:
        sc, pairs = tu.mesh_scene(scene, meshes[(10, 8)], "shuffled")
        vname = "mesh_front"
    tr = rt.RayTracer(abi.make_config(**kw), sc)
    check_calls(tr, kw, sc, pairs, oracle, vname, device_entry=True)
    tr.close()


# ---- 4. two objects that coincide after a refit ----------------------------------------------------------------------------
# Measured on an MI355X (printed by the test): see DESIGN.md 7, "closest-hit ties".

@pytest.mark.parametrize("coop", [False, True], ids=["plain", "cooperative"])
@pytest.mark.parametrize("size", tu.MESH_SIZES, ids=lambda s: "%dx%d" % s)
def test_coinciding_objects_after_a_refit(size, coop, scene, oracle, meshes, capsys, monkeypatch):
    """A context made with the copy displaced, so that it has tiles of its own, then rt_update_scene (refit: the tiling
    stays) to the scene where the copy lies exactly on the mesh: the triangles of a pair sit in different tiles, and for one
    sign of the displacement the HIGHER original index in the EARLIER tile — a plain `t < best` carried across tiles keeps the
    wrong one there.  Frames and the calls beside them against the oracle.  `cooperative`: the contexts made under
    UOB_RT_MASK_DEBUG=8 and five frames each, so that from frame 2 on the four waves of a block share the tiles and the two
    triangles of a pair reach merge_hits from different waves."""
    if coop:
        monkeypatch.setenv("UOB_RT_MASK_DEBUG", "8")                      # read once, in rt_init
    kw = mesh_kw(16)
    views = tu.views_of("mesh")
    best = 0
    for order in ("copy_first", "mesh_first"):
        for sign in (1.0, -1.0):
            apart, together, pairs = tu.coinciding(scene, meshes[size], order, (sign * 0.5, 0.0, 0.0))
            tr = rt.RayTracer(abi.make_config(**kw), apart)
            tr.render(*pose(kw, views[0]))
            tr.update_scene(together)                                    # refit
            tiles = tu.tile_positions(tr, together, pairs)
            orig, _ = tr.tile_data()
            slot = np.empty(len(orig), np.int64)
            slot[orig] = np.arange(len(orig))
            assert np.array_equal(tiles, slot[pairs] // 64), "tile_positions disagrees with the context's own tiled order"
            split, inverted = tu.split_counts(tiles)
            with capsys.disabled():
                print("\n[ties] coinciding %s %s offset %+.1f: of %d pairs %d split across two tiles, %d with the higher index in "
                      "the earlier tile" % (size, order, sign * 0.5, len(pairs), split, inverted))
            assert 2 * split >= len(pairs), "fewer than half of the pairs are split across two tiles"
            best = max(best, inverted)
            for k, vname in enumerate((views + views + views[:1]) if coop else views):
                same(tr.render(*pose(kw, vname), want_rgb=True), oracle_frame(oracle, ("coinciding", size, order), kw, together, vname),
                     "%s %s %+.1f frame %d (%s) after the refit, against the oracle" % (size, order, sign * 0.5, k, vname))
            if not coop:
                check_calls(tr, kw, together, pairs, oracle, views[0])
            tr.close()
            for flags in () if coop else (abi.RT_FLAG_NO_TILE_BINS,):
                tr = rt.RayTracer(abi.make_config(flags=flags, **kw), apart)
                tr.update_scene(together)
                got = frames_of(tr, kw, views)
                tr.close()
                for vi, vname in enumerate(views):
                    same(got[vi], oracle_frame(oracle, ("coinciding", size, order), kw, together, vname),
                         "%s %s %+.1f %s flags %d after the refit" % (size, order, sign * 0.5, vname, flags))
    assert 4 * best >= len(pairs), "in no arrangement a quarter of the pairs has the higher index in the earlier tile"
