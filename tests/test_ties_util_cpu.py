"""CPU: every scene builder of tests/ties_util.py holds what it claims, by the oracle alone, at the frame sizes and views
tests/test_gpu_ties.py renders: rays that meet the two triangles of a pair at bit-equal t — the lower original index wins in
either order of the pair, so what the ray shows flips with the order — at least 200 of them per scene.  The counts are
conditions on the INPUTS of the GPU tests, printed with -s; none of them is a result of the code under test."""
import numpy as np
import pytest

import ties_util as tu
from uob_raytracer_amd import abi, runtime as rt

BOX_FRAME = dict(width=160, height=96, aa_x=1, aa_y=1, shadow_samples=1)
MESH_FRAME = dict(width=96, height=64, aa_x=1, aa_y=1, shadow_samples=1)
MIN_FLIPS = 200


@pytest.fixture(scope="module")
def meshes(tmp_path_factory):
    d = tmp_path_factory.mktemp("ties_meshes")
    return {size: tu.load_mesh(size[0], size[1], d) for size in tu.MESH_SIZES}


def counts(oracle, kw, sc, pairs, views):
    """census summed over the views' primary rays"""
    cfg = abi.make_config(**kw)
    total = {}
    for name in views:
        yaw, pitch, cam, _, lens = tu.view(name)
        c = tu.census(oracle, cfg, sc, pairs, tu.primary_rays(cfg, rt.rotation_matrix(yaw, pitch), cam, tu.focal_for(cfg, lens)))
        c.pop("winner")
        total = {k: total.get(k, 0) + v for k, v in c.items()}
    return total


def frame_flips(oracle, kw, sc, pairs, vname):
    """Pixels of the frame that change when the two triangles of every pair change places"""
    cfg = abi.make_config(**kw)
    yaw, pitch, cam, light, lens = tu.view(vname)
    rot, focal = rt.rotation_matrix(yaw, pitch), tu.focal_for(cfg, lens)
    frames = []
    for s in (sc, tu.swapped(sc, pairs)):
        v, n, c = s.packed()
        frames.append(oracle.render(cfg, v, n, c, rot, cam, light, focal)[0])
    return frames[0] != frames[1]


@pytest.mark.parametrize("order", tu.ORDERS)
@pytest.mark.parametrize("kind", tu.BOX_KINDS)
def test_box_scenes_hold_ties(kind, order, scene, oracle):
    sc, pairs = tu.box_scene(scene, kind, order)
    assert len(sc) <= 64 and (pairs[:, 0] < pairs[:, 1]).all()
    c = counts(oracle, BOX_FRAME, sc, pairs, tu.views_of(kind))
    print("\n[ties] box %s/%s over %s: %s" % (kind, order, tu.views_of(kind), c))
    assert c["higher"] == 0, "the higher index of a pair won in both orders"
    assert c["tied"] >= MIN_FLIPS
    if kind in ("same", "reversed"):                 # the same three points: every hit on a pair is a tie
        assert c["tied"] == c["on_pair"] and c["untied"] == 0 and c["other"] == 0
    else:                                            # near ties, decided by the last bit of t
        assert c["untied"] > 0


@pytest.mark.parametrize("material", ["mirror", "glass"])
@pytest.mark.parametrize("kind", ["same", "reversed"])
def test_material_of_the_winner_shows(kind, material, scene, oracle):
    """A copy of another material: the winner decides between lit, reflect and refract, in the whole frame"""
    kw = dict(BOX_FRAME, max_bounces=5)
    for order in tu.ORDERS:
        sc, pairs = tu.box_scene(scene, kind, order, material)
        flips = sum(int(frame_flips(oracle, kw, sc, pairs, v).sum()) for v in tu.views_of(kind))
        print("\n[ties] box %s/%s %s: %d pixels flip with the order" % (kind, order, material, flips))
        assert flips >= MIN_FLIPS


@pytest.mark.parametrize("arrangement", tu.ARRANGEMENTS)
@pytest.mark.parametrize("size", tu.MESH_SIZES)
def test_mesh_scenes_hold_ties(size, arrangement, scene, oracle, meshes):
    sc, pairs = tu.mesh_scene(scene, meshes[size], arrangement)
    assert len(sc) == len(scene) + 2 * len(meshes[size]) and (pairs[:, 0] < pairs[:, 1]).all()
    for lo, hi in pairs[::17]:                       # a pair is the same three points, v1 and v2 exchanged
        a, b = sc.aos[lo], sc.aos[hi]
        assert np.array_equal(a[0], b[0]) and (np.array_equal(a[1], b[2]) and np.array_equal(a[2], b[1]))
    for vname in tu.views_of("mesh"):                # each view on its own: the GPU tests take either
        c = counts(oracle, MESH_FRAME, sc, pairs, (vname,))
        print("\n[ties] mesh %s %s %s: %d triangles, %s" % (size, arrangement, vname, len(sc), c))
        assert c["tied"] >= MIN_FLIPS and c["tied"] == c["on_pair"] and c["higher"] == 0


@pytest.mark.parametrize("variant", ["mirror_mesh", "mirror_wall"])
def test_mesh_variants_flip_the_frame(variant, scene, oracle, meshes):
    kw = dict(MESH_FRAME, max_bounces=10)
    sc, pairs = tu.mesh_scene(scene, meshes[(10, 8)], "shuffled", variant)
    cfg = abi.make_config(**kw)
    for vname in tu.views_of(variant):
        flips = frame_flips(oracle, kw, sc, pairs, vname)
        yaw, pitch, cam, _, lens = tu.view(vname)
        c = tu.census(oracle, cfg, sc, pairs, tu.primary_rays(cfg, rt.rotation_matrix(yaw, pitch), cam, tu.focal_for(cfg, lens)))
        partner, _ = tu.pair_tables(len(sc), pairs)
        w = c["winner"]
        primary = (w >= 0) & (partner[np.where(w >= 0, w, 0)] >= 0)
        behind = int((flips & ~primary).sum())       # pixels that flip though their primary ray meets no pair: a bounce ray did
        print("\n[ties] mesh (10, 8) shuffled %s %s: %d pixels flip, %d of them behind a bounce" % (variant, vname, flips.sum(), behind))
        assert flips.sum() >= MIN_FLIPS
        if variant == "mirror_wall":
            assert behind >= MIN_FLIPS, "no bounce ray of the mirror wall meets the tied mesh"


@pytest.mark.parametrize("order", ["copy_first", "mesh_first"])
@pytest.mark.parametrize("size", tu.MESH_SIZES)
def test_coinciding_objects(size, order, scene, oracle, meshes):
    for sign in (1.0, -1.0):
        apart, together, pairs = tu.coinciding(scene, meshes[size], order, (sign * 0.5, 0.0, 0.0))
        n = len(together)
        assert len(apart) == n and np.array_equal(apart.aos[:, 4], together.aos[:, 4])
        assert len({together.aos[i, 4].tobytes() for i in range(n)}) == n, "a colour per triangle"
        moved = np.flatnonzero((apart.aos[:, :3] != together.aos[:, :3]).any((1, 2)))
        which = pairs[:, 0] if order == "copy_first" else pairs[:, 1]
        assert np.array_equal(moved, np.sort(which)), "only the copy moves"
        c0 = counts(oracle, MESH_FRAME, apart, pairs, tu.views_of("mesh"))
        assert c0["tied"] == 0, "the displaced copy ties with the mesh"
    c = counts(oracle, MESH_FRAME, together, pairs, tu.views_of("mesh"))
    print("\n[ties] coinciding %s %s: %s" % (size, order, c))
    assert c["tied"] >= MIN_FLIPS and c["tied"] == c["on_pair"] and c["higher"] == 0


@pytest.mark.parametrize("which", ["box_reversed", "box_decal_wall", "mesh"])
def test_seeded_rays_meet_ties(which, scene, oracle, meshes):
    if which == "mesh":
        sc, pairs = tu.mesh_scene(scene, meshes[(10, 8)], "shuffled")
    else:
        sc, pairs = tu.box_scene(scene, which[4:], "first")
    rays = tu.seeded_rays(4000, 77, sc, pairs)
    assert rays.shape == (4000, 6) and rays.dtype == np.float32 and np.isfinite(rays).all()
    c = tu.census(oracle, abi.make_config(**BOX_FRAME), sc, pairs, rays)
    print("\n[ties] seeded rays into %s: %s" % (which, {k: v for k, v in c.items() if k != "winner"}))
    assert c["tied"] >= MIN_FLIPS and c["higher"] == 0


def test_swapped_and_tables(scene):
    sc, pairs = tu.box_scene(scene, "reversed", "first")
    sw = tu.swapped(sc, pairs)
    assert np.array_equal(sw.aos[pairs[:, 0]], sc.aos[pairs[:, 1]]) and np.array_equal(sw.aos[pairs[:, 1]], sc.aos[pairs[:, 0]])
    rest = np.setdiff1d(np.arange(len(sc)), pairs.ravel())
    assert np.array_equal(sw.aos[rest], sc.aos[rest])
    partner, lower = tu.pair_tables(len(sc), pairs)
    assert (partner[pairs[:, 0]] == pairs[:, 1]).all() and (lower[pairs[:, 1]] == pairs[:, 0]).all() and (partner[rest] == -1).all()
    for winding in ("same", "reversed", "rotated"):
        t = tu.copy_of(scene.aos[tu.FACES], winding)
        for a, b in zip(scene.aos[tu.FACES], t):
            assert {x.tobytes() for x in a[:3]} == {x.tobytes() for x in b[:3]}, "a copy lies on the same three points"
    d = tu.decal_of(scene.aos[tu.BACK_WALL])
    assert (d[:, :3, 2] == scene.aos[tu.BACK_WALL, :3, 2]).all() and np.abs(d[:, :3, :2]).max() == np.float32(0.6)
