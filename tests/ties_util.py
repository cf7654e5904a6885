"""Scenes with exact closest-hit ties, for tests/test_ties_util_cpu.py, tests/test_gpu_ties.py and the tie cases of
tests/test_oracle_vs_ref.py.

The reference replaces a hit only for a strictly smaller t and visits the triangles in their original order (kernels.cl:120,
:194): of several hits at bit-equal t the lowest original index wins.  Every builder here returns (scene, pairs): pairs is
int64 [k, 2], per tied pair the two original indices, lower first.  The two triangles of a pair are the same three points
(duplicates: same winding, reversed winding, vertex order rotated) or lie in one plane and overlap (a decal in a wall).  Each
copy carries a colour of its own, and a material of the caller's choice, so the winner decides what a pixel shows.

`census` states with the oracle alone what a scene holds for a set of rays; `swapped` exchanges the two triangles of every
pair, which is how a tie shows: with bit-equal t the lower INDEX wins in both orders (the visible material flips), with
unequal t the same TRIANGLE wins in both (the winning index flips)."""
import os

import numpy as np

import aov_util
from uob_raytracer_amd import abi, meshgen, runtime as rt

F = np.float32
FLOOR = [0, 1]                                # TestModelH.h: floor, left, right, ceiling, back wall; short block; tall block
BACK_WALL = [8, 9]
TALL_FACE = [18, 19]                          # the tall block's face towards the default camera
FACES = FLOOR + BACK_WALL + TALL_FACE
MIRROR = (1.0, 1.0, 1.0, 0.0)
MATERIAL_W = {"diffuse": 1.0, "mirror": 0.0, "glass": -1.0}
# one colour per copy, none of them a colour of the box
PALETTE = [(0.9, 0.1, 0.1), (0.1, 0.8, 0.2), (0.1, 0.3, 0.9), (0.9, 0.8, 0.1), (0.8, 0.2, 0.8), (0.1, 0.8, 0.8)]
COPY_COLOUR = (0.2, 0.7, 0.3, 1.0)            # the copies of a mesh
MIRROR_WALL_SHIFT = (0.9, -0.775, 1.15)       # the mesh of the `mirror_wall` variant: in mid-air in the free right rear of the room
DEFAULT_CAM = [0.0, 0.0, -3.2]                # skeleton.cpp:61-67
DEFAULT_LIGHT = [0.0, -0.5, -0.7]

BOX_KINDS = ("same", "reversed", "rotated", "decal_wall", "decal_floor")
ORDERS = ("after", "first")                   # the copies appended to the box / the copies, then the box
ARRANGEMENTS = ("mesh_copies", "copies_mesh", "shuffled")
MESH_SIZES = ((10, 8), (24, 16))              # 140 faces: 306 triangles with the copies, 5 tiles; 720 faces: 1466, 23 tiles


# ---- copies ------------------------------------------------------------------------------------------------------------

def copy_of(tris, winding):
    """Copies of triangles [k, 5, 4] on the same points: `same`; `reversed` (v1 and v2 exchanged, the normal negated);
    `rotated` (v1, v2, v0: the same orientation, another first vertex)"""
    t = np.array(tris, F, copy=True).reshape(-1, 5, 4)
    src = t.copy()
    if winding == "reversed":
        t[:, 1], t[:, 2] = src[:, 2], src[:, 1]
        t[:, 3, :3] = -src[:, 3, :3]
    elif winding == "rotated":
        t[:, 0], t[:, 1], t[:, 2] = src[:, 1], src[:, 2], src[:, 0]
    elif winding != "same":
        raise KeyError(winding)
    return t


def decal_of(quad, scale=0.6):
    """The two triangles of a quad scaled about the middle of its box, FP32: in an axis-aligned quad the coordinate across the
    plane has v - c == 0 and stays what it is, bit for bit, so the decal lies exactly in the plane"""
    t = np.array(quad, F, copy=True).reshape(-1, 5, 4)
    pts = t[:, :3, :3].reshape(-1, 3)
    c = ((pts.min(0) + pts.max(0)) * F(0.5)).astype(F)
    t[:, :3, :3] = (c + F(scale) * (t[:, :3, :3] - c).astype(F)).astype(F)
    return t


def _coloured(tris, material, palette=PALETTE):
    t = tris.copy()
    for k in range(len(t)):
        t[k, 4, :3] = palette[k % len(palette)]
        t[k, 4, 3] = MATERIAL_W[material]
    return t


def _assemble(base, copies, src, order):
    """-> (aos, pairs): copy k duplicates base[src[k]]"""
    nb, nc = len(base), len(copies)
    src = np.asarray(src, np.int64)
    if order == "after":
        return np.concatenate([base, copies]), np.stack([src, nb + np.arange(nc)], 1)
    if order == "first":
        return np.concatenate([copies, base]), np.stack([np.arange(nc), nc + src], 1)
    raise KeyError(order)


def box_scene(box, kind, order="after", material="diffuse"):
    """The box (n <= 64) plus, by kind: duplicates of the floor, the back wall and one face of the tall block — `same`,
    `reversed`, `rotated` — or a 0.6-scale decal lying exactly in the back wall / the floor (`decal_wall`, `decal_floor`).
    The copies in colours of their own and of the given material.  -> (Scene, pairs)"""
    base = box.aos
    if kind in ("same", "reversed", "rotated"):
        src = FACES
        copies = copy_of(base[src], kind)
    elif kind in ("decal_wall", "decal_floor"):
        src = BACK_WALL if kind == "decal_wall" else FLOOR
        copies = decal_of(base[src])
    else:
        raise KeyError(kind)
    aos, pairs = _assemble(base, _coloured(copies, material), src, order)
    return rt.Scene(aos), pairs


def load_mesh(lon, lat, tmpdir, color=None):
    """meshgen.write_sphere_obj(lon, lat) through the product's loader: the triangles [nf, 5, 4]"""
    path = os.path.join(str(tmpdir), "ties_%dx%d.obj" % (lon, lat))
    meshgen.write_sphere_obj(path, lon, lat)
    return rt.Scene.load_obj(path, color=color).aos


def mesh_scene(box, mesh, arrangement="mesh_copies", variant=None, seed=11):
    """The box plus a mesh [nf, 5, 4] with EVERY face a second time, reversed winding, in another colour ("double-sided").
    arrangement: the original order (ARRANGEMENTS; `shuffled` is a seeded permutation of the whole scene).  variant:
    `mirror_mesh` (the mesh's faces mirrors, the copies diffuse), `mirror_wall` (a mirror back wall: bounce rays meet the tied
    mesh).  -> (Scene, pairs)"""
    base = box.aos.copy()
    mesh = np.array(mesh, F, copy=True)
    if variant == "mirror_wall":               # where the loader puts it the tall block stands between the mesh and the wall
        mesh[:, :3, :3] = (mesh[:, :3, :3] + np.asarray(MIRROR_WALL_SHIFT, F)).astype(F)
    copies = copy_of(mesh, "reversed")
    copies[:, 4, :] = np.asarray(COPY_COLOUR, F)
    if variant == "mirror_mesh":
        mesh[:, 4, :] = np.asarray(MIRROR, F)
    elif variant == "mirror_wall":
        base[BACK_WALL, 4, :] = np.asarray(MIRROR, F)
    elif variant is not None:
        raise KeyError(variant)
    nb, nf = len(base), len(mesh)
    k = np.arange(nf)
    if arrangement == "copies_mesh":
        aos, pairs = np.concatenate([base, copies, mesh]), np.stack([nb + k, nb + nf + k], 1)
    else:
        aos, pairs = np.concatenate([base, mesh, copies]), np.stack([nb + k, nb + nf + k], 1)
        if arrangement == "shuffled":
            perm = np.random.default_rng(seed).permutation(len(aos))       # new position j holds old triangle perm[j]
            where = np.empty(len(aos), np.int64)
            where[perm] = np.arange(len(aos))
            aos, pairs = aos[perm], np.sort(where[pairs], 1)
        elif arrangement != "mesh_copies":
            raise KeyError(arrangement)
    return rt.Scene(aos), pairs


def unique_colours(aos):
    """Every triangle a diffuse colour of its own (exact in FP32), so that a tiled copy can be matched to the original order"""
    aos = aos.copy()
    i = np.arange(len(aos))
    aos[:, 4, 0] = (F(0.25) + (i % 16 + 1).astype(F) / F(32.0)).astype(F)
    aos[:, 4, 1] = (F(0.25) + ((i // 16) % 16 + 1).astype(F) / F(32.0)).astype(F)
    aos[:, 4, 2] = ((i // 256 + 1).astype(F) / F(16.0)).astype(F)
    aos[:, 4, 3] = F(1.0)
    return aos


def coinciding(box, mesh, order="copy_first", offset=(0.5, 0.0, 0.0)):
    """Two objects that coincide for a frame.  -> (apart, together, pairs): `apart` is the box, the copy C' of the mesh
    (reversed winding) displaced by `offset`, and the mesh M, C' before M in the original order (`copy_first`) or after it
    (`mesh_first`); `together` is the same scene with C' exactly on M.  A context made from `apart` gives C' tiles of its
    own; rt_update_scene (refit) to `together` keeps that tiling, so the two triangles of a pair sit in different tiles, and
    — by the sign of the offset — the higher original index in the EARLIER one, where a plain `t < best` carried across tiles
    keeps the wrong triangle.  Every triangle in a colour of its own (see tile_positions)."""
    base, mesh = box.aos, np.array(mesh, F, copy=True)
    copies = copy_of(mesh, "reversed")
    moved = copies.copy()
    moved[:, :3, :3] = (moved[:, :3, :3] + np.asarray(offset, F)).astype(F)
    nb, nf = len(base), len(mesh)
    k = np.arange(nf)
    pairs = np.stack([nb + k, nb + nf + k], 1)
    if order == "copy_first":
        apart, together = [base, moved, mesh], [base, copies, mesh]
    elif order == "mesh_first":
        apart, together = [base, mesh, moved], [base, mesh, copies]
    else:
        raise KeyError(order)
    return (rt.Scene(unique_colours(np.concatenate(apart))), rt.Scene(unique_colours(np.concatenate(together))), pairs)


def tile_positions(tr, scene, pairs, tile=64):
    """The tile numbers [k, 2] of the two triangles of every pair (column 0: the lower original index) in the mesh kernel's
    tiled copy of `scene`, the scene the context `tr` holds: the tiled permutation is recovered from
    scene_data(tiled=True) by matching vertices and colours, which must therefore be unique per triangle."""
    d = tr.scene_data(tiled=True)
    v, _, c = scene.packed()
    n = len(scene)

    def keys(vv, cc):
        return [vv[3 * j:3 * j + 3].tobytes() + cc[j].tobytes() for j in range(n)]

    index = {k: i for i, k in enumerate(keys(v, c))}
    assert len(index) == n, "tile_positions needs a unique (vertices, colour) per triangle"
    slot = np.empty(n, np.int64)
    seen = np.zeros(n, bool)
    for j, k in enumerate(keys(d["vertices_m"], d["colors_m"])):
        i = index[k]                                         # KeyError: the tiled copy holds a triangle the scene does not
        assert not seen[i]
        slot[i], seen[i] = j, True
    return slot[np.asarray(pairs)] // tile


def split_counts(tiles):
    """(pairs split across two tiles, pairs whose HIGHER original index sits in the EARLIER tile) of tile_positions' answer"""
    return int((tiles[:, 0] != tiles[:, 1]).sum()), int((tiles[:, 1] < tiles[:, 0]).sum())


# ---- what a scene holds ------------------------------------------------------------------------------------------------

def swapped(scene, pairs):
    """The scene with the two triangles of every pair exchanged in the original order"""
    aos = scene.aos.copy()
    aos[pairs[:, 0]], aos[pairs[:, 1]] = scene.aos[pairs[:, 1]], scene.aos[pairs[:, 0]]
    return rt.Scene(aos)


def pair_tables(n, pairs):
    """(partner [n] (-1: in no pair), lower [n]: the pair's lower index (own index where in no pair))"""
    partner = np.full(n, -1, np.int64)
    lower = np.arange(n)
    partner[pairs[:, 0]], partner[pairs[:, 1]] = pairs[:, 1], pairs[:, 0]
    lower[pairs[:, 1]] = pairs[:, 0]
    return partner, lower


def census(oracle, cfg, scene, pairs, rays):
    """The closest hits of `rays` in the scene and in swapped(scene), by the oracle.  -> dict of counts:
    on_pair   rays whose winner is a triangle of a pair;
    tied      of those, the lower index wins in BOTH orders (bit-equal t: what the ray shows flips with the order);
    untied    the same triangle wins in both orders (its index flips): t differs;
    higher    rays where the HIGHER index of a pair wins in both orders (never, for duplicates; a decal's outline apart);
    and `winner`, the winning index per ray in the scene as given."""
    v, n, c = scene.packed()
    t1, _ = oracle.closest_hit(cfg, v, n, c, rays)
    v, n, c = swapped(scene, pairs).packed()
    t2, _ = oracle.closest_hit(cfg, v, n, c, rays)
    partner, lower = pair_tables(len(scene), pairs)
    hit = t1 >= 0
    p1 = np.where(hit, partner[np.where(hit, t1, 0)], -1)
    on = hit & (p1 >= 0)
    is_lo = on & (lower[np.where(hit, t1, 0)] == t1)
    tied = on & (t2 == t1) & is_lo
    untied = on & (t2 == p1)
    higher = on & (t2 == t1) & ~is_lo
    return {"on_pair": int(on.sum()), "tied": int(tied.sum()), "untied": int(untied.sum()), "higher": int(higher.sum()),
            "other": int((on & ~tied & ~untied & ~higher).sum()), "winner": t1}


# ---- rays and frames ---------------------------------------------------------------------------------------------------

def primary_rays(cfg, rot, cam, focal):
    """[rows * W * aa, 6]: the frame's primary rays, as the AOV `direction` plane has them"""
    return aov_util.rays_of(cam, aov_util.primary_directions(cfg, rot, focal))


def seeded_rays(k, seed, scene, pairs):
    """k rays from points in the room towards points ON the paired triangles (random barycentrics), normalised"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.9, 0.9, (k, 3)).astype(F)
    o[:, 2] = rng.uniform(-3.0, -1.2, k).astype(F)             # in front of the box, as the camera is
    tri = scene.aos[pairs[rng.integers(0, len(pairs), k), 0]]
    b = rng.dirichlet((1.0, 1.0, 1.0), k).astype(F)
    target = (b[:, :, None] * tri[:, :3, :3]).sum(1).astype(F)
    d = (target - o).astype(F)
    d = (d / np.sqrt((d * d).sum(1, keepdims=True)).astype(F)).astype(F)
    return np.ascontiguousarray(np.concatenate([o, d], 1), F)


def view(name):
    """-> (yaw, pitch, cam, light, lens): lens multiplies the default focal length"""
    return {
        "default": (0.0, 0.0, DEFAULT_CAM, DEFAULT_LIGHT, 1.0),
        "side": (0.25, -0.05, [0.45, 0.1, -2.9], [0.2, -0.6, -0.4], 1.0),
        # the mesh stands on the floor left of the middle, at (-0.4, 0.78, -0.7): two views that fill a quarter of the frame with it
        "mesh_front": (0.0, 0.0, [-0.4, 0.7, -2.4], DEFAULT_LIGHT, 1.6),
        "mesh_side": (-0.35, -0.15, [0.25, 0.35, -2.3], [0.2, -0.6, -0.4], 1.6),
        # a decal's t equals its wall's on one hit in seven, bit for bit (other first vertex, other edges): a longer lens on
        # the wall, and two views down at the floor, hold enough of those
        "wall_zoom": (0.0, 0.0, DEFAULT_CAM, DEFAULT_LIGHT, 2.0),
        "wall_zoom_side": (0.1, 0.05, [0.2, 0.1, -2.8], DEFAULT_LIGHT, 2.0),
        "floor_near": (0.0, -1.2, [0.0, -0.9, -0.8], DEFAULT_LIGHT, 0.6),
        "floor_far": (0.0, -0.6, [0.0, -0.6, -2.6], DEFAULT_LIGHT, 1.5),
        # the shifted mesh of the `mirror_wall` variant from the left: beside it, its image in the back wall
        "mirror_wall": (0.36, 0.0, [-0.6, -0.1, -2.2], DEFAULT_LIGHT, 3.0),
        "mirror_wall_wide": (0.33, 0.0, [-0.6, -0.1, -2.2], DEFAULT_LIGHT, 2.4),
    }[name]


def views_of(kind):
    """The two views the tests render a box_scene kind / a mesh scene (`mesh`, or its variant) through"""
    return {"decal_wall": ("wall_zoom", "wall_zoom_side"), "decal_floor": ("floor_near", "floor_far"),
            "mesh": ("mesh_front", "mesh_side"), "mirror_mesh": ("mesh_front", "mesh_side"),
            "mirror_wall": ("mirror_wall", "mirror_wall_wide")}.get(kind, ("default", "side"))


def focal_for(cfg, lens=1.0):
    return 1100.0 * min(cfg.width, cfg.height) / 1024.0 * cfg.aa_x * lens


def config(**kw):
    return abi.make_config(**kw)
