"""Scenes of many small triangles for the scene-edit kernels above their size thresholds (tests/test_gpu_scene_sizes.py),
built vectorised in numpy, and two restatements independent of the library: the Morton order of the device tile build
(morton_order_np) and a sampled check of the tiles' data.  Checked on the CPU by tests/test_scene_sizes_util_cpu.py.

The thresholds, restated here so that the tests can assert that they cross them:"""
import ctypes as C

import numpy as np

from uob_raytracer_amd import abi, runtime as rt

SORT_CHUNK = 1024             # rt_tile_build.hip kSortChunk: elements of the sort owned by one wave
SORT_SCAN_TILE = 4096         # rt_tile_build.hip kSortScanTile: digit-table entries per step of rt_sort_scan
CHECK_GRID = 1024 * 256       # rt_scene_update.hip launch_scene_check: lanes of the capped grid
POSE_GRID = 2048 * 256        # rt_scene_pose.hip launch_pose: lanes of the capped grid
MAX_OBJECTS = 65535           # rt_host.h kPoseStatic = 0xffff marks "in no object"

F32 = np.float32
YELLOW = (0.7, 0.7, 0.2, 1.0)
GLASS = (0.0, 0.2, 0.5, -1.0)
N_BOX = 26


def sort_chunks(n):
    return (n + SORT_CHUNK - 1) // SORT_CHUNK


def scan_steps(n):
    """Steps of rt_sort_scan's loop for n triangles: its table has 256 entries per chunk."""
    return (256 * sort_chunks(n) + SORT_SCAN_TILE - 1) // SORT_SCAN_TILE


# ---- builders ---------------------------------------------------------------------------------------------------------
def small_triangles(centres, size=0.004, color=YELLOW):
    """AoS [m,5,4]: one upright triangle of half-width `size` around each centre (tests/test_gpu_scene_replace.py
    _small_triangles without its call per triangle).  The normals are left zero: finish() fills them."""
    c = np.asarray(centres, F32).reshape(-1, 3)
    s = F32(size)
    aos = np.zeros((len(c), 5, 4), F32)
    aos[:, 0, :3] = c + np.array([-s, -s, 0], F32)
    aos[:, 1, :3] = c + np.array([s, -s, 0], F32)
    aos[:, 2, :3] = c + np.array([0, s, 0], F32)
    aos[:, :3, 3] = 1.0
    aos[:, 4] = np.asarray(color, F32)
    return aos


def finish(aos):
    """The Scene of an AoS array, its normals filled by ONE rt_scene_transform call, the identity over [0, n), as
    Scene.posed fills them."""
    aos = np.ascontiguousarray(aos, F32).reshape(-1, 5, 4).copy()
    ident = np.ascontiguousarray(np.eye(3, 4, dtype=F32))
    rt.lib().rt_scene_transform(aos.ctypes.data_as(C.POINTER(abi.RtTriangle)), len(aos), 0, len(aos), rt._fp(ident))
    return rt.Scene(aos)


def box_and(box, small, box_last=False, box_scale=1.0):
    """The Cornell box (a Scene) and an AoS array of other triangles as one Scene: the box first, or last; box_scale
    shrinks the box's copy about the origin."""
    b = box.aos.copy()
    b[:, :3, :3] *= F32(box_scale)
    return finish(np.concatenate([small, b] if box_last else [b, small], 0))


def random_scene(box, n, seed):
    """n triangles: the box, then n - 26 small ones at seeded uniform centres inside it."""
    rng = np.random.default_rng(seed)
    return box_and(box, small_triangles(rng.uniform(-0.8, 0.8, (n - N_BOX, 3))))


CELL = 2.0 / 1023.0          # the box spans [-1, 1]^3: one Morton cell per axis


def key_case(box, case, m, seed=11):
    """The key distributions of tests/test_gpu_scene_replace.py _sort_cases with m small triangles behind the box:
    equal_keys    every small triangle has the same centre: one key;
    top_byte      centres 512 cells apart per axis: the keys differ in Morton bits 27..29 only;
    bottom_byte   centres 0..3 cells from a point whose cell numbers are multiples of four: bits 0..5 only;
    hot_digit     92 % of the small triangles share one centre, so in every pass of the sort one digit holds more
                  than 90 % of all elements; the others are spread;
    many_large    3000 'large' triangles (extent above a quarter of the scene's: key 0) spread evenly through the index range."""
    rng = np.random.default_rng(seed)
    if case == "equal_keys":
        return box_and(box, small_triangles(np.tile([0.1, 0.2, -0.3], (m, 1))))
    if case == "top_byte":
        far = -0.75 + 512.0 * CELL
        corners = np.array([[x, y, z] for x in (-0.75, far) for y in (-0.75, far) for z in (-0.75, far)], F32)
        return box_and(box, small_triangles(corners[rng.integers(0, 8, m)]))
    if case == "bottom_byte":
        near = np.array([0.3, 0.3, 0.3], F32) + rng.integers(0, 4, (m, 3)).astype(F32) * F32(CELL)
        return box_and(box, small_triangles(near, size=0.0004))
    if case == "hot_digit":
        c = rng.uniform(-0.8, 0.8, (m, 3))
        c[rng.permutation(m)[:(m * 92) // 100]] = (0.1, 0.2, -0.3)
        return box_and(box, small_triangles(c))
    if case == "many_large":
        aos = small_triangles(rng.uniform(-0.8, 0.8, (m, 3)))
        at = large_positions(m)
        aos[at] = small_triangles(rng.uniform(-0.3, 0.3, (len(at), 3)), size=0.5)
        return box_and(box, aos)
    raise KeyError(case)


N_LARGE = 3000


def large_positions(m):
    """Where key_case('many_large') puts its large triangles among the m small ones (add 26 for the scene's index)."""
    return (np.arange(N_LARGE, dtype=np.int64) * m) // N_LARGE


def check_scene(box, n, box_scale=1.0, seed=3):
    """n > CHECK_GRID triangles for rt_scene_check: n - 26 small ones, THEN the box, so that the extreme vertices of all
    three axes, lo and hi, belong to triangles of the grid-stride loop's second trip only; so do the only glass triangles
    (check_glass_indices).  box_scale < 1 gives a scene of the same count with another box."""
    assert n - N_BOX >= CHECK_GRID
    rng = np.random.default_rng(seed)
    aos = small_triangles(rng.uniform(-0.8, 0.8, (n - N_BOX, 3)))
    sc = box_and(box, aos, box_last=True, box_scale=box_scale)
    sc.aos[check_glass_indices(n), 4] = np.asarray(GLASS, F32)
    return sc


def check_glass_indices(n):
    return np.array([CHECK_GRID, CHECK_GRID + 5, n - N_BOX - 1, n - 1], np.int64)


OBJ_TRIS = 8


def pose_scene(box, nobj, seed=5):
    """26 + 8 nobj triangles for rt_pose_triangles: the box (static), then per object 8 consecutive small triangles around
    the object's centre.  Returns (Scene, ranges, centres [nobj,3])."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-0.8, 0.8, (nobj, 3)).astype(F32)
    offs = rng.uniform(-0.01, 0.01, (nobj, OBJ_TRIS, 3)).astype(F32)
    aos = small_triangles((centres[:, None, :] + offs).reshape(-1, 3), size=0.003)
    ranges = [(N_BOX + OBJ_TRIS * k, OBJ_TRIS) for k in range(nobj)]
    return box_and(box, aos), ranges, centres


def pose_xforms(centres, seed=9):
    """[nobj,3,4] float32: a seeded rotation about each object's centre plus a small translation; special_poses() names the
    objects that get a mirror, a non-uniform scale and a scale by 0 (which collapses the object: degenerate normals)."""
    rng = np.random.default_rng(seed)
    k = len(centres)
    axis = rng.normal(size=(k, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(-np.pi, np.pi, k)
    K = np.zeros((k, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -axis[:, 2], axis[:, 1], axis[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3)[None] + np.sin(ang)[:, None, None] * K + (1.0 - np.cos(ang))[:, None, None] * (K @ K)   # Rodrigues
    for name, idx in special_poses(k).items():
        R[idx] = {"mirror": np.diag([-1.0, 1.0, 1.0]), "stretch": np.diag([1.5, 0.25, 1.0]), "zero": np.zeros((3, 3))}[name]
    cen = np.asarray(centres, np.float64)
    t = rng.uniform(-0.02, 0.02, (k, 3)) + cen - np.einsum("kij,kj->ki", R, cen)
    return np.ascontiguousarray(np.concatenate([R, t[:, :, None]], axis=2), F32)


def special_poses(nobj):
    """Object indices with a special matrix, the first and the last object among them (nobj >= 8)."""
    return {"mirror": [0, nobj // 3], "stretch": [1, nobj - 1], "zero": [2, nobj // 2, nobj - 2]}


# ---- the Morton order, restated ---------------------------------------------------------------------------------------
def spread3_np(v):
    """10 bits -> every third bit (rt_tile_sort.hip spread3), on uint32 arrays."""
    v = v.astype(np.uint32) & np.uint32(1023)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def morton_cells_np(v4):
    """(small [n] bool, q [n,3] uint32): which triangles get a Morton code, and their cell numbers, in the float32
    operations of tiled_order(.., morton=true) (numpy float32 arithmetic does not contract)."""
    V = np.ascontiguousarray(v4, F32).reshape(-1, 3, 4)[:, :, :3]
    lo, hi = V.reshape(-1, 3).min(axis=0), V.reshape(-1, 3).max(axis=0)
    ext = max(F32(0.0), (hi - lo).max())
    inv = F32(1023.0) / ext if ext > 0 else F32(0.0)
    tl, th = V.min(axis=1), V.max(axis=1)
    te = (th - tl).max(axis=1)
    small = ~(te > F32(0.25) * ext)
    f = (F32(0.5) * (tl + th) - lo) * inv
    assert f.dtype == F32
    q = np.zeros(f.shape, np.uint32)
    inside = (f >= 0) & (f < 1023)
    q[inside] = f[inside].astype(np.uint32)          # (unsigned int)f truncates
    q[f >= 1023] = 1023
    return small, q


def morton_keys_np(v4):
    small, q = morton_cells_np(v4)
    code = np.uint32(0x40000000) | spread3_np(q[:, 0]) | (spread3_np(q[:, 1]) << np.uint32(1)) | (spread3_np(q[:, 2]) << np.uint32(2))
    return np.where(small, code, np.uint32(0)).astype(np.uint32)


def morton_order_np(v4):
    """orig[j] = original index of the triangle at tiled position j: large triangles (key 0) first, then Morton order of
    the centres, equal keys in index order."""
    return np.argsort(morton_keys_np(v4), kind="stable").astype(np.int32)


# ---- the tiles' data on a sample of tiles -----------------------------------------------------------------------------
def sample_tiles(keys_sorted, seed=1, k=16):
    """At most k + 3 tile numbers: a seeded sample, always with the first tile, the last (ragged) tile and the first tile
    that holds no large triangle (keys_sorted = the keys in tiled order)."""
    n = len(keys_sorted)
    ntiles = (n + 63) // 64
    nlarge = int((np.asarray(keys_sorted) == 0).sum())
    pick = {0, ntiles - 1, min((nlarge + 63) // 64, ntiles - 1)}
    rng = np.random.default_rng(seed)
    pick |= set(rng.integers(0, ntiles, min(k, ntiles)).tolist())
    return sorted(pick)


def tile_rows_np(tile_data_np, v4, orig, tiles):
    """tile_data_np (tests/test_gpu_scene_update.py: the host's per-tile formulas in float64 numpy) for the tiles named."""
    V = np.ascontiguousarray(v4, F32).reshape(-1, 3, 4)
    rows = []
    for t in tiles:
        idx = np.asarray(orig[64 * t:64 * t + 64], np.int64)
        rows.append(tile_data_np(V[idx].reshape(-1, 4), np.arange(len(idx)))[0])
    return np.stack(rows)
