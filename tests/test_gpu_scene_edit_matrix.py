"""-m gpu: the scene-edit entries side by side.  Every entry (rt_update_scene, rt_replace_scene, rt_pose_objects and their
_device forms) with every tile flag its Python wrapper takes (none, RT_UPDATE_REORDER, RT_UPDATE_DEVICE_TILES) edits a live
context; a 64x64 frame and a batch of closest-hit queries must then have the bits of a context created fresh with the
resulting scene.  Where the edit makes the tiles again (sorted on the host, or built on the device in Morton order) the
tile data must be the fresh context's too; where it only refits them the tiling legitimately differs.

Two sizes reach every branch: 129 triangles are three tiles (the mesh kernel with a tiled copy, no masks), 1089 are 18
tiles (above 16 * 64: tile masks, the world grid and the second stream).  A replace starts from the other size, so the
capacity grows in one case and stays in the other."""
import numpy as np
import pytest

import test_gpu_scene_pose as sp
import test_gpu_scene_replace as sr
from test_gpu_scene_replace import mesh2346, probes      # noqa: F401 (fixtures)
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

NONE, REORDER, DEVICE_TILES = 0, abi.RT_UPDATE_REORDER, abi.RT_UPDATE_DEVICE_TILES
HOST_SORT, DEVICE_BUILD, REFIT = "host sort", "device build", "refit"
SIZES = (129, 1089)

# entry -> {tile flag: what include/uob_rt.h says happens to the tiles}; only the flags the wrapper exposes
MATRIX = {
    "update_host": {NONE: REFIT, REORDER: HOST_SORT, DEVICE_TILES: DEVICE_BUILD},
    "update_device": {NONE: REFIT, REORDER: HOST_SORT, DEVICE_TILES: DEVICE_BUILD},
    "replace_host": {NONE: HOST_SORT, DEVICE_TILES: DEVICE_BUILD},            # replace_scene(device_tiles=)
    "replace_device": {NONE: DEVICE_BUILD, REORDER: HOST_SORT},               # replace_scene_device(reorder=)
    "pose_host": {NONE: REFIT, REORDER: HOST_SORT, DEVICE_TILES: DEVICE_BUILD},
    "pose_device": {NONE: REFIT, REORDER: HOST_SORT, DEVICE_TILES: DEVICE_BUILD},
}
CASES = [(e, f, n) for e in MATRIX for f in MATRIX[e] for n in SIZES]
FLAG_NAME = {NONE: "plain", REORDER: "reorder", DEVICE_TILES: "device_tiles"}


@pytest.fixture(scope="module")
def pool(mesh2346):
    return mesh2346


def _edit(tr, entry, flags, ranges, xf, result):
    """Apply the edit that leaves `result` in the context; device entries on a stream of their own."""
    import torch
    kw = sp.FLAG_KW[flags]
    stream = torch.cuda.Stream()
    if entry == "update_host":
        tr.update_scene(result, **kw)
    elif entry == "update_device":
        dv, dn, dc = sr._to_device(result)
        torch.cuda.synchronize()
        tr.update_scene_device(dv.data_ptr(), dn.data_ptr(), dc.data_ptr(), len(result), stream=stream.cuda_stream, **kw)
    elif entry == "replace_host":
        tr.replace_scene(result, **kw)
    elif entry == "replace_device":
        dv, dn, dc = sr._to_device(result)
        torch.cuda.synchronize()
        tr.replace_scene_device(dv, dn, dc, stream=stream, **kw)
    else:
        tr.set_objects(ranges)
        if entry == "pose_host":
            tr.pose_objects(xf, **kw)
        else:
            d_xf = torch.from_numpy(xf).cuda()
            torch.cuda.synchronize()
            tr.pose_objects_device(d_xf, stream=stream, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry,flags,n", CASES, ids=["%s-%s-%d" % (e, FLAG_NAME[f], n) for e, f, n in CASES])
def test_edit_gives_the_fresh_contexts_bits(entry, flags, n, pool, probes):
    cfg = sr._cfg()
    rest = sr.scene_of(pool, n)
    ranges, xf = sp._layouts(rest, n - 26)[1]              # two objects: inside one tile, and up to triangle n - 1
    result = rest.posed(ranges, xf)
    assert not np.array_equal(result.aos, rest.aos)
    start = sr.scene_of(pool, SIZES[1 - SIZES.index(n)]) if entry.startswith("replace") else rest
    tr = rt.RayTracer(cfg, start)
    sr._frame(tr, cfg)                                     # live: a previous frame and its scheduling state
    _edit(tr, entry, flags, ranges, xf, result)
    assert tr.n_triangles == n
    tiling = MATRIX[entry][flags]
    fresh = sr._fresh_morton(cfg, result) if tiling == DEVICE_BUILD else rt.RayTracer(cfg, result)
    try:
        assert sr._same_frame(sr._frame(tr, cfg), sr._frame(fresh, cfg))
        (tri, hit), (f_tri, f_hit) = tr.query_closest_hit(probes[0]), fresh.query_closest_hit(probes[0])
        assert np.array_equal(tri, f_tri) and np.array_equal(sr._bits(hit), sr._bits(f_hit))
        assert (tri >= 0).any()
        if tiling != REFIT:
            (orig, tiles), (f_orig, f_tiles) = tr.tile_data(), fresh.tile_data()
            assert np.array_equal(orig, f_orig)
            assert sr._same_tiles(tiles, f_tiles)
    finally:
        fresh.close()
        tr.close()
