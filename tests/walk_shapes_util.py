"""The inputs of tests/test_gpu_walk_shapes.py, shared with tools/walk_counters.py (which records the work counters of
the same inputs into tests/golden/walk_counters.json): the box plus a bumpy sphere cut to an exact triangle count, a
40 x 40 frame, and the passes and calls whose counters are kept."""
import os

import numpy as np

import aov_util
from uob_raytracer_amd import abi, meshgen, runtime as rt

CAM, LIGHT = [0.0, 0.0, -3.2], [0.0, -0.5, -0.7]
SIZE = 40          # no multiple of 8; a screen-cell edge (32) falls inside waves

# scene name -> (n_lon, n_lat, mesh triangles kept): 65 = two tiles, the second holding one triangle; 26 + 4097 = 65 tiles,
# i.e. candidate masks of two words and a walk that crosses the word boundary
SCENES = {"65": (5, 5, 39), "4123": (50, 42, 4097)}

# pass name -> (aa, sample, flags, bands): sample None = RT_AOV_ALL_SAMPLES (runs of 64 elements cross a cell edge mid-run);
# bands = (band_rows, band_index, band_count): the packed rows of band 1 of 2 jump from row 23 to row 36
PASSES = {
    "aa1_s0_bins": (1, 0, 0, None),
    "aa1_s0_nobins": (1, 0, abi.RT_FLAG_NO_TILE_BINS, None),
    "aa3_all_bins": (3, None, 0, None),
    "aa3_all_nobins": (3, None, abi.RT_FLAG_NO_TILE_BINS, None),
    "aa3_all_band1of2": (3, None, 0, (12, 1, 2)),
}
CALLS_PASS = "aa3_all_bins"      # the context and the rays (camera, the pass's direction plane) of the three calls
RADIUS_SQ = 16.0                 # of the in-shadow query: the mesh and the near walls are within reach, the back wall is not
PLANES = ("prim", "position", "normal", "albedo", "direction")


def build_scene(name, tmpdir):
    lon, lat, keep = SCENES[name]
    path = os.path.join(str(tmpdir), "walk_%s.obj" % name)
    assert meshgen.write_sphere_obj(path, lon, lat) >= keep
    sc = rt.Scene.cornell_box() + rt.Scene(rt.Scene.load_obj(path).aos[:keep])
    assert len(sc) == int(name)
    return sc


def config_of(pass_name):
    aa, _, flags, bands = PASSES[pass_name]
    kw = dict(width=SIZE, height=SIZE, aa_x=aa, aa_y=aa, flags=flags)
    if bands:
        kw.update(band_rows=bands[0], band_index=bands[1], band_count=bands[2])
    return abi.make_config(**kw)


def run_pass(sc, pass_name):
    """-> (the context, still open; the planes; aov_stats of the pass)"""
    cfg = config_of(pass_name)
    tr = rt.RayTracer(cfg, sc)
    focal = 1100.0 * SIZE / 1024.0 * cfg.aa_x
    planes = tr.render_aov(rt.rotation_matrix(0.0, 0.0), CAM, focal, sample=PASSES[pass_name][1], planes=PLANES)
    return tr, planes, tr.aov_stats()


def rays_of_pass(planes):
    return aov_util.rays_of(CAM, planes["direction"][..., :3])


def run_calls(tr, rays):
    """One closest-hit query, one in-shadow query and one radiance call on `rays` -> their counters and answers"""
    tri, out10 = tr.query_closest_hit(rays)
    closest = tr.trace_stats()
    blocked = tr.query_in_shadow(rays, np.full(rays.shape[0], RADIUS_SQ, np.float32))
    shadow = tr.trace_stats()
    rgba = tr.radiance_rays(rays, LIGHT)
    radiance = tr.radiance_stats()
    return {"closest": closest, "shadow": shadow, "radiance": radiance}, {"tri": tri, "out10": out10, "blocked": blocked, "rgba": rgba}
