"""-m gpu: which kernel renders a frame (the table at its head).

A frame that goes to a slower kernel, or to another instantiation of the wave kernel, is bit-identical to the one it should
have been: no other test sees it.  What does show the path is what each path leaves behind, so one fresh context per row
(made under UOB_RT_TIMELINE=1) renders one frame, and then
  T  wave_timeline() answers — the wave kernel rendered it — and counts the frame's jobs, which is its job size;
  S  wave_seeds() holds a table — the (4x2 AA, 64 samples) instantiation with 64-pixel jobs, and the pre-pass in front;
  B  block_costs() answers — the mesh kernel rendered it;
  X  count_executed() answers, or fails with RT_E_UNSUPPORTED: the wave and mesh frames that have a counting build.
Neither T nor B: the thread-per-pixel kernel.

Frames of 128x8 pixels where a seed is in question (two 64-pixel jobs per row), 64x48 elsewhere; the mesh is the box and a
sphere of 416 triangles.  The job counts are the ones the commit before the family and the wave variant were stated once
reported, row by row; the rest of the table was read from that commit's code and agreed with its run.
"""
import numpy as np
import pytest

import wave_masks_util as wm
from uob_raytracer_amd import abi, meshgen, runtime as rt

pytestmark = pytest.mark.gpu

STRIP = dict(width=128, height=8)
SMALL = dict(width=64, height=48)
HEAD = dict(STRIP, aa_x=4, aa_y=2, shadow_samples=64)
JT8 = {"UOB_RT_JOB_TASKS": "8"}
UNSUPPORTED = "unsupported"

# id -> (scene, config, knobs, flags, T: jobs of the frame or None, S, B, X)
ROWS = {
    "box_4x2_64_jt8": ("box", HEAD, JT8, 0, 16, True, False, "ok"),
    "box_4x2_64_jt8_no_cull": ("box", HEAD, JT8, abi.RT_FLAG_NO_CULL, 16, False, False, "ok"),
    "box_4x2_64_jt8_no_specialise": ("box", HEAD, dict(JT8, UOB_RT_NO_SPECIALISE="1"), 0, 16, False, False, "ok"),
    "box_4x2_64_jt8_no_seed": ("box", HEAD, dict(JT8, UOB_RT_NO_SEED="1"), 0, 16, False, False, "ok"),
    "box_4x2_64_short_jobs": ("box", HEAD, {}, 0, 64, False, False, "ok"),
    "box34_4x2_64_jt8": ("box34", HEAD, JT8, 0, 16, False, False, "ok"),
    "box_2x2_16": ("box", dict(SMALL, aa_x=2, aa_y=2, shadow_samples=16), {}, 0, 192, False, False, "ok"),
    "box_96_samples": ("box", dict(SMALL, aa_x=4, aa_y=2, shadow_samples=96), {}, 0, 192, False, False, UNSUPPORTED),
    "box_9x9_16": ("box", dict(SMALL, aa_x=9, aa_y=9, shadow_samples=16), {}, 0, 192, False, False, UNSUPPORTED),
    "box_9x9_16_no_cull": ("box", dict(SMALL, aa_x=9, aa_y=9, shadow_samples=16), {}, abi.RT_FLAG_NO_CULL, None, False, False, UNSUPPORTED),
    "box_9x9_96": ("box", dict(SMALL, aa_x=9, aa_y=9, shadow_samples=96), {}, 0, None, False, False, UNSUPPORTED),
    "box_generic_flag": ("box", HEAD, JT8, abi.RT_FLAG_GENERIC_KERNEL, None, False, False, UNSUPPORTED),
    "box_all_glass": ("glass", HEAD, JT8, 0, None, False, False, UNSUPPORTED),
    "empty_scene": ("empty", HEAD, JT8, 0, None, False, False, UNSUPPORTED),
    "mesh": ("mesh", dict(SMALL, aa_x=2, aa_y=2, shadow_samples=16), {}, 0, None, False, True, "ok"),
    "mesh_no_tile_bins": ("mesh", dict(SMALL, aa_x=2, aa_y=2, shadow_samples=16), {}, abi.RT_FLAG_NO_TILE_BINS, None, False, True, "ok"),
    "mesh_96_samples": ("mesh", dict(SMALL, aa_x=2, aa_y=2, shadow_samples=96), {}, 0, None, False, True, "ok"),
    "mesh_no_cull": ("mesh", dict(SMALL, aa_x=2, aa_y=2, shadow_samples=16), {}, abi.RT_FLAG_NO_CULL, None, False, False, UNSUPPORTED),
    "mesh_generic_flag": ("mesh", dict(SMALL, aa_x=2, aa_y=2, shadow_samples=16), {}, abi.RT_FLAG_GENERIC_KERNEL, None, False, False, UNSUPPORTED),
    "mesh_9x9": ("mesh", dict(SMALL, aa_x=9, aa_y=9, shadow_samples=16), {}, 0, None, False, False, UNSUPPORTED),
}


@pytest.fixture(scope="module")
def scenes(scene, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("frame_path") / "sphere.obj")
    assert meshgen.write_sphere_obj(path, 15, 14) + len(scene) == 416
    glass = scene.with_color(range(len(scene)), (1.0, 1.0, 1.0, -1.0))       # glass casts no shadow: n_shadow == 0
    return {"box": scene, "box34": wm.box34(scene), "glass": glass, "empty": rt.Scene(np.zeros((0, 5, 4), np.float32)),
            "mesh": scene + rt.Scene.load_obj(path)}


def _answers(call):
    """-> (the call's result or None, the error code or 0)"""
    try:
        return call(), 0
    except rt.RtError as e:
        return None, e.code


@pytest.mark.parametrize("row", list(ROWS))
def test_the_path_of_a_frame(row, scenes):
    which, kw, knobs, flags, jobs, seeded, blocks, counted = ROWS[row]
    tr = wm.context(kw, dict(knobs, UOB_RT_TIMELINE="1"), scenes[which], flags)
    try:
        rot = rt.rotation_matrix(0.0, 0.0)
        focal = 1100.0 * kw["width"] / 1024.0 * kw["aa_x"]
        tr.render(rot, wm.DEFAULT_CAM, wm.DEFAULT_LIGHT, focal)
        timeline, t_err = _answers(tr.wave_timeline)
        seeds = tr.wave_seeds()
        costs, b_err = _answers(tr.block_costs)
        _, x_err = _answers(lambda: tr.count_executed(rot, wm.DEFAULT_CAM, wm.DEFAULT_LIGHT, focal))
    finally:
        tr.close()
    got = (timeline["jobs"] if timeline else None, seeds["tile_rows"] > 0, costs is not None,
           {0: "ok", abi.RT_E_UNSUPPORTED: UNSUPPORTED}.get(x_err, x_err))
    print("%s: jobs %s, seeded %s, block costs %s, count_executed %s" % ((row,) + got))
    assert t_err in (0, abi.RT_E_UNSUPPORTED) and b_err in (0, abi.RT_E_UNSUPPORTED)
    assert got == (jobs, seeded, blocks, counted)
