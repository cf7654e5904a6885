"""-m gpu: every frame of a context writes every pixel exactly once.

What decides which wave renders which pixels of which frame — the wave kernel's queue heads, its list of last frame's
expensive jobs (phase A), the flags by which the plain sequence skips a listed job, the two lists and flag arrays that swap
by generation, the roll-back of a flag when the list is full, the row neighbours listed with a job; the row and band
arithmetic of all three kernel families — is pinned here in three ways the other tests cannot see:

* frames go into device tensors the test has poisoned (frame_coverage_util.render_checked): a pixel no job wrote keeps
  the poison, on a context's first frame and on a static view alike;
* the view CHANGES between the frames of a context, so that a job dropped in one frame shows the previous view's pixels;
* UOB_RT_TIMELINE's job count must equal the frame's job count exactly: each job once, none dropped, none rendered twice.

UOB_RT_JOB_TASKS, UOB_RT_HEAVY_FACTOR4 and UOB_RT_HEAVY_DILATE (read once, in rt_init) turn the list on at frames of a few
thousand pixels; without them launch_frame uses it only from 4-task jobs on, which fill_params grants to frames of ~82 000
jobs.  Expected bits come from a fresh context on the thread-per-pixel kernel and from the CPU oracle."""
import numpy as np
import pytest

import frame_coverage_util as fc
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

_REF = {}          # (what, config key, scene key, view index) -> (argb, tap): computed once, shared, never changed


def _key(kw):
    return tuple(sorted(kw.items()))


def _generic(kw, scene, scene_key, vi, view, focal_of):
    """The frame of a fresh context on the thread-per-pixel kernel, no knobs (ARGB, tap)"""
    k = ("generic", _key(kw), scene_key, vi, focal_of.__name__)
    if k not in _REF:
        cfg = abi.make_config(flags=abi.RT_FLAG_GENERIC_KERNEL, **kw)
        tr = rt.RayTracer(cfg, scene)
        yaw, pitch, cam, light = view
        _REF[k] = fc.render_checked(tr, rt.rotation_matrix(yaw, pitch), cam, light, focal_of(cfg))
        tr.close()
    return _REF[k]


def _oracle(oracle, kw, scene, scene_key, vi, view, focal_of):
    k = ("oracle", _key(kw), scene_key, vi, focal_of.__name__)
    if k not in _REF:
        cfg = abi.make_config(**kw)
        _REF[k] = fc.oracle_frame(oracle, cfg, scene, view, focal_of(cfg))
    return _REF[k]


# ---- sequences with the list on (wave kernel) ----------------------------------------------------------------------------------
HEADLINE = dict(width=256, height=96, aa_x=4, aa_y=2, shadow_samples=64, light_spread=fc.SEQ_SPREAD)
RAGGED = dict(width=250, height=37, aa_x=4, aa_y=2, shadow_samples=64, light_spread=fc.SEQ_SPREAD)
# case -> (config, knobs, forced job size in tasks, what the list must do)
#   "some":  a frame after the first starts from a non-empty list
#   "full":  the list a frame starts from holds njobs // 3 entries, its cap, from the third frame on
#   "empty": the machinery runs, the list stays empty
SEQUENCES = {
    # the headline instantiation, 64-pixel jobs, nseg 4
    "a": (HEADLINE, {"UOB_RT_JOB_TASKS": "8"}, 8, "some"),
    # the unspecialised instantiation
    "b": (HEADLINE, {"UOB_RT_JOB_TASKS": "8", "UOB_RT_NO_SPECIALISE": "1"}, 8, "some"),
    # ragged last job, odd row count; threshold a quarter of the mean: the list fills, the only way in to the list-full roll-back
    "c": (RAGGED, {"UOB_RT_JOB_TASKS": "4", "UOB_RT_HEAVY_FACTOR4": "1"}, 4, "full"),
    # the reference's constants
    "d": (dict(width=200, height=50, aa_x=2, aa_y=2, shadow_samples=10, light_spread=fc.SEQ_SPREAD),
          {"UOB_RT_JOB_TASKS": "4", "UOB_RT_HEAVY_FACTOR4": "1"}, 4, "full"),
    # 35-pixel jobs; the aa_magic / shfl path of aa_sum
    "e": (dict(width=100, height=40, aa_x=3, aa_y=3, shadow_samples=5, light_spread=fc.SEQ_SPREAD),
          {"UOB_RT_JOB_TASKS": "5", "UOB_RT_HEAVY_FACTOR4": "2"}, 5, "some"),
    # chunked grid (81 AA samples): the list is on without the job knob
    "f": (dict(width=83, height=40, aa_x=9, aa_y=9, shadow_samples=16, light_spread=fc.SEQ_SPREAD),
          {"UOB_RT_HEAVY_FACTOR4": "1"}, None, "full"),
    # band row mapping under phase A
    "g": (dict(HEADLINE, band_rows=8, band_index=1, band_count=3), {"UOB_RT_JOB_TASKS": "8"}, 8, "some"),
    # state machinery on, list empty
    "h": (HEADLINE, {"UOB_RT_JOB_TASKS": "8", "UOB_RT_HEAVY_FACTOR4": "4096"}, 8, "empty"),
    # nseg 1 and 2: a listed job has no left or right neighbour in its row; with and without the neighbours
    "i-60-dilate0": (dict(HEADLINE, width=60, height=24), {"UOB_RT_JOB_TASKS": "8", "UOB_RT_HEAVY_FACTOR4": "1", "UOB_RT_HEAVY_DILATE": "0"}, 8, "full"),
    "i-60-dilate1": (dict(HEADLINE, width=60, height=24), {"UOB_RT_JOB_TASKS": "8", "UOB_RT_HEAVY_FACTOR4": "1", "UOB_RT_HEAVY_DILATE": "1"}, 8, "full"),
    "i-128-dilate0": (dict(HEADLINE, width=128, height=24), {"UOB_RT_JOB_TASKS": "8", "UOB_RT_HEAVY_FACTOR4": "1", "UOB_RT_HEAVY_DILATE": "0"}, 8, "full"),
    "i-128-dilate1": (dict(HEADLINE, width=128, height=24), {"UOB_RT_JOB_TASKS": "8", "UOB_RT_HEAVY_FACTOR4": "1", "UOB_RT_HEAVY_DILATE": "1"}, 8, "full"),
}


def _knobbed_context(cfg, scene, knobs, monkeypatch):
    """A context created under the knobs and UOB_RT_TIMELINE=1; rt_init reads them once, so they are gone right after"""
    env = dict(knobs, UOB_RT_TIMELINE="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return rt.RayTracer(cfg, scene)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _checked_frame(tr, kw, scene, scene_key, vi, oracle, what, oracle_too):
    """Frame `what` of view vi: every pixel written, the bits of a fresh generic context, on view 1 also the oracle's, and
    half of the pixels on the scene"""
    view = fc.SEQ_VIEWS[vi]
    want_argb, want_tap = _generic(kw, scene, scene_key, vi, view, fc.seq_focal)
    yaw, pitch, cam, light = view
    argb, tap = fc.render_checked(tr, rt.rotation_matrix(yaw, pitch), cam, light, fc.seq_focal(tr.cfg), expected_tap=want_tap)
    fc.same_frame(argb, tap, want_argb, want_tap, what + " against the generic kernel")
    if oracle_too:
        o_argb, o_rgb = _oracle(oracle, kw, scene, scene_key, vi, view, fc.seq_focal)
        fc.same_frame(argb, tap, o_argb, o_rgb, what + " against the CPU oracle")
    share = (argb != fc.BACKGROUND).mean()
    assert share >= 0.5, "%s: only %.0f %% of the pixels are on the scene" % (what, 100 * share)
    return argb


@pytest.mark.parametrize("case", sorted(SEQUENCES))
def test_changing_views_with_the_list_on(case, scene, oracle, monkeypatch, capsys):
    """One context, the views V0 V0 V1 V2 V0 V1 (frame_coverage_util.SEQ_VIEWS): every frame holds no poison, equals a fresh
    generic context's frame (on V1 also the CPU oracle's, whole frame), renders exactly expected_jobs jobs and starts from a
    list of at most njobs // 3.

    The list a frame starts from (wave_timeline's listed_jobs) is built by the frame before, against the mean cost of the frame
    before that: a context's first frame has no mean and lists nothing, its second frame starts from that empty list and
    builds the first one, so the third frame is the first that can start from a full list.  "full" cases assert 0, 0, cap,
    cap, cap, cap.  In case c more than half of the 296 jobs cost over a quarter of the mean (half the pixels are on the
    scene, the background is what is cheap), so the list reaches its cap of 98 while listable jobs remain: the
    `else atomicExch` branch is the only way the kernel can then go.  Whether it ran cannot be seen from outside; this
    asserts the visible half."""
    kw, knobs, jt, mode = SEQUENCES[case]
    cfg = abi.make_config(**kw)
    njobs = fc.expected_jobs(cfg, jt)
    tr = _knobbed_context(cfg, scene, knobs, monkeypatch)
    listed = []
    for k, vi in enumerate(fc.SEQ_ORDER):
        what = "case %s, frame %d (view %d)" % (case, k, vi)
        _checked_frame(tr, kw, scene, "box", vi, oracle, what, vi == 1)
        t = tr.wave_timeline()
        listed.append(t["listed_jobs"])
        assert t["jobs"] == njobs, "%s: %d jobs rendered, the frame has %d" % (what, t["jobs"], njobs)
        assert t["listed_jobs"] <= njobs // 3, "%s: a list of %d for %d jobs" % (what, t["listed_jobs"], njobs)
    tr.close()
    with capsys.disabled():
        print("\n[frame coverage] case %s: %d jobs, listed_jobs per frame %s" % (case, njobs, listed))
    if mode == "some":
        assert any(listed[1:]), "did not exercise the list: %s" % listed
    elif mode == "full":
        assert listed == [0, 0] + [njobs // 3] * (len(fc.SEQ_ORDER) - 2), "the list did not reach its cap: %s of %d" % (listed, njobs // 3)
    else:
        assert not any(listed), "the list was meant to stay empty: %s" % listed


def test_the_list_across_scene_edits(scene, oracle, monkeypatch, tmp_path, capsys):
    """Case c's context through scene edits.  A replace that stays within 64 triangles (one wall turned into a mirror) keeps
    the list, its generation and the cost mean: the next frame starts from a full list made for another scene.  A replace
    to box + 44 triangles (n = 70, the mesh kernel) and back restarts the wave kernel's scheduling state, as rt_scene.hip
    scene_switch says: the frame after coming back is a first frame again (0, 0, then the cap).  Every frame against a fresh
    context of the scene it shows; the timeline is asserted on the wave-kernel frames."""
    kw, knobs, jt, _ = SEQUENCES["c"]
    cfg = abi.make_config(**kw)
    njobs, cap = fc.expected_jobs(cfg, jt), fc.expected_jobs(cfg, jt) // 3
    mirror = scene.with_color([8, 9], (1.0, 1.0, 1.0, 0.0))
    mesh = fc.mesh_scene(tmp_path)
    scenes = {"box": scene, "mirror": mirror, "mesh70": mesh}
    # (scene, view, listed_jobs the frame must start from; None: not a wave-kernel frame)
    plan = [("box", 0, 0), ("box", 0, 0), ("box", 1, cap), ("mirror", 2, cap), ("mirror", 0, cap), ("box", 1, cap),
            ("mesh70", 2, None), ("mesh70", 0, None), ("box", 0, 0), ("box", 1, 0), ("box", 2, cap), ("box", 0, cap)]
    tr = _knobbed_context(cfg, scene, knobs, monkeypatch)
    now, listed = "box", []
    for k, (name, vi, want_listed) in enumerate(plan):
        if name != now:
            tr.replace_scene(scenes[name])
            now = name
        what = "frame %d (%s, view %d)" % (k, name, vi)
        _checked_frame(tr, kw, scenes[name], name, vi, oracle, what, vi == 1)
        if want_listed is None:
            listed.append(None)
            continue
        t = tr.wave_timeline()
        listed.append(t["listed_jobs"])
        assert t["jobs"] == njobs, "%s: %d jobs rendered, the frame has %d" % (what, t["jobs"], njobs)
    tr.close()
    with capsys.disabled():
        print("\n[frame coverage] scene edits: %d jobs, listed_jobs per frame %s" % (njobs, listed))
    assert listed == [p[2] for p in plan]


def test_several_devices_store_by_global_row(scene, oracle, monkeypatch):
    """Case k: a parent of two children on device 0 with bands of 16 rows, 64-pixel jobs and the list on in each child; the
    parent's render_device into a poisoned frame, the changing views, against the fresh generic context and the oracle."""
    kw = dict(HEADLINE)
    cfg = abi.make_config(devices=(0, 0), device_band_rows=16, **kw)
    tr = _knobbed_context(cfg, scene, {"UOB_RT_JOB_TASKS": "8"}, monkeypatch)
    for k, vi in enumerate(fc.SEQ_ORDER):
        _checked_frame(tr, kw, scene, "box", vi, oracle, "two children, frame %d (view %d)" % (k, vi), vi == 1)
    tr.close()


# ---- queue and frame-shape edges ---------------------------------------------------------------------------------------------
GRIDS = {"1x1": (1, 1, 1), "2x2": (2, 2, 10), "4x2": (4, 2, 64), "3x3": (3, 3, 5), "8x8": (8, 8, 3), "9x8": (9, 8, 16)}
# 27 of the 72 pairs: every shape at least twice, every grid at least four times; 1x1, 16x1 (one job) and 496x1 (31 sixteen-
# pixel jobs, one per queue head) meet 1x1 AA, 4x2 and 9x8; 512x1 is 32 jobs
PAIRS = [
    ((1, 1), "1x1"), ((1, 1), "4x2"), ((1, 1), "9x8"), ((16, 1), "1x1"), ((16, 1), "4x2"), ((16, 1), "9x8"),
    ((496, 1), "1x1"), ((496, 1), "4x2"), ((496, 1), "9x8"), ((1, 7), "2x2"), ((1, 7), "3x3"), ((7, 1), "8x8"), ((7, 1), "2x2"),
    ((15, 2), "3x3"), ((15, 2), "4x2"), ((17, 3), "8x8"), ((17, 3), "1x1"), ((63, 2), "2x2"), ((63, 2), "9x8"),
    ((64, 1), "3x3"), ((64, 1), "8x8"), ((65, 2), "4x2"), ((65, 2), "2x2"), ((33, 31), "3x3"), ((33, 31), "8x8"),
    ((512, 1), "2x2"), ((512, 1), "1x1"),
]
# path -> (flags, scene): the wave kernel, the same testing every triangle, the thread-per-pixel kernel, the mesh kernel
PATHS = {"default": (0, "box"), "nocull": (abi.RT_FLAG_NO_CULL, "box"), "generic": (abi.RT_FLAG_GENERIC_KERNEL, "box"),
         "mesh": (0, "mesh70")}


def _edge_cases():
    for (w, h), grid in PAIRS:
        for path in PATHS:
            if grid == "9x8" and path == "nocull":       # more than 64 AA samples: the wave kernel exists with the cull only
                continue
            yield pytest.param(w, h, grid, path, id="%dx%d-%s-%s" % (w, h, grid, path))


@pytest.fixture(scope="module")
def scenes(scene, tmp_path_factory):
    return {"box": scene, "mesh70": fc.mesh_scene(tmp_path_factory.mktemp("coverage"))}


def _grid_kw(w, h, grid, **extra):
    ax, ay, s = GRIDS[grid]
    return dict(width=w, height=h, aa_x=ax, aa_y=ay, shadow_samples=s, **extra)


@pytest.mark.parametrize("w,h,grid,path", list(_edge_cases()))
def test_edge_shapes_against_the_oracle(w, h, grid, path, scenes, oracle):
    """Frames of fewer jobs than queue heads, narrower than a job, of one row; two frames of one context on two views, whole
    frame against the CPU oracle, ARGB and tap; from 16 pixels on a quarter of the pixels is on the scene."""
    flags, scene_key = PATHS[path]
    kw = _grid_kw(w, h, grid)
    tr = rt.RayTracer(abi.make_config(flags=flags, **kw), scenes[scene_key])
    for vi, view in enumerate(fc.EDGE_VIEWS):
        o_argb, o_rgb = _oracle(oracle, kw, scenes[scene_key], scene_key, vi, view, fc.edge_focal)
        if w * h >= 16:
            assert (o_argb != fc.BACKGROUND).mean() >= 0.25
        yaw, pitch, cam, light = view
        argb, tap = fc.render_checked(tr, rt.rotation_matrix(yaw, pitch), cam, light, fc.edge_focal(tr.cfg), expected_tap=o_rgb)
        fc.same_frame(argb, tap, o_argb, o_rgb, "%dx%d %s %s, view %d" % (w, h, grid, path, vi))
    tr.close()


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("w,h,grid", [(33, 31, "2x2"), (33, 5, "4x2")])
def test_bands_of_one_row_assemble_the_frame(w, h, grid, path, scenes, oracle):
    """band_rows = 1, band_count = 7, every index: each rank's rows through the poisoned tensors, assembled, equal the unbanded
    frame of the oracle.  On the 5-row frame the ranks 5 and 6 own no row: the call succeeds and writes nothing."""
    flags, scene_key = PATHS[path]
    kw = _grid_kw(w, h, grid)
    for vi, view in enumerate(fc.EDGE_VIEWS):
        o_argb, o_rgb = _oracle(oracle, kw, scenes[scene_key], scene_key, vi, view, fc.edge_focal)
        frame = np.full((h, w), fc.SENTINEL, np.uint32)
        taps = np.full((h, w, 4), np.nan, np.float32)
        yaw, pitch, cam, light = view
        for index in range(7):
            cfg = abi.make_config(flags=flags, band_rows=1, band_index=index, band_count=7, **kw)
            rows = fc.owned_rows(cfg)
            tr = rt.RayTracer(cfg, scenes[scene_key])
            assert tr.rows == len(rows) and bool(rows) != (h == 5 and index >= 5)
            argb, tap = fc.render_checked(tr, rt.rotation_matrix(yaw, pitch), cam, light, fc.edge_focal(cfg))
            tr.close()
            assert argb.shape == (len(rows), w)
            frame[rows], taps[rows] = argb, tap
        fc.check_written(frame, taps, o_rgb)
        fc.same_frame(frame, taps, o_argb, o_rgb, "%dx%d %s %s in 7 bands, view %d" % (w, h, grid, path, vi))


# ---- the limits of validate_config (32767 per side, 2^24 pixels) --------------------------------------------------------
LIMITS = [
    pytest.param(32767, 512, "1x1", "default", id="32767x512-default"),
    pytest.param(32767, 512, "1x1", "mesh", id="32767x512-mesh"),
    pytest.param(512, 32767, "1x1", "default", id="512x32767-default"),
    pytest.param(512, 32767, "1x1", "mesh", id="512x32767-mesh"),
    pytest.param(32767, 2, "4x2", "default", id="32767x2-4x2"),
    pytest.param(3, 32767, "2x2", "default", id="3x32767-2x2"),
    pytest.param(32000, 524, "1x1", "default", id="32000x524-nseg500"),       # nseg 500: div_magic with a real error term
]


@pytest.mark.parametrize("w,h,grid,path", LIMITS)
def test_frames_at_the_size_limits(w, h, grid, path, scenes, oracle):
    """One frame, ARGB only, no tap tensor, compared on the device: no poison left, the path's frame equals the thread-per-
    pixel kernel's over the whole frame, both equal the CPU oracle on 3000 seeded pixels, 5 % of the pixels on the scene.
    The focal length follows the LONG side, so that the strip crosses the room."""
    import torch
    flags, scene_key = PATHS[path]
    kw = _grid_kw(w, h, grid)
    yaw, pitch, cam, light = fc.LIMIT_VIEW
    rot = rt.rotation_matrix(yaw, pitch)
    frames = {}
    for name, f in (("generic", abi.RT_FLAG_GENERIC_KERNEL), (path, flags)):
        cfg = abi.make_config(flags=f, **kw)
        tr = rt.RayTracer(cfg, scenes[scene_key])
        frames[name], _ = fc.render_checked(tr, rot, cam, light, fc.long_side_focal(cfg), want_tap=False, to_host=False)
        tr.close()
    differ = frames[path] != frames["generic"]
    ndiff = int(differ.sum())
    assert ndiff == 0, "%d pixels differ from the generic kernel, first at (row, x) = %s" % (ndiff, differ.nonzero()[0].tolist())
    share = float((frames[path] != fc.BACKGROUND - (1 << 32)).float().mean())        # (the tensors are int32)
    assert share >= 0.05, "only %.1f %% of the pixels are on the scene" % (100 * share)
    pix = np.sort(np.random.default_rng(w * 7 + h).choice(w * h, 3000, replace=False)).astype(np.int32)
    cfg = abi.make_config(**kw)
    want, _ = fc.oracle_frame(oracle, cfg, scenes[scene_key], fc.LIMIT_VIEW, fc.long_side_focal(cfg), pix=pix)
    at = torch.from_numpy(pix.astype(np.int64)).to(frames[path].device)
    got = frames["generic"].reshape(-1)[at].cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of 3000 pixels differ from the oracle, first pixel id %d" % (bad.size, pix[bad[0]])
