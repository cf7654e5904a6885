"""-m gpu: the wide parts of the wave kernel's tile seeds (rt_kernel_wave.hip rt_wave_seed, DESIGN.md 4.1 "tile seeds").

The pre-pass keeps a primary part for any tile whose bound is finite (every triangle a primary ray of the tile can hit, and
whether a sphere may be touched) and a shadow part for any tile whose centre ray lands on a lit diffuse point (the whole
outcome of level 1 there: casters, sphere candidate, blocked), under the caps UOB_RT_SEED_KP, UOB_RT_SEED_CASTERS and
UOB_RT_SEED_SPH.  A job that starts from such a record does less work and writes the same bits.

  * the windows of tests/test_gpu_tile_seed.py (and floor_in_umbra, and a view built to reach a blocked level 1) at three
    settings of the caps — what the strict rule kept, the shipped defaults, everything — each against UOB_RT_NO_SEED=1, the
    no-cull path, the thread-per-pixel kernel and the CPU oracle, ARGB and float tap, bit for bit;
  * the raw table (RayTracer.wave_seeds_wide) against the AOV pass's primitive ids tile by tile, the strict view
    (RayTracer.wave_seeds) against check_table of the existing test, the wide counters against
    tests/golden/tile_seed_wide_counters.json (tools/record_tile_seed_wide_golden.py);
  * every new kind of record is reached; sequences of frames, two streams, a scene edit, bands, one headline-size pair.

The cap on casters counts Kh, the casters off h's plane: with 0 (and no sphere candidate, not blocked) that is the strict
rule, whose K still names h's own plane.
"""
import json
import os

import numpy as np
import pytest

import frame_coverage_util as fc
import test_gpu_tile_seed as ts
import wave_masks_util as wm
from conftest import ROOT
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu

# (UOB_RT_SEED_KP, UOB_RT_SEED_CASTERS, UOB_RT_SEED_SPH); DEFAULT: what Tuning in rt_host.h holds
PARENT, DEFAULT, OPEN = (1, 0, 0), (64, 32, 1), (64, 64, 1)
CAPS = {"parent": PARENT, "default": DEFAULT, "open": OPEN}
# A quad 0.1 over the floor under a light a tenth as wide: the camera looks under its near edge at floor whose every shadow
# ray meets the quad's near triangle a sixth of a unit inside that edge, at a fifteenth of its way to the light — one caster
# blocks every ray of a tile's direction set, by a wide margin in u, v and the distance (light_bundle_bound, all_blocked).
BLOCKED_VIEW = "floor_under_quad"
WIDE_VIEWS = ["default_view", "pulled_back", "floor_penumbra", "floor_in_umbra", "rows_across_diagonal",
              "mirror_wall_glass_sphere", "moved_by_3e4", "default_view_ball", BLOCKED_VIEW]
_REF = {}                                    # references: computed once, shared, never changed


def knobs_of(caps):
    return {} if caps is None else {"UOB_RT_SEED_KP": str(caps[0]), "UOB_RT_SEED_CASTERS": str(caps[1]), "UOB_RT_SEED_SPH": str(caps[2])}


def wide_setup(view, box):
    if view != BLOCKED_VIEW:
        return ts.seeded_setup(view, box)
    kw, knobs, s, rot, cam, light, focal = ts.seeded_setup("floor_penumbra", box)
    fy = np.float32(wm._floor_y(box))
    s = box + wm._quad(box, 0.6, 0.0, 0.1, float(fy - np.float32(0.1)))          # x in [-0.6, 0.6], z in [-0.5, 0.7]
    return dict(kw, light_spread=0.005), knobs, s, rt.rotation_matrix(0.0, -0.34), cam, light, focal


def references(view, box, oracle):
    """-> ({name: (argb, tap)}, AOV primitive ids [rows, W, aa]) of a window, none of them seeded"""
    if view not in _REF:
        kw, knobs, s, rot, cam, light, focal = wide_setup(view, box)
        tr = wm.context(kw, dict(knobs, **ts.NO_SEED), s)
        refs = {"UOB_RT_NO_SEED=1": tr.render(rot, cam, light, focal, want_rgb=True)}
        prim = tr.render_aov(rot, cam, focal, sample=None, planes=("prim",))["prim"]
        tr.close()
        refs["no cull"] = ts._render(kw, knobs, s, rot, cam, light, focal, abi.RT_FLAG_NO_CULL)[:2]
        refs["generic kernel"] = ts._render(kw, knobs, s, rot, cam, light, focal, abi.RT_FLAG_GENERIC_KERNEL)[:2]
        v, n, c = s.packed()
        refs["CPU oracle"] = oracle.render(abi.make_config(**kw), v, n, c, rot, cam, light, focal, nthreads=8)
        _REF[view] = (refs, prim)
    return _REF[view]


def wide_case(view, caps, box):
    """-> (frame, wide table, strict table, scene) of a window under the caps (None: no knob set)"""
    kw, knobs, s, rot, cam, light, focal = wide_setup(view, box)
    tr = wm.context(kw, dict(knobs, **knobs_of(caps)), s)
    frame = tr.render(rot, cam, light, focal, want_rgb=True)
    wide, strict = tr.wave_seeds_wide(), tr.wave_seeds()
    tr.close()
    return frame, wide, strict, s


def wide_counters(d):
    return {k: d[k] for k in d if k != "records"}


def _bits(x):
    return bin(int(x)).count("1")


def check_wide_table(d, prim, scene, caps):
    """Every raw record against what its tile shows.  prim: the AOV pass's primitive ids [rows, W, aa] (-1 miss, -2 sphere)"""
    kp_cap, caster_cap, keep_sph = caps
    rec, r, n = d["records"], d["rows_per_tile"], scene.aos.shape[0]
    known = rt.SEED_PRIMARY | rt.SEED_SHADOW | rt.SEED_PRIMARY_WIDE | rt.SEED_PRIMARY_SPH | rt.SEED_SHADOW_WIDE | rt.SEED_SHADOW_SPH | \
        rt.SEED_SHADOW_BLOCKED
    for tr_ in range(d["tile_rows"]):
        for col in range(d["tiles_per_row"]):
            q = rec[tr_, col]
            ids = set(np.unique(prim[tr_ * r:(tr_ + 1) * r, col * 64:(col + 1) * 64]).tolist()) - {-1}
            fl, where = int(q["flags"]), "tile (%d, %d)" % (tr_, col)
            kp, k, kh = int(q["Kp"]), int(q["K"]), int(q["Kh"])
            assert fl & ~known == 0, where
            if fl & rt.SEED_PRIMARY:
                assert fl & rt.SEED_PRIMARY_WIDE and not fl & rt.SEED_PRIMARY_SPH and _bits(kp) == 1, where
            if fl & rt.SEED_SHADOW:
                assert fl & rt.SEED_PRIMARY and fl & rt.SEED_SHADOW_WIDE and kh == 0, where
                assert not fl & (rt.SEED_SHADOW_SPH | rt.SEED_SHADOW_BLOCKED), where
            if fl & rt.SEED_PRIMARY_WIDE:
                assert _bits(kp) <= kp_cap, "%s: %d triangles in Kp, the cap is %d" % (where, _bits(kp), kp_cap)
                missing = [i for i in ids if i >= 0 and not (kp >> i) & 1]
                assert not missing, "%s shows %s, Kp is %x" % (where, sorted(ids), kp)
                if -2 in ids:
                    assert fl & rt.SEED_PRIMARY_SPH, where + " shows a sphere, its primary part has no sphere bit"
            else:
                assert kp == 0 and not fl & rt.SEED_PRIMARY_SPH, where
            if fl & rt.SEED_SHADOW_WIDE:
                h = int(q["h"])
                assert 0 <= h < n and scene.aos[h, 4, 3] > 0, "%s: h = %d is no diffuse triangle" % (where, h)
                assert h == prim[tr_ * r + r // 2, col * 64 + 32, 0], where + ": h is not what sample 0 of the centre pixel shows"
                assert kh & ~k == 0, where + ": Kh is no subset of K"
                assert np.isfinite(q["D0"]).all() and np.isfinite(q["ed"]) and q["ed"] > 0, where
                if not fl & rt.SEED_SHADOW_BLOCKED:
                    assert _bits(kh) <= caster_cap, "%s: %d casters off h's plane, the cap is %d" % (where, _bits(kh), caster_cap)
                    assert keep_sph or not fl & rt.SEED_SHADOW_SPH, where + ": a sphere candidate was kept"
            else:
                assert not fl & (rt.SEED_SHADOW_SPH | rt.SEED_SHADOW_BLOCKED), where
                assert k == 0 and kh == 0 and q["ed"] == 0, where + ": an invalid shadow part holds nothing"


def check_counters(wide, strict):
    """The wide counters against the records, and against the strict view's"""
    f = wide["records"]["flags"]
    kh = wide["records"]["Kh"]
    sh = (f & rt.SEED_SHADOW_WIDE) != 0
    assert wide["tiles_primary"] == int(((f & rt.SEED_PRIMARY_WIDE) != 0).sum()) and wide["tiles_shadow"] == int(sh.sum())
    assert wide["tiles_casters"] == int((sh & (kh != 0)).sum())
    assert wide["tiles_sphere"] == int((sh & ((f & rt.SEED_SHADOW_SPH) != 0)).sum())
    assert wide["tiles_blocked"] == int((sh & ((f & rt.SEED_SHADOW_BLOCKED) != 0)).sum())
    for k in rt.SEED_WIDE_KEYS:
        assert wide["jobs_" + k] >= wide["tiles_" + k]
    assert wide["tiles_primary"] >= strict["tiles_primary"] and wide["jobs_primary"] >= strict["jobs_primary"]
    assert wide["tiles_shadow"] >= strict["tiles_shadow"] and wide["jobs_shadow"] >= strict["jobs_shadow"]
    assert strict["tiles_primary"] == int(((f & rt.SEED_PRIMARY) != 0).sum()) and strict["tiles_shadow"] == int(((f & rt.SEED_SHADOW) != 0).sum())


# ---- 1. frames and tables of the windows ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "tile_seed_wide_counters.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("caps", sorted(CAPS))
@pytest.mark.parametrize("view", WIDE_VIEWS)
def test_window(view, caps, scene, oracle, golden, capsys):
    refs, prim = references(view, scene, oracle)
    got, wide, strict, s = wide_case(view, None if caps == "default" else CAPS[caps], scene)
    c = wide_counters(wide)
    with capsys.disabled():
        print("\n[tile seed, wide] %s, %s caps: %s; strict %s" % (view, caps, c, ts.seed_counters(strict)))
    for what, want in refs.items():
        ts._same(got, want, "%s, %s caps, against %s" % (view, caps, what))
    check_wide_table(wide, prim, s, CAPS[caps])
    ts.check_table(strict, prim, s)
    check_counters(wide, strict)
    if caps != "parent":
        if view == "rows_across_diagonal":
            assert wide["jobs_primary"] > strict["jobs_primary"], "no job started from a primary part of several triangles"
        if view == "floor_penumbra":
            assert wide["tiles_casters"] > 0 and wide["jobs_casters"] > 0, "no shadow part with casters"
        if view == "default_view_ball":
            f = wide["records"]["flags"]
            assert ((f & rt.SEED_PRIMARY_SPH) != 0).any(), "no primary part with the sphere bit under the ball's outline"
            assert wide["tiles_sphere"] > 0 and wide["jobs_sphere"] > 0, "no shadow part names a sphere candidate"
    if view == BLOCKED_VIEW:
        assert wide["tiles_blocked"] > 0 and wide["jobs_blocked"] > 0, "no blocked shadow part"       # kept whatever the caps
    assert c == golden["%s-%s" % (view, caps)]


def test_the_strict_view_does_not_depend_on_the_caps(scene):
    for view in ("rows_across_diagonal", "default_view_ball"):
        views = [wide_case(view, caps, scene)[2] for caps in (PARENT, OPEN)]
        assert ts.seed_counters(views[0]) == ts.seed_counters(views[1])
        assert views[0]["records"].tobytes() == views[1]["records"].tobytes()


def test_a_sphere_candidate_reaches_a_shadow_part(scene):
    """A diffuse ball of radius 0.1 half way between the floor point in the middle of the floor_penumbra window and the
    light (far above the window's rays, so it does not show): level 1 over the tiles in and around its shadow names a sphere
    candidate.  With UOB_RT_SEED_SPH=0 those tiles keep a shadow part only where a triangle blocks them; the frames are the
    unseeded frame either way."""
    kw, knobs, s, rot, cam, light, focal = ts.seeded_setup("floor_penumbra", scene)
    d3 = np.asarray([rot[2], rot[6], rot[10]], np.float64)               # the middle ray: the third column of the rotation
    x = np.asarray(cam, np.float64) + (wm._floor_y(scene) - cam[1]) / d3[1] * d3
    centre = (0.5 * (x + np.asarray(light, np.float64))).tolist()
    kw = dict(kw, spheres=((tuple(centre), 0.01, (0.8, 0.3, 0.2, 1.0)),))
    want = ts._render(kw, dict(knobs, **ts.NO_SEED), s, rot, cam, light, focal)[:2]
    seen = {}
    for sph in (0, 1):
        tr = wm.context(kw, dict(knobs, **knobs_of((64, 64, sph))), s)
        got = tr.render(rot, cam, light, focal, want_rgb=True)
        d = tr.wave_seeds_wide()
        tr.close()
        ts._same(got, want, "UOB_RT_SEED_SPH=%d against UOB_RT_NO_SEED=1" % sph)
        seen[sph] = d
    assert seen[1]["tiles_sphere"] > 0 and seen[1]["jobs_sphere"] > 0, "no shadow part names a sphere candidate"
    f0, f1 = seen[0]["records"]["flags"], seen[1]["records"]["flags"]
    only_sph = ((f1 & rt.SEED_SHADOW_SPH) != 0) & ((f1 & rt.SEED_SHADOW_BLOCKED) == 0)
    assert only_sph.any(), "every sphere candidate lies in a blocked tile"
    assert ((f0 & rt.SEED_SHADOW_WIDE) == 0)[only_sph].all(), "UOB_RT_SEED_SPH=0 kept a sphere candidate"
    assert (f0[~only_sph] == f1[~only_sph]).all()


# ---- 2. state across the frames of one context, streams, edits, bands -------------------------------------------------

@pytest.mark.parametrize("caps", ("default", "open"))
def test_views_and_light_change_between_frames(caps, scene):
    tr = wm.context(ts.SEQ, dict(wm.KNOBS, **knobs_of(None if caps == "default" else OPEN)), scene)
    wide = []
    for k, vi in enumerate(fc.SEQ_ORDER):
        argb, tap = ts._frame_of(tr, ts.VIEWS3[vi])
        fc.same_frame(argb, tap, *ts._fresh(scene, "box", ts.VIEWS3[vi]), "frame %d (view %d)" % (k, vi))
        wide.append(tr.wave_seeds_wide()["jobs_shadow"])
    for lx in (0.0, 0.3, -0.4, 0.0):                                  # the light moves, the view stands
        view = (ts.UP[0][0], ts.UP[0][1], wm.DEFAULT_CAM, [lx, -0.5, -0.7])
        argb, tap = ts._frame_of(tr, view)
        fc.same_frame(argb, tap, *ts._fresh(scene, "box", view), "light at x = %g" % lx)
    tr.close()
    assert all(wide), "a frame of the sequence started no job from a shadow part: %s" % wide


def test_two_contexts_on_two_streams(scene):
    import torch
    dev = torch.device("cuda")
    s = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    trs = [wm.context(ts.SEQ, dict(wm.KNOBS, **knobs_of(c)), scene) for c in (None, OPEN)]
    rows, w = trs[0].rows, trs[0].width
    order = (0, 1, 2, 0, 2, 1)
    # every frame's buffers poisoned before the first frame is enqueued: the fills run on torch's current stream, which the two
    # streams below do not wait for
    bufs = [(torch.full((rows * w,), fc.SENTINEL, dtype=torch.int32, device=dev),
             torch.full((rows * w, 4), float("nan"), dtype=torch.float32, device=dev)) for _ in range(2 * len(order))]
    out = []
    torch.cuda.synchronize(dev)
    for k, vi in enumerate(order):                                    # frames interleaved, nothing waited for in between
        for c in (0, 1):
            yaw, pitch, cam, light = ts.VIEWS3[(vi + c) % 3]
            a, t = bufs[2 * k + c]
            trs[c].render_device(rt.rotation_matrix(yaw, pitch), cam, light, ts._seq_focal(), a.data_ptr(), t.data_ptr(), stream=s[c].cuda_stream)
            out.append(((vi + c) % 3, a, t, "context %d, frame %d" % (c, k)))
    torch.cuda.synchronize(dev)
    for vi, a, t, what in out:
        argb, tap = a.reshape(rows, w).cpu().numpy().view(np.uint32), t.reshape(rows, w, 4).cpu().numpy()
        fc.check_written(argb, tap)
        fc.same_frame(argb, tap, *ts._fresh(scene, "box", ts.VIEWS3[vi]), what)
    for tr in trs:
        tr.close()


def test_the_wall_turns_into_a_mirror_and_back(scene):
    mirror = scene.with_color(wm.BACK_WALL, wm.MIRROR)
    view = ts.VIEWS3[0]
    tr = wm.context(ts.SEQ, dict(wm.KNOBS, **knobs_of(OPEN)), scene)

    def check(s, key, what):
        argb, tap = ts._frame_of(tr, view)
        fc.same_frame(argb, tap, *ts._fresh(s, key, view), what)
        return tr.wave_seeds_wide()

    before = check(scene, "box", "first frame")
    assert before["jobs_shadow"] > 0
    tr.update_scene(mirror)
    d = check(mirror, "mirror", "the wall is a mirror")
    h = d["records"]["h"][(d["records"]["flags"] & rt.SEED_SHADOW_WIDE) != 0]
    assert not np.isin(h, wm.BACK_WALL).any(), "a shadow part on the mirror"
    assert d["tiles_primary"] == before["tiles_primary"], "the primary parts do not depend on the material"
    tr.replace_scene(scene)
    after = check(scene, "box", "the wall is diffuse again")
    tr.close()
    assert wide_counters(after) == wide_counters(before)
    assert after["records"].tobytes() == before["records"].tobytes()


def test_a_rank_whose_bands_miss_every_other_tile_row(scene):
    """Bands of 16 rows, rank 1 of 2, tiles of 16 rows: the even tile rows hold none of its rows and get no record"""
    kw = dict(ts.SEQ, band_rows=16, band_index=1, band_count=2)
    yaw, pitch, cam, light = ts.VIEWS3[0]
    rot = rt.rotation_matrix(yaw, pitch)
    want = ts._render(kw, dict(wm.KNOBS, **ts.NO_SEED), scene, rot, cam, light, ts._seq_focal())[:2]
    tr = wm.context(kw, dict(wm.KNOBS, **knobs_of(OPEN)), scene)
    argb, tap = fc.render_checked(tr, rot, cam, light, ts._seq_focal())
    d = tr.wave_seeds_wide()
    tr.close()
    fc.same_frame(argb, tap, want[0], want[1], "rank 1 of 2, bands of 16 rows")
    assert (d["tile_rows"], d["tiles_per_row"], d["rows_per_tile"]) == (6, 4, 16)
    f = d["records"]["flags"]
    assert (f[0::2] == 0).all(), "a tile without a row of the rank has a record"
    assert (f[1::2] & rt.SEED_PRIMARY_WIDE).all() and d["jobs_primary"] == 16 * d["tiles_primary"] == 16 * 12


def test_headline_frame_on_the_device(scene):
    """The 4096^2 frame bench.py measures, seeded at the shipped caps against UOB_RT_NO_SEED=1, compared on the device"""
    import torch
    rot = rt.rotation_matrix(0.0, 0.0)
    frames = []
    for knobs in ({}, ts.NO_SEED):
        tr = wm.context(wm.HEADLINE, knobs, scene)
        frames.append(fc.render_checked(tr, rot, wm.DEFAULT_CAM, wm.DEFAULT_LIGHT, wm.HEADLINE_FOCAL, to_host=False))
        if not knobs:
            d = tr.wave_seeds_wide()
            assert d["jobs_primary"] > 0 and d["jobs_shadow"] > 0
        tr.close()
    same_argb = torch.equal(frames[0][0], frames[1][0])
    same_tap = torch.equal(frames[0][1][:, :, :3].contiguous().view(torch.int32), frames[1][1][:, :, :3].contiguous().view(torch.int32))
    del frames
    torch.cuda.empty_cache()                 # 0.7 GB of frames and taps: not left in torch's cache for the tests that follow
    assert same_argb, "ARGB words differ"
    assert same_tap, "float tap differs"
