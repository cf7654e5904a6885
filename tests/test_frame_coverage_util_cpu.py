"""CPU: tests/frame_coverage_util.py — what tests/test_gpu_frame_coverage.py measures with — checked without a device:
expected_jobs on hand-computed shapes, the poison checks on planted poison, and the helper's band rows against
rt_config_owned_rows."""
import ctypes as C

import numpy as np
import pytest

import frame_coverage_util as fc
from uob_raytracer_amd import abi, runtime as rt


@pytest.mark.parametrize("kw,job_tasks,want", [
    (dict(width=256, height=96, aa_x=4, aa_y=2), 8, 4 * 96),                       # 64-pixel jobs
    (dict(width=250, height=37, aa_x=4, aa_y=2), 4, 8 * 37),                       # ragged: 7 jobs of 32 pixels + one of 26
    (dict(width=200, height=50, aa_x=2, aa_y=2), 4, 4 * 50),                       # 16 pixels per task: 3 jobs of 64 + one of 8
    (dict(width=100, height=40, aa_x=3, aa_y=3), 5, 3 * 40),                       # 7 pixels per task: 35-pixel jobs
    (dict(width=60, height=24, aa_x=4, aa_y=2), 8, 24),                            # narrower than one job
    (dict(width=83, height=40, aa_x=9, aa_y=9), None, 6 * 40),                     # chunked grid: 16-pixel jobs
    (dict(width=83, height=40, aa_x=16, aa_y=16), 8, 6 * 40),                      # ... whatever the knob says
    (dict(width=256, height=96, aa_x=4, aa_y=2, band_rows=8, band_index=1, band_count=3), 8, 4 * 32),   # rows 8-15, 32-39, 56-63, 80-87
    (dict(width=33, height=5, aa_x=4, aa_y=2, band_rows=1, band_index=6, band_count=7), 2, 0),          # a rank without rows
])
def test_expected_jobs(kw, job_tasks, want):
    assert fc.expected_jobs(abi.make_config(**kw), job_tasks) == want


@pytest.mark.parametrize("kw,job_tasks", [
    (dict(width=64, height=8, aa_x=4, aa_y=2), 1),        # 8-pixel jobs: below the 16 the knob is honoured from
    (dict(width=64, height=8, aa_x=2, aa_y=2), 5),        # 80-pixel jobs: beyond a wave
    (dict(width=64, height=8, aa_x=4, aa_y=2), None),     # no chunked grid: the size must be given
])
def test_expected_jobs_refuses_what_the_knob_may_not_do(kw, job_tasks):
    with pytest.raises(ValueError):
        fc.expected_jobs(abi.make_config(**kw), job_tasks)


def _clean(rows=5, w=7):
    argb = np.full((rows, w), 0xFF102030, np.uint32)
    tap = np.zeros((rows, w, 4), np.float32)
    tap[..., 3] = fc.TAP_W
    return argb, tap


def test_the_poison_checks_flag_planted_poison():
    assert fc.SENTINEL >> 24 == 0 and fc.SENTINEL < 2 ** 31            # alpha 0, and an int32 tensor can hold it
    argb, tap = _clean()
    fc.check_written(argb, tap)
    fc.check_written(argb)
    fc.check_written(argb[:0], tap[:0])                                   # a rank without rows
    bad = argb.copy()
    bad[3, 6] = fc.SENTINEL
    with pytest.raises(AssertionError, match=r"1 of 35 pixels were never written.*\[3 6\]"):
        fc.check_written(bad, tap)
    with pytest.raises(AssertionError, match="never written"):
        fc.check_written(bad.view(np.int32))                              # as the tensor's dtype
    bad = tap.copy()
    bad[4, 0, 1] = np.nan
    with pytest.raises(AssertionError, match=r"1 tap components are NaN.*\[4 0 1\]"):
        fc.check_written(argb, bad)
    expected = np.zeros((5, 7, 3), np.float32)
    with pytest.raises(AssertionError, match="NaN"):
        fc.check_written(argb, bad, expected)
    expected[4, 0, 1] = np.nan                                            # the expected tap has one there: allowed
    fc.check_written(argb, bad, expected)
    bad = tap.copy()
    bad[0, 0, 3] = np.nan                                                 # a tap whose w was never stored
    with pytest.raises(AssertionError, match="w = 1"):
        fc.check_written(argb, bad)
    bad = argb.copy()
    bad[0, 0] = 0x00FFFFFF
    with pytest.raises(AssertionError, match="alpha"):
        fc.check_written(bad)


def test_same_frame_names_the_first_difference():
    argb, tap = _clean()
    fc.same_frame(argb, tap, argb.ravel(), tap[..., :3].reshape(-1, 3), "x")
    other = argb.copy()
    other[2, 1] ^= 1
    with pytest.raises(AssertionError, match=r"x: 1 of 35 pixels differ.*\[2 1\]"):
        fc.same_frame(argb, tap, other, None, "x")
    other = tap.copy()
    other[1, 1, 2] = -0.0                                                 # bits, not values
    with pytest.raises(AssertionError, match=r"1 tap components differ.*\[1 1 2\]"):
        fc.same_frame(argb, tap, argb, other, "x")


@pytest.mark.parametrize("height,band_rows,band_count", [(96, 8, 3), (31, 1, 7), (5, 1, 7), (37, 16, 2), (40, 40, 1)])
def test_band_rows_agree_with_the_library(height, band_rows, band_count):
    seen = []
    for index in range(band_count):
        cfg = abi.make_config(width=33, height=height, band_rows=band_rows, band_index=index, band_count=band_count)
        rows = fc.owned_rows(cfg)
        assert rt.lib().rt_config_owned_rows(C.byref(cfg)) == len(rows)
        seen += rows
    assert sorted(seen) == list(range(height))                            # every row in exactly one band
    if (height, band_count) == (5, 7):
        assert fc.owned_rows(abi.make_config(width=33, height=5, band_rows=1, band_index=6, band_count=7)) == []
