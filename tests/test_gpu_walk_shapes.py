"""-m gpu: the one tiled walk (rt_tiles.h tile_walk) at the shapes where its loop can go wrong — a second tile holding one
triangle (n = 65), candidate masks of two words (n = 26 + 4097: 65 tiles), a 40 x 40 frame whose waves straddle the
screen-cell edge at 32, runs of 64 (pixel, sample) elements that cross it mid-run, a banded context whose packed rows jump,
with and without tile bins (tests/walk_shapes_util.py).
The planes of every pass, and the answers of one closest-hit query, one in-shadow query and one rt_radiance_rays call on
the same scenes, equal the brute-force diagnostic rt_debug_trace_rays fed the pass's own direction plane, bit for bit.
NOT here yet: the comparison of the work counters of those passes and calls with values recorded on the commit before the
AOV pass moved into the shared walk.  tools/walk_counters.py records them (tests/golden/walk_counters.json); no device could
be reached when this file was written, and a fixture that was never run is not committed."""
import numpy as np
import pytest

import aov_util
import walk_shapes_util as ws

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_shapes")
    return {name: ws.build_scene(name, d) for name in ws.SCENES}


@pytest.mark.parametrize("pass_name", list(ws.PASSES))
@pytest.mark.parametrize("name", list(ws.SCENES))
def test_pass_equals_brute_force(name, pass_name, scenes):
    tr, planes, stats = ws.run_pass(scenes[name], pass_name)
    tri, out10 = tr.trace_closest_hit(ws.rays_of_pass(planes))
    tr.close()
    want = aov_util.expected_planes(ws.CAM, planes["direction"][..., :3], tri, out10)
    aov_util.assert_planes_equal(planes, want, ("prim", "position", "normal", "albedo"))
    prim = planes["prim"]
    assert (prim >= 26).any() and (prim == -1).any() and ((prim >= 0) & (prim < 26)).any()     # mesh, misses and box in view
    print(stats)
    assert stats["tiles"] == (int(name) + 63) // 64 and stats["waves"] > 0


@pytest.mark.parametrize("name", list(ws.SCENES))
def test_calls_equal_brute_force(name, scenes):
    tr, planes, _ = ws.run_pass(scenes[name], ws.CALLS_PASS)
    rays = ws.rays_of_pass(planes)
    stats, got = ws.run_calls(tr, rays)
    tri, out10 = tr.trace_closest_hit(rays)
    blocked = tr.trace_in_shadow(rays, np.full(rays.shape[0], ws.RADIUS_SQ, np.float32))
    tr.close()
    assert np.array_equal(got["tri"], tri) and np.array_equal(aov_util.u32(got["out10"]), aov_util.u32(out10))
    assert np.array_equal(got["blocked"], blocked) and 0 < blocked.sum() < blocked.size
    assert np.array_equal(got["rgba"][:, 3] != 0, tri != -1)
    print(stats)
