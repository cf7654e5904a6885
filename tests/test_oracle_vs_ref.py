"""CPU: the oracle restatement against the reference kernel itself on inputs beyond the committed frame fixtures —
different views, lights and a modified scene.  The reference kernel (built from the reference's kernels.cl for x86-64
by oracle/build_ref.py) rendered every case once: tests/golden/oracle_vs_ref.json holds the SHA-256 of its ARGB words
and of its clamped 255*c taps per (case, scene, view), written by `python tests/golden/make_golden.py --vs-ref`.
Equal hashes are equal bits: tolerance 0."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import pyref
from uob_raytracer_amd import abi

G = os.path.join(os.path.dirname(__file__), "golden")

VIEWS = [(0.0, 0.0, [0.0, 0.0, -3.2], [0.4, -0.5, -0.7]), (-0.5, 0.3, [-0.4, -0.2, -2.7], [0.0, 0.3, -0.2]),
         (1.2, 0.0, [1.5, 0.0, -1.5], [0.0, -0.9, 0.0])]
CASES = {"default256": dict(width=256, height=256),
         "cfg2_256": dict(width=256, height=256, shadow_samples=16, spheres=()),
         "cfg3_480": dict(width=480, height=270, max_bounces=5),
         "aa3_256": dict(width=256, height=256, aa_x=3, aa_y=3),
         "cfg1": dict(width=256, height=256, aa_x=1, aa_y=1, shadow_samples=1, light_spread=0.0, spheres=())}


def scenes(aos):
    """The scene as loaded, and the same box with a mirror left wall and one glass face of the tall block."""
    mod = aos.copy()
    mod[[2, 3], 4, :] = (1.0, 1.0, 1.0, 0.0)      # left wall -> mirror
    mod[[20, 21], 4, :] = (0.0, 0.0, 0.0, -1.0)   # one tall-block face -> glass
    return [aos, mod]


def digest(a):
    """SHA-256 of an array's 32-bit words (ARGB words or float32 taps), with its shape."""
    a = np.ascontiguousarray(a)
    return {"shape": list(a.shape), "sha256": hashlib.sha256(a.view(np.uint32).tobytes()).hexdigest()}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(G, "oracle_vs_ref.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_reference_kernel(name, scene, oracle, golden):
    kw = CASES[name]
    cfg = abi.make_config(**kw)
    want = golden["cases"][name]
    assert want["config"] == json.loads(json.dumps(kw)) and golden["views"] == json.loads(json.dumps(VIEWS))
    focal = 1100.0 * min(cfg.width, cfg.height) / 1024.0 * cfg.aa_x
    for si, scene_aos in enumerate(scenes(scene.aos)):
        v, n, c = pyref.pack_scene(scene_aos)
        for vi, (yaw, pitch, cam, light) in enumerate(VIEWS):
            rot = pyref.rot_matrix(yaw, pitch)
            a1, r1 = oracle.render(cfg, v, n, c, rot, cam, light, focal)
            ref = want["frames"][si][vi]
            assert digest(a1) == ref["argb"], "%s scene %d view %d: ARGB differs from the reference kernel" % (name, si, vi)
            _, tap = pyref.quantise(r1)
            assert digest(tap) == ref["tap"], "%s scene %d view %d: taps differ from the reference kernel" % (name, si, vi)


# ---- closest-hit ties --------------------------------------------------------------------------------------------------
# The reference keeps a hit unless a later triangle is STRICTLY nearer (kernels.cl:120, :194): at bit-equal t the lowest
# original index wins.  Scenes of tests/ties_util.py in which thousands of rays meet two triangles at equal t, on the
# reference's default kernel at 256x256: frames, and single_ray_intersections (:168) on 4 000 rays aimed at the tied
# triangles — the winning index and the ten outputs.  tests/golden/ties_mesh_10x8_aos.npy is meshgen's (10, 8) sphere
# through the product's loader, stored so that the hashed input does not depend on a machine's sin and cos.
TIE_CASE = "default256"
TIE_VIEWS = ["default", "side", "mesh_front"]
TIE_SCENES = ["double_reversed_after", "double_reversed_first", "decal_wall_after", "decal_wall_first", "mesh_10x8_double_sided"]
TIE_RAYS = 4000


def tie_scene(name, box):
    """-> (aos, pairs, rays) of a TIE_SCENES name"""
    import ties_util as tu
    from uob_raytracer_amd import runtime as rt
    if name.startswith("mesh_"):
        s, pairs = tu.mesh_scene(rt.Scene(box), np.load(os.path.join(G, "ties_mesh_10x8_aos.npy")), "mesh_copies")
    else:
        kind, order = name.rsplit("_", 1)
        s, pairs = tu.box_scene(rt.Scene(box), {"double_reversed": "reversed", "decal_wall": "decal_wall"}[kind], order)
    return s.aos, pairs, tu.seeded_rays(TIE_RAYS, 4242, s, pairs)


def tie_view(name):
    """-> (rot, cam, light, focal) of a TIE_VIEWS name on the TIE_CASE frame"""
    import ties_util as tu
    yaw, pitch, cam, light, lens = tu.view(name)
    kw = CASES[TIE_CASE]
    return pyref.rot_matrix(yaw, pitch), cam, light, 1100.0 * min(kw["width"], kw["height"]) / 1024.0 * 2 * lens


@pytest.mark.parametrize("name", TIE_SCENES)
def test_oracle_ties_equal_reference_kernel(name, scene, oracle, golden):
    import ties_util as tu
    want = golden["ties"]
    assert want["case"] == TIE_CASE and want["views"] == TIE_VIEWS and want["rays"] == TIE_RAYS
    cfg = abi.make_config(**CASES[TIE_CASE])
    aos, pairs, rays = tie_scene(name, scene.aos)
    v, n, c = pyref.pack_scene(aos)
    ref = want["scenes"][name]
    for vi, vname in enumerate(TIE_VIEWS):
        rot, cam, light, focal = tie_view(vname)
        a1, r1 = oracle.render(cfg, v, n, c, rot, cam, light, focal)
        assert digest(a1) == ref["frames"][vi]["argb"], "%s view %s: ARGB differs from the reference kernel" % (name, vname)
        assert digest(pyref.quantise(r1)[1]) == ref["frames"][vi]["tap"], "%s view %s: taps differ" % (name, vname)
    tri, out = oracle.closest_hit(cfg, v, n, c, rays)
    assert (tri != -1).all(), "a ray of the record misses the scene"        # (-2: a sphere in front)
    assert digest(tri) == ref["closest_hit"]["tri"], name + ": the winning triangles differ from the reference's"
    assert digest(out) == ref["closest_hit"]["out"], name + ": the ten outputs differ from the reference's"
    # the record holds what it is for: rays that meet a pair at equal t, won by the lower index
    from uob_raytracer_amd import runtime as rt
    c_ = tu.census(oracle, cfg, rt.Scene(aos), pairs, rays)
    print("%s: of %d rays %d on a pair, %d tied, %d untied" % (name, len(rays), c_["on_pair"], c_["tied"], c_["untied"]))
    assert c_["tied"] >= 200 and c_["higher"] == 0 and ref["tied_rays"] == c_["tied"]


def test_product_scene_equals_reference_scene(scene):
    """scene_cornell_aos.npy is the reference's own LoadTestModel (tests/golden/make_golden.py)."""
    want = np.load(os.path.join(G, "scene_cornell_aos.npy"))
    assert np.array_equal(scene.aos.view(np.uint32), want.view(np.uint32))
