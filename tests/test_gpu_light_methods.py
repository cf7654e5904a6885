"""-m gpu: render_direct_light, render_filtered_light and render_accumulated_light agree with each other where they state the
same thing: on the Cornell box at 64 x 48, one sample per pixel, 4 shadow samples, the first frame of an accumulated sequence
has the term and the visibility of the filtered light bit for bit, again after reset_history(); and the direct light is 0
exactly where the pixel sees nothing and negative nowhere."""
import numpy as np
import pytest

from conftest import DEFAULT_CAM, DEFAULT_LIGHT, focal_for
from uob_raytracer_amd import abi, runtime as rt

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_the_three_light_methods_agree_on_a_first_frame(scene):
    import torch
    cfg = abi.make_config(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=4)
    tr = rt.RayTracer(cfg, scene)
    try:
        rot = rt.rotation_matrix(0.0, 0.0)
        view = (rot, DEFAULT_CAM, DEFAULT_LIGHT, focal_for(cfg))
        _, f_term, f_vis, _ = tr.render_filtered_light(*view, want_parts=True)
        first = tr.render_accumulated_light(*view, want_parts=True)
        direct = tr.render_direct_light(*view)
        tr.reset_history()
        again = tr.render_accumulated_light(*view, want_parts=True)
        torch.cuda.synchronize()
        prim = tr.render_aov(rot, DEFAULT_CAM, focal_for(cfg), planes=("prim",))["prim"]
    finally:
        tr.close()
    assert np.array_equal(_bits(first[1]), _bits(f_term)) and np.array_equal(_bits(first[2]), _bits(f_vis))
    assert len(first) == len(again) == 6
    for a, b in zip(first, again):                              # out, term, V, V_mean, variance, count
        assert np.array_equal(_bits(a), _bits(b))
    miss = prim == -1
    direct = direct.cpu().numpy()
    assert direct.shape == miss.shape == (48, 64) and miss.any() and not miss.all()
    assert (direct[miss] == 0).all() and (direct >= 0).all() and (direct[~miss] > 0).any()
    assert (f_vis.cpu().numpy()[~miss] > 0).any() and (f_term.cpu().numpy()[~miss] > 0).any()       # the parts are not all zero
