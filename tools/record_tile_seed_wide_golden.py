"""Records tests/golden/tile_seed_wide_counters.json: the counters of RayTracer.wave_seeds_wide of every window of
tests/test_gpu_tile_seed_wide.py test_window at its three settings of the caps, from this build, after showing each frame
identical to the unseeded frames (UOB_RT_NO_SEED=1, no cull, thread-per-pixel kernel, CPU oracle) and both views of the table
consistent with the AOV pass.
usage (repository root, on the GPU): python tools/record_tile_seed_wide_golden.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_tile_seed as ts
import test_gpu_tile_seed_wide as tw
from oracle import pyref
from uob_raytracer_amd import runtime as rt

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "tile_seed_wide_counters.json")
box, oracle = rt.Scene.cornell_box(), pyref.Oracle()
golden = {}
for view in tw.WIDE_VIEWS:
    refs, prim = tw.references(view, box, oracle)
    for caps in sorted(tw.CAPS):
        got, wide, strict, s = tw.wide_case(view, None if caps == "default" else tw.CAPS[caps], box)
        for what, want in refs.items():
            ts._same(got, want, "%s, %s caps, against %s" % (view, caps, what))
        tw.check_wide_table(wide, prim, s, tw.CAPS[caps])
        ts.check_table(strict, prim, s)
        tw.check_counters(wide, strict)
        golden["%s-%s" % (view, caps)] = tw.wide_counters(wide)
        print(view, caps, golden["%s-%s" % (view, caps)], "strict", ts.seed_counters(strict), flush=True)
with open(out, "w") as f:
    json.dump(golden, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out)
