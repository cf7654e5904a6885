"""Records tests/golden/tile_seed_counters.json: the counters of RayTracer.wave_seeds (tiles with a valid primary / shadow
part, jobs that started from one) of every window of tests/test_gpu_tile_seed.py test_seeded_window, from this build, after
showing each seeded frame identical to the frame under UOB_RT_NO_SEED=1 and the table consistent with the AOV pass.
usage (repository root, on the GPU): python tools/record_tile_seed_golden.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_tile_seed as ts
from uob_raytracer_amd import runtime as rt

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "tile_seed_counters.json")
box = rt.Scene.cornell_box()
golden = {}
for view in ts.SEEDED_VIEWS:
    for rows in ts.ROWS:
        got, want, d, prim, s = ts.seeded_case(view, rows, box)
        ts._same(got, want, "%s, %s rows per tile" % (view, rows))
        mixed, not_diffuse = ts.check_table(d, prim, s)
        golden["%s-%s" % (view, rows)] = ts.seed_counters(d)
        print(view, rows, golden["%s-%s" % (view, rows)], "mixed", mixed, "not diffuse", not_diffuse, flush=True)
with open(out, "w") as f:
    json.dump(golden, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out)
