"""What the tile seeds hold on the headline frame (4096^2, 4x2 AA, 64 samples) with the caps wide open: tiles and jobs per
class of record, read through RayTracer.wave_seeds_wide (profiles/tile_seed_wide_counts.txt).
usage (repository root, on the GPU): python tools/tile_seed_wide_counts.py [rows per tile ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uob_raytracer_amd import abi, runtime as rt

pop = np.vectorize(lambda x: bin(int(x)).count("1"))
for rows in (sys.argv[1:] or ["16"]):
    os.environ.update(UOB_RT_SEED_ROWS=rows, UOB_RT_SEED_KP="64", UOB_RT_SEED_CASTERS="64", UOB_RT_SEED_SPH="1")
    tr = rt.RayTracer(abi.make_config(width=4096, height=4096, aa_x=4, aa_y=2, shadow_samples=64), rt.Scene.cornell_box())
    tr.render(rt.rotation_matrix(0, 0), [0, 0, -3.2], [0, -0.5, -0.7], 17600.0)
    d, strict = tr.wave_seeds_wide(), tr.wave_seeds()
    tr.close()
    r = d["records"].reshape(-1)
    f, jobs = r["flags"], int(rows)                  # the whole frame: every tile holds `rows` jobs
    print("R = %s: %d tiles, %d jobs" % (rows, r.size, r.size * jobs))
    print("  strict: %s" % {k: strict[k] for k in ("tiles_primary", "jobs_primary", "tiles_shadow", "jobs_shadow")})
    print("  wide:   %s" % {k: d[k] for k in d if k[:5] in ("tiles", "jobs_") and k != "tiles_per_row"})

    def line(what, m):
        print("  %-58s %6d tiles %8d jobs" % (what, int(m.sum()), int(m.sum()) * jobs))

    pw, sw = (f & rt.SEED_PRIMARY_WIDE) != 0, (f & rt.SEED_SHADOW_WIDE) != 0
    nkp, nk, nkh = pop(r["Kp"]), pop(r["K"]), pop(r["Kh"])
    sph, blk = (f & rt.SEED_SHADOW_SPH) != 0, (f & rt.SEED_SHADOW_BLOCKED) != 0
    line("no primary part", ~pw)
    for lo, hi in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 64)):
        line("primary part, %s triangles" % (lo if lo == hi else "%d+" % lo), pw & (nkp >= lo) & (nkp <= hi))
    line("primary part with the sphere bit", pw & ((f & rt.SEED_PRIMARY_SPH) != 0))
    line("primary part, strict", (f & rt.SEED_PRIMARY) != 0)
    line("no shadow part", ~sw)
    line("shadow part, strict", (f & rt.SEED_SHADOW) != 0)
    line("shadow part, blocked", sw & blk)
    line("shadow part, sphere candidate, not blocked", sw & sph & ~blk)
    for name, cnt in (("K", nk), ("Kh", nkh)):
        for lo, hi in ((0, 0), (1, 1), (2, 2), (3, 4), (5, 64)):
            line("shadow part, not blocked, popcount(%s) %s" % (name, lo if lo == hi else "%d..%d" % (lo, hi)),
                 sw & ~blk & (cnt >= lo) & (cnt <= hi))
    line("shadow part not strict, on a strict primary tile", sw & ((f & rt.SEED_SHADOW) == 0) & ((f & rt.SEED_PRIMARY) != 0))
    line("shadow part on a tile of several triangles or a sphere", sw & ((f & rt.SEED_PRIMARY) == 0))
