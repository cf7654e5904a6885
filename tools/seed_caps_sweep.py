"""The caps of the tile seeds on the headline frame: one context per setting of (UOB_RT_SEED_KP, UOB_RT_SEED_CASTERS,
UOB_RT_SEED_SPH) in ONE process (rt_init reads the knobs), timed in interleaved rounds of 40 frames, median kernel ms per
round.  A screening tool: a setting it prefers is confirmed with tools/ab_time.py and bench.py in processes of their own.
usage (repository root, on the GPU): python tools/seed_caps_sweep.py [rounds]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uob_raytracer_amd import abi, runtime as rt

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
settings = [("no seed", None), ("1/0/0", (1, 0, 0))]
settings += [("%d/0/0" % kp, (kp, 0, 0)) for kp in (2, 3, 4, 64)]
settings += [("1/%d/0" % k, (1, k, 0)) for k in (1, 2, 4, 32)] + [("1/0/1", (1, 0, 1))]
settings += [("64/%d/%d" % (k, s), (64, k, s)) for k in (0, 1, 2, 4, 32) for s in (0, 1)]
cfg = abi.make_config(width=4096, height=4096, aa_x=4, aa_y=2, shadow_samples=64)
rot, cam, light = rt.rotation_matrix(0, 0), [0, 0, -3.2], [0, -0.5, -0.7]
buf = torch.empty((4096, 4096), dtype=torch.int32, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
ctx = []
for name, caps in settings:
    for k in ("UOB_RT_NO_SEED", "UOB_RT_SEED_KP", "UOB_RT_SEED_CASTERS", "UOB_RT_SEED_SPH"):
        os.environ.pop(k, None)
    if caps is None:
        os.environ["UOB_RT_NO_SEED"] = "1"
    else:
        os.environ.update(UOB_RT_SEED_KP=str(caps[0]), UOB_RT_SEED_CASTERS=str(caps[1]), UOB_RT_SEED_SPH=str(caps[2]))
    ctx.append(rt.RayTracer(cfg, rt.Scene.cornell_box()))
res = [[] for _ in settings]
for rnd in range(rounds + 1):                       # round 0 warms every context (and the clocks) up
    for i, tr in enumerate(ctx):
        ts = []
        for _ in range(40):
            tr.render_device(rot, cam, light, 17600.0, buf.data_ptr(), None, stream)
            ts.append(tr.last_kernel_ms())
        if rnd:
            res[i].append(sorted(ts)[20])
print("KP/CASTERS/SPH   median kernel ms per round (pre-pass + memset + draw kernel)")
for (name, _), r in zip(settings, res):
    print("  %-10s %s   best %.4f" % (name, " ".join("%.4f" % v for v in r), min(r)))
for tr in ctx:
    tr.close()
