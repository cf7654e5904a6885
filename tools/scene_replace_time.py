"""Cost of replacing a context's scene by one of another triangle count (rt_replace_scene / rt_replace_scene_device), against
rt_destroy + rt_init, and what the tiling each leaves does to the frames after it.  One JSON line per method:
  scene   Cornell Box + meshgen.write_cubesphere_obj(n=91) (99 398 triangles); the context starts with the box + a mesh of
          n - 8 (fewer triangles: the replace stays outside its capacity the first time, inside it from then on);
          2048x2048, 1 spp, 1 shadow ray, no spheres (bench.py configs[4], "cfg5")
  method  init = rt_destroy + rt_init; replace = rt_replace_scene (host tiles: kd unless UOB_RT_TILE_ORDER=morton);
          replace_dt = rt_replace_scene with RT_UPDATE_DEVICE_TILES; device = rt_replace_scene_device from torch tensors
Timing: one warm-up round, then the median of --reps (>= 7) rounds; a round alternates between the two scenes, so every timed
replace is within the capacity.  Blocking calls by wall clock; the device entry also by stream events around the call (what
the GPU spends on it, `device_ms`) next to the wall time until the call returns (`call_ms`, the read-back wait included) and
until the stream has passed it (`done_ms`).  steady_ms = median kernel time of --steady frames after the last replace;
tile_visits = rt_count_executed's primary and shadow tile visits of that context.
  python tools/scene_replace_time.py [--size 2048] [--n 91] [--reps 7] [--steady 5]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uob_raytracer_amd import abi, meshgen, runtime as rt   # noqa: E402


def mesh_scene(box, n):
    path = os.path.join(tempfile.mkdtemp(), "m%d.obj" % n)
    meshgen.write_cubesphere_obj(path, n)
    return box + rt.Scene.load_obj(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--n", type=int, default=91)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steady", type=int, default=5)
    a = ap.parse_args()
    import torch
    box = rt.Scene.cornell_box()
    big, small = mesh_scene(box, a.n), mesh_scene(box, a.n - 8)
    cfg = abi.make_config(width=a.size, height=a.size, aa_x=1, aa_y=1, shadow_samples=1, spheres=())
    rot, cam, light, focal = rt.rotation_matrix(0.0, 0.0), [0.0, 0.0, -3.2], [0.0, -0.5, -0.7], 1100.0 * a.size / 1024
    for method in ("init", "replace", "replace_dt", "device"):
        tr = rt.RayTracer(cfg, small)
        tr.render(rot, cam, light, focal)
        dev = {id(s): [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in s.packed()] for s in (big, small)}
        stream = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        call, done, gpu = [], [], []
        for rep in range(2 * (a.reps + 1)):                      # (the first round of two warms up: it grows the buffers)
            new = big if rep % 2 == 0 else small
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if method == "init":
                tr.close()
                tr = rt.RayTracer(cfg, new)
            elif method == "device":
                e0.record(stream)
                tr.replace_scene_device(*dev[id(new)], stream=stream)
                e1.record(stream)
            else:
                tr.replace_scene(new, device_tiles=method == "replace_dt")
            t1 = time.perf_counter()
            stream.synchronize()
            t2 = time.perf_counter()
            if rep >= 2 and rep % 2 == 0:                        # the replaces by the larger scene
                call.append((t1 - t0) * 1e3)
                done.append((t2 - t0) * 1e3)
                if method == "device":
                    gpu.append(e0.elapsed_time(e1))
            tr.render(rot, cam, light, focal)                    # a context in use: a frame between the replaces
        if len(tr.scene if tr.scene is not None else big) != len(big) or tr.n_triangles != len(big):
            if method == "device":
                tr.replace_scene_device(*dev[id(big)], stream=stream)
            elif method == "init":
                tr.close()
                tr = rt.RayTracer(cfg, big)
            else:
                tr.replace_scene(big, device_tiles=method == "replace_dt")
        ms = []
        for _ in range(a.steady + 1):
            tr.render(rot, cam, light, focal)
            ms.append(tr.last_kernel_ms())
        work = tr.count_executed(rot, cam, light, focal)
        rec = {"method": method, "triangles": len(big), "size": a.size, "reps": len(call), "call_ms": float(np.median(call)),
               "done_ms": float(np.median(done)), "steady_ms": float(np.median(ms[1:])),
               "capacity": tr.scene_capacity(),
               "tile_visits": [work["primary_tile_visits"], work["shadow_tile_visits"]]}
        if gpu:
            rec["device_ms"] = float(np.median(gpu))
        tr.close()
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)


if __name__ == "__main__":
    main()
