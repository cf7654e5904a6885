"""Cost of replacing a context's triangles between frames (rt_update_scene / rt_update_scene_device), against rt_destroy +
rt_init, and what each does to the frames after it.  One JSON line per (scene, motion, method):
  scene   mesh = Cornell Box + meshgen.write_cubesphere_obj(n=91) (~100k triangles), box = the 26 triangles alone;
          2048x2048, 1 spp, 1 shadow ray, no spheres (bench.py configs[4], "cfg5")
  motion  rigid = the mesh (the short block for the box) slides by a small offset; squash = half of it is flattened to
          half its height about its centre (a strong non-rigid deformation)
  method  init = rt_destroy + rt_init, refit = rt_update_scene, reorder = rt_update_scene(RT_UPDATE_REORDER),
          device = rt_update_scene_device from torch tensors (the call's wall time, then the stream's)
Reported: update_ms (wall time of the call; for `device` also the time until the stream has passed it), first_ms = kernel
time of the first frame after, steady_ms = the median of the next `--steady` frames.
  python tools/scene_update_time.py [--size 2048] [--n 91] [--steady 5] [--only mesh|box]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uob_raytracer_amd import abi, meshgen, runtime as rt   # noqa: E402


def frames(tr, steady, view):
    rot, cam, light, focal = view
    tr.render(rot, cam, light, focal)
    first = tr.last_kernel_ms()
    times = []
    for _ in range(steady):
        tr.render(rot, cam, light, focal)
        times.append(tr.last_kernel_ms())
    return first, float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--n", type=int, default=91)
    ap.add_argument("--steady", type=int, default=5)
    ap.add_argument("--only", choices=("mesh", "box"), default=None)
    a = ap.parse_args()
    import torch
    box = rt.Scene.cornell_box()
    path = os.path.join(tempfile.mkdtemp(), "m.obj")
    nf = meshgen.write_cubesphere_obj(path, a.n)
    cases = {"box": (box, list(range(10, 18))), "mesh": (box + rt.Scene.load_obj(path), list(range(26, 26 + nf)))}
    cfg = abi.make_config(width=a.size, height=a.size, aa_x=1, aa_y=1, shadow_samples=1, spheres=())
    view = (rt.rotation_matrix(0.0, 0.0), [0.0, 0.0, -3.2], [0.0, -0.5, -0.7], 1100.0 * a.size / 1024)
    for name, (scene, moving) in cases.items():
        if a.only and name != a.only:
            continue
        centre = scene.aos[moving, :3, :3].reshape(-1, 3).mean(axis=0).astype(np.float32)
        sq = np.diag([1.0, 0.5, 1.0]).astype(np.float32)
        motions = {"rigid": scene.transformed(moving, np.eye(3), (0.05, 0.0, -0.05)),
                   "squash": scene.transformed(moving[:len(moving) // 2], sq, centre - sq @ centre)}
        for motion, new in motions.items():
            for method in ("init", "refit", "reorder", "device"):
                tr = rt.RayTracer(cfg, scene)
                frames(tr, 2, view)                                   # warm: the scheduling state of a running context
                rec = {"scene": name, "triangles": len(scene), "size": a.size, "motion": motion, "method": method}
                if method == "device":
                    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in new.packed()]
                    stream = torch.cuda.Stream()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr.update_scene_device(*(t.data_ptr() for t in dev), len(new), stream=stream.cuda_stream)
                    t1 = time.perf_counter()
                    stream.synchronize()
                    t2 = time.perf_counter()
                    rec["update_ms"], rec["update_done_ms"] = (t1 - t0) * 1e3, (t2 - t0) * 1e3
                elif method == "init":
                    t0 = time.perf_counter()
                    tr.close()
                    tr = rt.RayTracer(cfg, new)
                    rec["update_ms"] = (time.perf_counter() - t0) * 1e3
                else:
                    t0 = time.perf_counter()
                    tr.update_scene(new, reorder=method == "reorder")
                    rec["update_ms"] = (time.perf_counter() - t0) * 1e3
                rec["first_ms"], rec["steady_ms"] = frames(tr, a.steady, view)
                tr.close()
                print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)


if __name__ == "__main__":
    main()
