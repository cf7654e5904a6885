"""Ray queries (rt_trace_rays) against the brute-force diagnostic (rt_debug_trace_rays) on 2^20 rays per set.

Scenes: the box + a meshgen.write_sphere_obj(path, 256, 196) mesh (99 866 triangles), and the box alone.  Ray sets:
  camera  : from the default camera through a 1024^2 grid (row-major), the default view's focal length
  shadow  : from the camera rays' hit points towards the default light, as direct_light sets them up (kernels.cl:323-326)
  random  : uniformly random starts inside the box, uniformly random directions
One JSON line per (scene, set): end-to-end ms of rt_trace_rays and rt_debug_trace_rays (the same host copies), the device
entry's ms from stream events, whether the answers are identical, and the query's work counters (rt_debug_trace_stats).
usage: python tools/ray_query_time.py [--reps 3] [--only mesh|box]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from uob_raytracer_amd import abi, meshgen, runtime as rt  # noqa: E402

CAM = np.array([0.0, 0.0, -3.2], np.float32)
LIGHT = np.array([0.0, -0.5, -0.7], np.float32)
SIDE = 1024


def camera_rays():
    y, x = np.divmod(np.arange(SIDE * SIDE, dtype=np.int64), SIDE)
    d = np.stack([x - SIDE / 2 + 0.5, y - SIDE / 2 + 0.5, np.full(x.shape, 1100.0)], 1).astype(np.float32)
    d /= np.sqrt((d * d).sum(1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(CAM, d.shape), d], 1), np.float32)


def shadow_rays(out):
    p = out[:, 0:3]
    d = (LIGHT - p).astype(np.float32)
    s = (p + np.float32(1e-4) * d).astype(np.float32)
    r2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([s, d], 1), np.float32), r2


def random_rays(k, seed=1):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-1.0, 1.0, (k, 3)).astype(np.float32)
    d = rng.normal(size=(k, 3)).astype(np.float32)
    d /= np.sqrt((d * d).sum(1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([s, d], 1), np.float32)


def best_ms(fns, reps):
    """Best wall time of each function, the functions called in turn (interleaved: drift hits them alike)."""
    ts = [[] for _ in fns]
    res = [None] * len(fns)
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            res[i] = fn()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [min(t) for t in ts], res


def device_ms(tr, torch, what, rays, r2, reps):
    """Mean device time of `reps` back-to-back rt_trace_rays_device calls between two stream events (a query shorter than
    its own enqueue on the host shows the enqueue time instead)."""
    s = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays).cuda()
    d_r2 = torch.from_numpy(r2).cuda() if r2 is not None else None
    out_tri = torch.empty(len(rays), dtype=torch.int32, device="cuda")
    out10 = torch.empty((len(rays), 10), dtype=torch.float32, device="cuda") if r2 is None else None
    tr.query_device(what, d_rays, d_r2, out_tri, out10, stream=s)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        tr.query_device(what, d_rays, d_r2, out_tri, out10, stream=s)
    e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / reps


def run(name, scene, reps, torch):
    tr = rt.RayTracer(abi.make_config(width=64, height=64), scene)
    cam = camera_rays()
    c_tri, c_out = tr.query_closest_hit(cam)
    srays, r2 = shadow_rays(c_out)
    sets = [("camera", cam, None), ("shadow", srays, r2), ("random", random_rays(len(cam)), None)]
    for set_name, rays, rr in sets:
        if rr is None:
            (q_ms, b_ms), ((q_tri, q_out), (b_tri, b_out)) = best_ms(
                [lambda: tr.query_closest_hit(rays), lambda: tr.trace_closest_hit(rays)], reps)
            same = bool(np.array_equal(q_tri, b_tri) and np.array_equal(q_out.view(np.uint32), b_out.view(np.uint32)))
            what = abi.RT_TRACE_CLOSEST_HIT
        else:
            (q_ms, b_ms), (q, b) = best_ms([lambda: tr.query_in_shadow(rays, rr), lambda: tr.trace_in_shadow(rays, rr)], reps)
            same = bool(np.array_equal(q, b))
            what = abi.RT_TRACE_IN_SHADOW
        dev = device_ms(tr, torch, what, rays, rr, reps)
        stats = tr.trace_stats()                   # (of the last query, on the same rays)
        print(json.dumps({"scene": name, "triangles": len(scene), "set": set_name, "rays": len(rays),
                          "query_ms": round(q_ms, 3), "debug_trace_ms": round(b_ms, 3), "speedup": round(b_ms / q_ms, 2),
                          "device_ms": round(dev, 3), "identical": same, "stats": stats}), flush=True)
    tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("mesh", "box"))
    a = ap.parse_args()
    import torch
    box = rt.Scene.cornell_box()
    if a.only != "box":
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.obj")
            meshgen.write_sphere_obj(path, 256, 196)
            run("box+mesh", box + rt.Scene.load_obj(path), a.reps, torch)
    if a.only != "mesh":
        run("box", box, a.reps, torch)


if __name__ == "__main__":
    main()
