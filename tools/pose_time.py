"""Cost of posing a rigid object (rt_pose_objects / rt_pose_objects_device) against the two ways that exist without it, and
what a refit pose does to the frame that follows.  Scene and frame of tools/scene_update_time.py: Cornell Box +
meshgen.write_cubesphere_obj(n=91) (100 026 triangles), the mesh one object, 2048x2048, 1 spp, 1 shadow ray, no spheres.
One pose = the mesh turned by an angle about the vertical axis through its centre; every sample uses another angle.

  (a) pose_host      rt_pose_objects: 48 bytes up, the pose kernel, check, copy, refit; blocking
  (b) pose_device    rt_pose_objects_device, the matrix in a torch tensor: `call` = until the call returns (the check has
                     been read back), `done` = until the stream has passed it
  (c) host_update    Scene.transformed (one rt_scene_transform call) + RayTracer.update_scene (rt_scene_pack +
                     rt_update_scene); `transform` / `update` are its two parts
  (d) torch_update   the same arithmetic as torch ops on the device (normals by torch.linalg.cross and a division, which
                     need not be the reference's bits) + rt_update_scene_device; `call` / `done` as in (b)
  (e) frame_after    kernel time (rt_last_kernel_ms) of the first frame after a refit pose of 0, 1 and 8 steps of 0.1 rad,
                     and of the first frame after RT_UPDATE_DEVICE_TILES at 8 steps
Every figure: median of --samples samples after --warmup unrecorded ones, with min and max, in ms, host clock around work
that ends in a synchronise (kernel times: device events).  The clocks are warm: frames are rendered before anything is timed.
  python tools/pose_time.py [--size 2048] [--n 91] [--samples 30] [--warmup 5]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uob_raytracer_amd import abi, meshgen, runtime as rt   # noqa: E402


def spin(centre, angle):
    c, s = np.cos(angle), np.sin(angle)
    m = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.concatenate([m, (centre - m @ centre)[:, None]], axis=1).astype(np.float32)[None]


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4), "max": round(float(ms.max()), 4),
            "samples": int(ms.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--n", type=int, default=91)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pose_time.py measures on the GPU: no HIP device present")
    box = rt.Scene.cornell_box()
    path = os.path.join(tempfile.mkdtemp(), "m.obj")
    nf = meshgen.write_cubesphere_obj(path, a.n)
    scene = box + rt.Scene.load_obj(path)
    first, n = len(box), len(scene)
    centre = scene.aos[first:, :3, :3].reshape(-1, 3).mean(axis=0).astype(np.float64)
    cfg = abi.make_config(width=a.size, height=a.size, aa_x=1, aa_y=1, shadow_samples=1, spheres=())
    view = (rt.rotation_matrix(0.0, 0.0), [0.0, 0.0, -3.2], [0.0, -0.5, -0.7], 1100.0 * a.size / 1024)
    angles = [0.01 * (k + 1) for k in range(a.warmup + a.samples)]
    print(json.dumps({"triangles": n, "object": [first, nf], "size": a.size, "warmup": a.warmup}), flush=True)

    def timed(fn):
        """fn(angle) -> tuple of times in ms; the medians over the recorded samples."""
        rows = [fn(x) for x in angles][a.warmup:]
        return [stats(col) for col in zip(*rows)]

    tr = rt.RayTracer(cfg, scene)
    for _ in range(10):                                       # warm clocks, a running context
        tr.render(*view)
    tr.set_objects([(first, nf)])
    stream = torch.cuda.Stream()

    def pose_host(x):
        xf = spin(centre, x)
        t0 = time.perf_counter()
        tr.pose_objects(xf)
        return ((time.perf_counter() - t0) * 1e3,)

    def pose_device(x):
        d_xf = torch.from_numpy(spin(centre, x)).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.pose_objects_device(d_xf, stream=stream)
        t1 = time.perf_counter()
        stream.synchronize()
        return ((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3)

    print(json.dumps({"method": "pose_host", "ms": timed(pose_host)[0]}), flush=True)
    call, done = timed(pose_device)
    print(json.dumps({"method": "pose_device", "call_ms": call, "done_ms": done}), flush=True)

    def frame_after(steps, **kw):
        ms = []
        for _ in range(max(a.samples // 3, 5)):
            tr.pose_objects(spin(centre, 0.1 * steps), **kw)
            tr.render(*view)
            ms.append(tr.last_kernel_ms())
        return stats(ms)

    for steps in (0, 1, 8):
        print(json.dumps({"method": "frame_after", "pose": "refit", "steps_of_0.1rad": steps, "kernel_ms": frame_after(steps)}), flush=True)
    print(json.dumps({"method": "frame_after", "pose": "device_tiles", "steps_of_0.1rad": 8,
                      "kernel_ms": frame_after(8, device_tiles=True)}), flush=True)
    tr.close()

    # the baselines: what the parent commit offers
    tr = rt.RayTracer(cfg, scene)
    for _ in range(3):
        tr.render(*view)
    mesh = slice(first, n)

    def host_update(x):
        xf = spin(centre, x)[0]
        t0 = time.perf_counter()
        new = scene.transformed(mesh, xf[:, :3], xf[:, 3])
        t1 = time.perf_counter()
        tr.update_scene(new)
        t2 = time.perf_counter()
        return ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3)

    tf, up, whole = timed(host_update)
    print(json.dumps({"method": "host_update", "transform_ms": tf, "update_ms": up, "whole_ms": whole}), flush=True)

    v0, n0, c0 = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in scene.packed())
    v, nr = v0.clone(), n0.clone()

    def torch_update(x):
        xf = torch.from_numpy(spin(centre, x)[0]).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            p = v0[3 * first:, :3] @ xf[:, :3].T + xf[:, 3]
            v[3 * first:, :3] = p
            p = p.reshape(-1, 3, 3)
            cr = torch.linalg.cross(p[:, 2] - p[:, 0], p[:, 1] - p[:, 0])
            nr[first:, :3] = cr / torch.linalg.norm(cr, dim=1, keepdim=True)
            tr.update_scene_device(v.data_ptr(), nr.data_ptr(), c0.data_ptr(), n, stream=stream.cuda_stream)
        t1 = time.perf_counter()
        stream.synchronize()
        return ((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3)

    call, done = timed(torch_update)
    print(json.dumps({"method": "torch_update", "call_ms": call, "done_ms": done}), flush=True)
    tr.close()


if __name__ == "__main__":
    main()
