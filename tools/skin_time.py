"""Cost of posing a skin (rt_pose_skin_device) at 2 and 256 bones, beside the two ways the same mesh could move before:
a host upload (rt_update_scene) and a rigid pose (rt_pose_objects_device).  Scene of bench.py's configs[4]: Cornell Box +
meshgen.write_sphere_obj(250, 201) (100 026 triangles), 2048x2048, 1 spp, 1 shadow ray, no spheres.

  skin_device     rt_pose_skin_device, the bones in a torch tensor, for nbones in (2, 256) and flags in (0,
                  RT_UPDATE_DEVICE_TILES): `call` = until the call returns (the check has been read back), `done` = until the
                  stream has passed it (the skin kernel, check, copy, refit or tile build).  2 bones: weights by height, as the
                  application's --bend.  256 bones: four non-zero influences per corner, the bones of a corner drawn from a
                  window of 8 around its height band (neighbouring lanes read neighbouring bones, as a rigged mesh does).
  objects_device  rt_pose_objects_device, the mesh one object: the same tail without the blend (flags as above)
  host_update     RayTracer.update_scene of an already skinned Scene: rt_scene_pack + rt_update_scene, 80 bytes per triangle
                  over the bus; blocking
The four skin contexts, the object context and the update context take turns sample by sample, so drift of the clocks hits
all alike.  Every figure: median of --samples samples after --warmup unrecorded ones, with min and max, in ms, host clock
around work that ends in a synchronise.  The clocks are warm: frames are rendered before anything is timed.
  python tools/skin_time.py [--size 2048] [--lon 250 --lat 201] [--samples 30] [--warmup 5] > profiles/skin_time.txt"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uob_raytracer_amd import abi, meshgen, runtime as rt   # noqa: E402

F32 = np.float32


def turn(centre, angle):
    c, s = np.cos(angle), np.sin(angle)
    m = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.concatenate([m, (centre - m @ centre)[:, None]], axis=1).astype(F32)


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4), "max": round(float(ms.max()), 4),
            "samples": int(ms.size)}


def skin_table(scene, first, count, nbones, seed=1):
    """(bone_index, weights) of the mesh: by height.  2 bones: (1 - t, t, 0, 0); more: four non-zero weights over bones
    of a window of 8 around band t * (nbones - 8)."""
    y = scene.aos[first:first + count, :3, 1].reshape(-1)
    t = np.clip((y - y.min()) / (y.max() - y.min()), F32(0), F32(1)).astype(F32)
    idx = np.zeros((3 * count, 4), np.uint16)
    w = np.zeros((3 * count, 4), F32)
    if nbones == 2:
        idx[:, 1] = 1
        w[:, 0], w[:, 1] = F32(1) - t, t
        return idx, w
    rng = np.random.default_rng(seed)
    base = np.floor(t * (nbones - 8)).astype(np.int64)
    idx[:] = base[:, None] + rng.permuted(np.tile(np.arange(8), (3 * count, 1)), axis=1)[:, :4]
    r = rng.uniform(0.1, 1.0, (3 * count, 4))
    w[:] = (r / r.sum(axis=1, keepdims=True)).astype(F32)
    return idx, w


def bones_for(centre, nbones, angle):
    """Bone k turned by angle * k / (nbones - 1) about the vertical axis through the centre: a twist along the height."""
    return np.stack([turn(centre, angle * k / (nbones - 1)) for k in range(nbones)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--lon", type=int, default=250)
    ap.add_argument("--lat", type=int, default=201)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("skin_time.py measures on the GPU: no HIP device present")
    box = rt.Scene.cornell_box()
    path = os.path.join(tempfile.mkdtemp(), "m.obj")
    nf = meshgen.write_sphere_obj(path, a.lon, a.lat)
    scene = box + rt.Scene.load_obj(path)
    first, n = len(box), len(scene)
    centre = scene.aos[first:, :3, :3].reshape(-1, 3).mean(axis=0).astype(np.float64)
    cfg = abi.make_config(width=a.size, height=a.size, aa_x=1, aa_y=1, shadow_samples=1, spheres=())
    view = (rt.rotation_matrix(0.0, 0.0), [0.0, 0.0, -3.2], [0.0, -0.5, -0.7], 1100.0 * a.size / 1024)
    angles = [0.01 * (k + 1) for k in range(a.warmup + a.samples)]
    print(json.dumps({"triangles": n, "mesh": [first, nf], "size": a.size, "warmup": a.warmup,
                      "skin_table_bytes": 3 * nf * 24}), flush=True)
    stream = torch.cuda.Stream()

    def context():
        tr = rt.RayTracer(cfg, scene)
        for _ in range(5):                                    # warm clocks, a running context
            tr.render(*view)
        return tr

    def device_pose(pose, mats, kw):
        d = torch.from_numpy(mats).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pose(d, stream=stream, **kw)
        t1 = time.perf_counter()
        stream.synchronize()
        return ((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3)

    cases = []                                                # (label, fn(angle) -> times in ms, names of the times)
    open_ctx = []
    tables = {nb: skin_table(scene, first, nf, nb) for nb in (2, 256)}
    for nb in (2, 256):
        for flag, kw in (("0", {}), ("RT_UPDATE_DEVICE_TILES", {"device_tiles": True})):
            tr = context()
            tr.set_skin(first, nf, *tables[nb], nb)
            open_ctx.append(tr)
            cases.append(({"method": "skin_device", "nbones": nb, "flags": flag},
                          lambda x, tr=tr, nb=nb, kw=kw: device_pose(tr.pose_skin_device, bones_for(centre, nb, x), kw),
                          ("call_ms", "done_ms")))
    for flag, kw in (("0", {}), ("RT_UPDATE_DEVICE_TILES", {"device_tiles": True})):
        tr = context()
        tr.set_objects([(first, nf)])
        open_ctx.append(tr)
        cases.append(({"method": "objects_device", "flags": flag},
                      lambda x, tr=tr, kw=kw: device_pose(tr.pose_objects_device, turn(centre, x)[None], kw),
                      ("call_ms", "done_ms")))
    tr_up = context()
    open_ctx.append(tr_up)
    skinned = [scene.skinned(first, nf, *tables[2], bones_for(centre, 2, x)) for x in (0.1, 0.2)]   # made before the clock

    def host_update(x, state=[0]):
        state[0] ^= 1
        t0 = time.perf_counter()
        tr_up.update_scene(skinned[state[0]])
        return ((time.perf_counter() - t0) * 1e3,)

    cases.append(({"method": "host_update", "flags": "0"}, host_update, ("whole_ms",)))

    rows = [[] for _ in cases]
    for x in angles:                                          # the cases take turns
        for k, (_, fn, _) in enumerate(cases):
            rows[k].append(fn(x))
    for (label, _, names), r in zip(cases, rows):
        out = dict(label)
        for name, col in zip(names, zip(*r[a.warmup:])):
            out[name] = stats(col)
        print(json.dumps(out), flush=True)
    for tr in open_ctx:
        tr.close()


if __name__ == "__main__":
    main()
