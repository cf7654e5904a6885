"""Cost of the motion planes and of the accumulate call that takes them (rt_motion_planes_device,
rt_accumulate_plane_moving_device).

The planes are the position / normal / prim planes of the Cornell box (rt_render_aov_device, 1 sample per pixel) at --sizes
(1024 and 4096 squared) with the short block an object: the history is what two accumulate calls on the rest pose left, the
snapshot is the rest pose, and the block is then turned by 0.1 rad about its vertical axis and moved by (0.03, 0, 0.02).  Per
size, in ms per call:
  motion          rt_motion_planes_device, both outputs
  motion_torch    the same function written as a torch expression (gathers of the two scenes, elementwise FP32) on the same
                  GPU; its outputs are compared with the library's and the number of differing words is reported
  moving          rt_accumulate_plane_moving_device with the motion planes, all three outputs
  plain           rt_accumulate_plane_device on the same planes (it restarts the block's history)
  floors          motion: 68 bytes per element (read: prim 4, position4 16, normal4 16; written: two float4 planes, 32; the
                  triangles come from the caches) and moving: 176 bytes per pixel (the plain call's 144 and the two motion
                  planes), at the measured HBM copy rate of the microarchitecture guide, 6.29 TB/s; `x_floor` = time / floor
Device events on a stream of their own around each call; one unrecorded warm-up of every case, then the median of --samples
(7), with min and max.  The cases take turns sample by sample, so drift of the clocks hits all alike.
  python tools/motion_time.py [--sizes 1024 4096] [--samples 7] >> profiles/motion_time.txt"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uob_raytracer_amd import abi, runtime as rt   # noqa: E402

HBM_BYTES_PER_S = 6.29e12
MOTION_BYTES, MOVING_BYTES = 68, 176
CAM, LIGHT = [0.0, 0.0, -3.2], [0.0, -0.5, -0.7]
BLOCK = (10, 8)                         # the short block of the box
TURN, SHIFT = 0.1, (0.03, 0.0, 0.02)


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4), "max": round(float(ms.max()), 4)}


def torch_motion(torch, v_now, v_then, n_then, prim, pos, nrm):
    """The definition of include/uob_rt.h as a torch expression -> (prev_position4, prev_normal4)."""
    n = n_then.shape[0]
    ok = (pos[..., 3] > 0) & (prim >= -2) & (prim < n)
    tri = ok & (prim >= 0)
    t = torch.where(tri, prim, torch.zeros_like(prim)).to(torch.int64)
    now, then = v_now.reshape(n, 3, 4)[t], v_then.reshape(n, 3, 4)[t]
    same = (now[..., :3] == then[..., :3]).all(-1).all(-1)
    moved = tri & ~same
    a, b, c = (now[..., k, :3] for k in range(3))
    a0, b0, c0 = (then[..., k, :3] for k in range(3))
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    e1, e2, d, f1, f2 = b - a, c - a, pos[..., :3] - a, b0 - a0, c0 - a0
    d11, d12, d22, p1, p2 = dot(e1, e1), dot(e1, e2), dot(e2, e2), dot(d, e1), dot(d, e2)
    den = d11 * d22 - d12 * d12
    u = ((d22 * p1 - d12 * p2) / den)[..., None]
    v = ((d11 * p2 - d12 * p1) / den)[..., None]
    carried = (a0 + u * f1) + v * f2
    quiet = torch.tensor(0x7FC00000, dtype=torch.int32, device=pos.device).view(torch.float32)
    carried = torch.where(torch.isnan(carried), quiet, carried)
    one, zero = torch.ones_like(pos[..., :1]), torch.zeros_like(pos[..., :1])
    keep = (ok & ~moved)[..., None]
    out_p = torch.where(moved[..., None], torch.cat([carried, one], -1), torch.where(keep, pos, torch.zeros_like(pos)))
    out_n = torch.where(moved[..., None], torch.cat([n_then[t][..., :3], zero], -1), torch.where(keep, nrm, torch.zeros_like(nrm)))
    return out_p, out_n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--samples", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("motion_time.py measures on the GPU: no HIP device present")
    print(json.dumps({"hbm_bytes_per_s": HBM_BYTES_PER_S, "motion_floor_bytes_per_element": MOTION_BYTES,
                      "moving_floor_bytes_per_pixel": MOVING_BYTES, "samples": a.samples, "warmup": 1,
                      "pose": {"block": BLOCK, "turn": TURN, "shift": SHIFT}}), flush=True)
    stream = torch.cuda.Stream()
    scene = rt.Scene.cornell_box()
    centre = scene.aos[BLOCK[0]:BLOCK[0] + BLOCK[1], :3, :3].reshape(-1, 3).mean(axis=0).astype(np.float64)
    c, s = np.cos(TURN), np.sin(TURN)
    m = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    xform = np.concatenate([m, (np.asarray(SHIFT) + centre - m @ centre)[:, None]], 1).astype(np.float32)[None]
    for size in a.sizes:
        tr = rt.RayTracer(abi.make_config(width=size, height=size, aa_x=1, aa_y=1, shadow_samples=4), scene)
        tr.set_objects([BLOCK])
        focal, rot = 1100.0 * size / 1024, rt.rotation_matrix(0.0, 0.0)

        def planes_now():
            shape = (size, size)
            out = {"prim": torch.empty(shape, dtype=torch.int32, device="cuda"),
                   "position": torch.empty(shape + (4,), device="cuda"), "normal": torch.empty(shape + (4,), device="cuda")}
            tr.render_aov_device(rot, CAM, focal, out=out)
            _, _, vis, _ = tr.render_filtered_light(rot, CAM, LIGHT, focal, want_parts=True, passes=1)
            return vis, out["position"], out["normal"], out["prim"]

        v0, p0, n0, i0 = planes_now()
        prm = rt.accumulate_params(size, size, rot, CAM, focal)
        h1, _, _ = tr.accumulate_plane_device(v0, p0, n0, prim=i0, want_mean=False, want_variance=False, params=prm)
        prev, _, _ = tr.accumulate_plane_device(v0, p0, n0, prim=i0, prev=h1, want_mean=False, want_variance=False, params=prm)
        del h1, v0, p0, n0, i0
        then = tr.scene_data()
        tr.motion_snapshot()
        tr.pose_objects(xform)
        now = tr.scene_data()
        vis, pos, nrm, prim = planes_now()
        d_now, d_then, d_nthen = (torch.from_numpy(x).cuda() for x in (now["vertices"], then["vertices"], then["normals"]))
        rp, rn = torch.empty_like(pos), torch.empty_like(pos)
        nxt = torch.empty((size, size, 12), device="cuda")
        mean, var = torch.empty((size, size), device="cuda"), torch.empty((size, size), device="cuda")
        tr.motion_planes_device(prim, pos, nrm, out_position4=rp, out_normal4=rn)
        torch.cuda.synchronize()
        stream.wait_stream(torch.cuda.current_stream())

        def timed(fn):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                t0.record(stream)
                fn()
                t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1)

        cases = [
            ("motion", lambda: tr.motion_planes_device(prim, pos, nrm, out_position4=rp, out_normal4=rn, stream=stream)),
            ("motion_torch", lambda: torch_motion(torch, d_now, d_then, d_nthen, prim, pos, nrm)),
            ("moving", lambda: tr.accumulate_plane_device(vis, pos, nrm, prim=prim, prev=prev, next=nxt, out_mean=mean, out_variance=var,
                                                          stream=stream, params=prm, reproj_position4=rp, reproj_normal4=rn)),
            ("plain", lambda: tr.accumulate_plane_device(vis, pos, nrm, prim=prim, prev=prev, next=nxt, out_mean=mean, out_variance=var,
                                                         stream=stream, params=prm)),
        ]
        rows = {label: [] for label, _ in cases}
        for k in range(1 + a.samples):                        # the first round is the warm-up; the cases take turns
            for label, fn in cases:
                ms = timed(fn)
                if k:
                    rows[label].append(ms)
        with torch.cuda.stream(stream):
            tr.motion_planes_device(prim, pos, nrm, out_position4=rp, out_normal4=rn, stream=stream)
            ref = torch_motion(torch, d_now, d_then, d_nthen, prim, pos, nrm)
        stream.synchronize()
        motion_stats = tr.motion_stats()
        differs = sum(int((x.contiguous().view(torch.int32) != y.contiguous().view(torch.int32)).sum()) for x, y in zip((rp, rn), ref))
        del ref
        with torch.cuda.stream(stream):
            cases[2][1]()
        stream.synchronize()
        moving_stats = tr.accumulate_stats()
        with torch.cuda.stream(stream):
            cases[3][1]()
        stream.synchronize()
        plain_stats = tr.accumulate_stats()
        px = size * size
        floor_motion, floor_moving = MOTION_BYTES * px / HBM_BYTES_PER_S * 1e3, MOVING_BYTES * px / HBM_BYTES_PER_S * 1e3
        ms = {label: stats(r) for label, r in rows.items()}
        print(json.dumps({"size": size, "motion_ms": ms["motion"], "motion_floor_ms": round(floor_motion, 4),
                          "motion_x_floor": round(ms["motion"]["median"] / floor_motion, 2), "motion_torch_ms": ms["motion_torch"],
                          "torch_over_device": round(ms["motion_torch"]["median"] / ms["motion"]["median"], 1),
                          "words_torch_differs": differs, "motion_stats": motion_stats}), flush=True)
        print(json.dumps({"size": size, "moving_ms": ms["moving"], "moving_floor_ms": round(floor_moving, 4),
                          "moving_x_floor": round(ms["moving"]["median"] / floor_moving, 2), "plain_ms": ms["plain"],
                          "moving_over_plain": round(ms["moving"]["median"] / ms["plain"]["median"], 2),
                          "found_history_moving": moving_stats["found_history"], "found_history_plain": plain_stats["found_history"],
                          "valid_pixels": moving_stats["valid_pixels"]}), flush=True)
        tr.close()
        del vis, pos, nrm, prim, prev, rp, rn, nxt, mean, var
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
