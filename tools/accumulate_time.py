"""Cost and effect of the temporal reprojection (rt_accumulate_plane_device).

Timing: the guides are the position / normal / prim planes of the Cornell box (rt_render_aov_device, 1 sample per pixel), the
value plane is the visibility of 4 shadow samples, the history is what two accumulate calls on the previous view left, at
--sizes (1024 and 4096 squared), for a still view (previous view = the default view) and for a small pan (yaw 0.02 rad and a
translation of (0.02, 0, 0.03) from it).  Per size and case three figures, in ms per call:
  device     rt_accumulate_plane_device as it ships, all three outputs
  torch      the same function written as a torch expression (four gathers of the history, elementwise FP32) on the same GPU;
             its history, mean and variance are compared with the library's and the number of differing words is reported
  floor      144 bytes per pixel (read: value 4, position4 16, normal4 16, prim 4, one history record 48; written: a history
             record 48, mean 4, variance 4) at the measured HBM copy rate of the microarchitecture guide, 6.29 TB/s;
             `x_floor` = device / floor
Device events on a stream of their own around each call; one unrecorded warm-up of every case, then the median of --samples
(7), with min and max.  The cases take turns sample by sample, so drift of the clocks hits all alike.

Quality: the default view at 256 x 256, still, S = 1 and 4 shadow samples per frame, light_spread as shipped (0.05) and wider
(0.3): after K = 1, 2, 4, 8, 16, 32 frames of render_accumulated_light the RMS error of term * V_mean against the 64-sample
light of the same points (render_direct_light of a 64-sample context), over the pixels whose primary hit is diffuse.
Reported whichever way it comes out.
  python tools/accumulate_time.py [--sizes 1024 4096] [--samples 7] > profiles/accumulate_time.txt"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uob_raytracer_amd import abi, runtime as rt   # noqa: E402

HBM_BYTES_PER_S = 6.29e12
FLOOR_BYTES_PER_PIXEL = 144
CAM, LIGHT = [0.0, 0.0, -3.2], [0.0, -0.5, -0.7]
PAN_YAW, PAN_CAM = 0.02, [0.02, 0.0, -3.17]
FRAMES = (1, 2, 4, 8, 16, 32)


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4), "max": round(float(ms.max()), 4)}


def torch_accumulate(torch, value, pos, nrm, prim, prev, p):
    """The definition of include/uob_rt.h as a torch expression -> (next [h, w, 12], mean, variance)."""
    h, w = value.shape
    dev = value.device
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)
    quiet = torch.tensor(0x7FC00000, dtype=torch.int32, device=dev).view(torch.float32)
    rot, cam = [float(x) for x in p.prev_rot], [float(x) for x in p.prev_cam]
    valid = pos[..., 3] > 0
    P, N = [pos[..., k] for k in range(3)], [nrm[..., k] for k in range(3)]
    d = [P[k] - cam[k] for k in range(3)]
    q = [(d[0] * rot[j] + d[1] * rot[4 + j]) + d[2] * rot[8 + j] for j in range(3)]
    fx = (q[0] * p.prev_focal_px) / q[2] + 0.5 * float(w)
    fy = (q[1] * p.prev_focal_px) / q[2] + 0.5 * float(h)
    cand = valid & (q[2] > 0) & (fx >= -1) & (fx < float(w)) & (fy >= -1) & (fy < float(h))
    xf, yf = torch.floor(fx), torch.floor(fy)
    ax, ay = fx - xf, fy - yf
    bx, by = 1.0 - ax, 1.0 - ay
    x0 = torch.where(cand, xf, torch.zeros_like(xf)).to(torch.int64)
    y0 = torch.where(cand, yf, torch.zeros_like(yf)).to(torch.int64)
    num, num2, den = torch.zeros_like(value), torch.zeros_like(value), torch.zeros_like(value)
    cmin = torch.full_like(value, float("inf"))
    found = torch.zeros_like(valid)
    flat = prev.reshape(h * w, 12)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            wt = (ax if i else bx) * (ay if j else by)
            acc = cand & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (wt > 0)
            r = flat[(qy.clamp(0, h - 1) * w + qx.clamp(0, w - 1)).reshape(-1)].reshape(h, w, 12)
            acc &= r[..., 8] > 0
            acc &= r[..., 9].view(torch.int32) == prim
            acc &= ((N[0] * r[..., 4] + N[1] * r[..., 5]) + N[2] * r[..., 6]) >= p.normal_min_dot
            e = [r[..., k] - P[k] for k in range(3)]
            acc &= ((N[0] * e[0] + N[1] * e[1]) + N[2] * e[2]).abs() <= p.plane_eps
            num = torch.where(acc, num + wt * r[..., 3], num)
            num2 = torch.where(acc, num2 + wt * r[..., 7], num2)
            den = torch.where(acc, den + wt, den)
            cmin = torch.where(acc & (r[..., 8] < cmin), r[..., 8], cmin)
            found |= acc
    vv = value * value
    mp, sp = num / den, num2 / den
    nmax = f32(float(p.max_history - 1))
    n = torch.where(cmin < nmax, cmin, nmax) + 1.0
    a = torch.ones_like(n) / n                           # (a division, not a reciprocal instruction)
    mean5 = mp + a * (value - mp)
    m25 = sp + a * (vv - sp)
    mean = torch.where(found, torch.where(torch.isnan(mean5), quiet, mean5), value)
    m2 = torch.where(found, m25, vv)
    m2 = torch.where(torch.isnan(m2), quiet, m2)
    count = torch.where(found, n, valid.to(torch.float32))
    t = m2 - mean * mean
    var = torch.where(t > 0, t, torch.zeros_like(t))
    zero = torch.zeros_like(value)
    nxt = torch.stack([P[0], P[1], P[2], mean, N[0], N[1], N[2], m2, count, prim.view(torch.float32), zero, zero], -1)
    return nxt, mean, var


def timing(torch, a):
    stream = torch.cuda.Stream()
    scene = rt.Scene.cornell_box()
    for size in a.sizes:
        cfg = abi.make_config(width=size, height=size, aa_x=1, aa_y=1, shadow_samples=4)
        tr = rt.RayTracer(cfg, scene)
        focal = 1100.0 * size / 1024
        rot0 = rt.rotation_matrix(0.0, 0.0)

        def planes_of(rot, cam):
            shape = (size, size)
            out = {"prim": torch.empty(shape, dtype=torch.int32, device="cuda"),
                   "position": torch.empty(shape + (4,), device="cuda"), "normal": torch.empty(shape + (4,), device="cuda")}
            tr.render_aov_device(rot, cam, focal, out=out)
            _, _, vis, _ = tr.render_filtered_light(rot, cam, LIGHT, focal, want_parts=True, passes=1)
            return vis, out["position"], out["normal"], out["prim"]

        # the history: two frames of the previous (default) view
        v0, p0, n0, i0 = planes_of(rot0, CAM)
        prm0 = rt.accumulate_params(size, size, rot0, CAM, focal)
        h1, _, _ = tr.accumulate_plane_device(v0, p0, n0, prim=i0, want_mean=False, want_variance=False, params=prm0)
        prev, _, _ = tr.accumulate_plane_device(v0, p0, n0, prim=i0, prev=h1, want_mean=False, want_variance=False, params=prm0)
        del h1
        views = {"still": (v0, p0, n0, i0), "pan": planes_of(rt.rotation_matrix(PAN_YAW, 0.0), PAN_CAM)}
        nxt = torch.empty((size, size, 12), device="cuda")
        mean, var = torch.empty((size, size), device="cuda"), torch.empty((size, size), device="cuda")
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

        cases = []
        for name, (v, p, n, i) in views.items():
            cases.append((("device", name), lambda v=v, p=p, n=n, i=i: tr.accumulate_plane_device(
                v, p, n, prim=i, prev=prev, next=nxt, out_mean=mean, out_variance=var, stream=stream, params=prm0)))
            cases.append((("torch", name), lambda v=v, p=p, n=n, i=i: torch_accumulate(torch, v, p, n, i, prev, prm0)))
        rows = {label: [] for label, _ in cases}
        for k in range(1 + a.samples):                        # the first round is the warm-up; the cases take turns
            for label, fn in cases:
                ms = timed(fn)
                if k:
                    rows[label].append(ms)
        floor = FLOOR_BYTES_PER_PIXEL * size * size / HBM_BYTES_PER_S * 1e3
        for name, (v, p, n, i) in views.items():
            with torch.cuda.stream(stream):
                ours = tr.accumulate_plane_device(v, p, n, prim=i, prev=prev, stream=stream, params=prm0)
                ref = torch_accumulate(torch, v, p, n, i, prev, prm0)
            stream.synchronize()
            differs = sum(int((x.contiguous().view(torch.int32) != y.contiguous().view(torch.int32)).sum()) for x, y in zip(ours, ref))
            dms = stats(rows[("device", name)])
            tms = stats(rows[("torch", name)])
            print(json.dumps({"size": size, "view": name, "device_ms": dms, "torch_ms": tms, "floor_ms": round(floor, 4),
                              "x_floor": round(dms["median"] / floor, 2), "torch_over_device": round(tms["median"] / dms["median"], 1),
                              "words_torch_differs": differs, "accumulate_stats": tr.accumulate_stats()}), flush=True)
            del ours, ref
        tr.close()
        del views, prev, nxt, mean, var, v0, p0, n0, i0
        torch.cuda.empty_cache()


def quality(torch):
    size = 256
    scene = rt.Scene.cornell_box()
    view = (rt.rotation_matrix(0.0, 0.0), CAM, LIGHT, 1100.0 * size / 1024)

    def ctx(s, spread):
        return rt.RayTracer(abi.make_config(width=size, height=size, aa_x=1, aa_y=1, shadow_samples=s, light_spread=spread), scene)

    for spread in (0.05, 0.3):
        ref_tr = ctx(64, spread)
        ref = ref_tr.render_direct_light(*view).cpu().numpy().astype(np.float64)
        aov = ref_tr.render_aov(view[0], view[1], view[3], planes=("prim", "albedo"))
        diffuse = (aov["prim"] != -1) & (aov["albedo"][..., 3] > 0)
        ref_tr.close()
        rms = lambda x: float(np.sqrt(np.mean((x[diffuse] - ref[diffuse]) ** 2)))
        for s in (1, 4):
            tr = ctx(s, spread)
            row = {"quality": "256x256 default view, still", "light_spread": spread, "shadow_samples": s,
                   "diffuse_pixels": int(diffuse.sum()), "mean_light_64": round(float(ref[diffuse].mean()), 6)}
            for k in range(1, max(FRAMES) + 1):
                out, term, vis, vis_m, var, count = tr.render_accumulated_light(*view, want_parts=True)
                if k == 1:
                    row["penumbra_pixels_frame_1"] = int(((vis > 0) & (vis < 1)).cpu().numpy()[diffuse].sum())
                if k in FRAMES:
                    row["rms_after_%d" % k] = round(rms(out.cpu().numpy().astype(np.float64)), 6)
            row["rms_single_frame_32"] = round(rms((term * vis).cpu().numpy().astype(np.float64)), 6)
            row["rms_after_33_filtered"] = round(rms(tr.render_accumulated_light(*view, filter=True).cpu().numpy().astype(np.float64)), 6)
            print(json.dumps(row), flush=True)
            tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--samples", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("accumulate_time.py measures on the GPU: no HIP device present")
    print(json.dumps({"hbm_bytes_per_s": HBM_BYTES_PER_S, "floor_bytes_per_pixel": FLOOR_BYTES_PER_PIXEL, "samples": a.samples,
                      "warmup": 1, "tile": [64, 4], "pan": {"yaw": PAN_YAW, "cam": PAN_CAM}}), flush=True)
    timing(torch, a)
    quality(torch)


if __name__ == "__main__":
    main()
