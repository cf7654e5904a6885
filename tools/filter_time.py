"""Cost and effect of the a-trous filter (rt_filter_plane_device).

Timing: the guides are the position / normal planes of the default view of the Cornell box (rt_render_aov_device, 1 sample
per pixel), the value plane is the visibility of 4 shadow samples (render_filtered_light's V), at --sizes (1024 and 4096
squared) and 1, 5 and 8 passes, default edge stops.  Per size and pass count four figures, in ms per call:
  built_in   the library as it ships: passes of spacing <= 32 staged in LDS, the others from the caches
  direct     a context made under UOB_RT_FILTER_FORM=direct: every pass takes its taps from the caches
  torch      the same filter written as a torch expression (25 shifted views per pass, elementwise FP32) on the same GPU; its
             output is compared with the library's and the number of differing pixels is reported
  floor      40 bytes per pixel and pass (a record, a value read, a value written) at the measured HBM copy rate of the
             microarchitecture guide, 6.29 TB/s; `x_floor` = built_in / floor.  The guide packing of a call (64 bytes per
             pixel, once) is part of built_in and direct and not of the floor.
Device events on a stream of their own around each call; one unrecorded warm-up of every case, then the median of --samples
(7), with min and max.  The cases take turns sample by sample, so drift of the clocks hits all alike.

Quality: the default view at 256 x 256, shadow_samples S = 4, 8 and 16 against the 64-sample light of the same points
(render_direct_light of a 64-sample context): RMS error over the pixels whose primary hit is diffuse, of term * V (before) and
of render_filtered_light (after), default edge stops; beside it the same with value_max_diff = 0.25 and with 2 passes.
Reported whichever way it comes out.
  python tools/filter_time.py [--sizes 1024 4096] [--samples 7] > profiles/filter_time.txt"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uob_raytracer_amd import abi, runtime as rt   # noqa: E402

HBM_BYTES_PER_S = 6.29e12
CAM, LIGHT = [0.0, 0.0, -3.2], [0.0, -0.5, -0.7]
TAP = (0.375, 0.25, 0.0625)


def view_of(size):
    return (rt.rotation_matrix(0.0, 0.0), CAM, LIGHT, 1100.0 * size / 1024)


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4), "max": round(float(ms.max()), 4)}


def torch_filter(torch, value, pos, nrm, passes, nmin=0.9, eps=0.01):
    """The definition of include/uob_rt.h as a torch expression (value_max_diff = +INF: condition 4 is 'not NaN')."""
    h, w = value.shape
    valid = pos[..., 3] > 0
    yy = torch.arange(h, device=value.device)[:, None]
    xx = torch.arange(w, device=value.device)[None, :]
    P, N = pos[..., :3], nrm[..., :3]
    v = value
    quiet = torch.tensor(0x7FC00000, dtype=torch.int32, device=value.device).view(torch.float32)
    for i in range(passes):
        s = 1 << i
        num, den = torch.zeros_like(v), torch.zeros_like(v)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                wt = TAP[abs(dx)] * TAP[abs(dy)]
                if dx == 0 and dy == 0:
                    vq, acc = v, valid
                else:
                    oy, ox = dy * s, dx * s
                    inside = (yy + oy >= 0) & (yy + oy < h) & (xx + ox >= 0) & (xx + ox < w)
                    vq = torch.roll(v, (-oy, -ox), (0, 1))
                    Pq, Nq = torch.roll(P, (-oy, -ox), (0, 1)), torch.roll(N, (-oy, -ox), (0, 1))
                    acc = valid & inside & torch.roll(valid, (-oy, -ox), (0, 1))
                    acc &= ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]) >= nmin
                    d = Pq - P
                    acc &= ((N[..., 0] * d[..., 0] + N[..., 1] * d[..., 1]) + N[..., 2] * d[..., 2]).abs() <= eps
                    acc &= (vq - v).abs() <= float("inf")
                num = torch.where(acc, num + wt * vq, num)
                den = torch.where(acc, den + wt, den)
        q = num / den
        q = torch.where(torch.isnan(q), quiet, q)
        v = torch.where(valid & (den != 0.140625), q, v)
    return v


def timing(torch, a):
    os.environ.pop("UOB_RT_FILTER_FORM", None)
    stream = torch.cuda.Stream()
    scene = rt.Scene.cornell_box()
    for size in a.sizes:
        cfg = abi.make_config(width=size, height=size, aa_x=1, aa_y=1, shadow_samples=4)
        tr = rt.RayTracer(cfg, scene)
        os.environ["UOB_RT_FILTER_FORM"] = "direct"
        tr_direct = rt.RayTracer(cfg, scene)
        del os.environ["UOB_RT_FILTER_FORM"]
        planes = {"position": torch.empty((size, size, 4), device="cuda"), "normal": torch.empty((size, size, 4), device="cuda")}
        tr.render_aov_device(*view_of(size)[:2], view_of(size)[3], out=planes)
        _, _, vis, _ = tr.render_filtered_light(*view_of(size), want_parts=True, passes=1)
        pos, nrm = planes["position"], planes["normal"]
        out = torch.empty_like(vis)
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
        for passes in (1, 5, 8):
            cases.append((("built_in", passes), lambda p=passes: tr.filter_plane_device(vis, pos, nrm, out=out, stream=stream, passes=p)))
            cases.append((("direct", passes), lambda p=passes: tr_direct.filter_plane_device(vis, pos, nrm, out=out, stream=stream, passes=p)))
            cases.append((("torch", passes), lambda p=passes: torch_filter(torch, vis, pos, nrm, p)))
        rows = {label: [] for label, _ in cases}
        for k in range(1 + a.samples):                        # the first round is the warm-up; the cases take turns
            for label, fn in cases:
                ms = timed(fn)
                if k:
                    rows[label].append(ms)
        for passes in (1, 5, 8):
            with torch.cuda.stream(stream):
                ours = tr.filter_plane_device(vis, pos, nrm, stream=stream, passes=passes)
                other = tr_direct.filter_plane_device(vis, pos, nrm, stream=stream, passes=passes)
                ref = torch_filter(torch, vis, pos, nrm, passes)
            stream.synchronize()
            floor = 40.0 * size * size * passes / HBM_BYTES_PER_S * 1e3
            b = stats(rows[("built_in", passes)])
            print(json.dumps({"size": size, "passes": passes, "built_in_ms": b, "direct_ms": stats(rows[("direct", passes)]),
                              "torch_ms": stats(rows[("torch", passes)]), "floor_ms": round(floor, 4),
                              "x_floor": round(b["median"] / floor, 2),
                              "pixels_direct_differs": int((ours.view(torch.int32) != other.view(torch.int32)).sum()),
                              "pixels_torch_differs": int((ours.view(torch.int32) != ref.view(torch.int32)).sum()),
                              "filter_stats": tr.filter_stats()}), flush=True)
        tr.close()
        tr_direct.close()
        del planes, pos, nrm, vis, out
        torch.cuda.empty_cache()


def quality(torch):
    size = 256
    scene = rt.Scene.cornell_box()
    view = view_of(size)

    def ctx(s):
        return rt.RayTracer(abi.make_config(width=size, height=size, aa_x=1, aa_y=1, shadow_samples=s), scene)

    ref_tr = ctx(64)
    ref = ref_tr.render_direct_light(*view).cpu().numpy().astype(np.float64)
    aov = ref_tr.render_aov(view[0], view[1], view[3], planes=("prim", "albedo"))
    diffuse = (aov["prim"] != -1) & (aov["albedo"][..., 3] > 0)
    ref_tr.close()
    for s in (4, 8, 16):
        tr = ctx(s)
        out, term, vis, vis_f = (t.cpu().numpy().astype(np.float64) for t in tr.render_filtered_light(*view, want_parts=True))
        before = term * vis
        stopped = tr.render_filtered_light(*view, value_max_diff=0.25).cpu().numpy().astype(np.float64)
        short = tr.render_filtered_light(*view, passes=2).cpu().numpy().astype(np.float64)
        rms = lambda x: float(np.sqrt(np.mean((x[diffuse] - ref[diffuse]) ** 2)))
        print(json.dumps({"quality": "256x256 default view", "shadow_samples": s, "diffuse_pixels": int(diffuse.sum()),
                          "rms_before": round(rms(before), 6), "rms_after": round(rms(out), 6),
                          "rms_after_value_max_diff_0.25": round(rms(stopped), 6), "rms_after_2_passes": round(rms(short), 6),
                          "mean_light_64": round(float(ref[diffuse].mean()), 6),
                          "penumbra_pixels": int(((vis > 0) & (vis < 1) & diffuse).sum())}), flush=True)
        tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--samples", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filter_time.py measures on the GPU: no HIP device present")
    print(json.dumps({"hbm_bytes_per_s": HBM_BYTES_PER_S, "floor_bytes_per_pixel_and_pass": 40, "samples": a.samples, "warmup": 1,
                      "tile": [64, 4], "tiled_up_to_spacing": 32}), flush=True)
    timing(torch, a)
    quality(torch)


if __name__ == "__main__":
    main()
