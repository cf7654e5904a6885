"""Cost and effect of the variance-guided a-trous filter (rt_filter_plane_variance_device, DESIGN.md 4.8a').

Timing: tools/filter_time.py's planes — the guides are the position / normal planes of the default view of the Cornell box
(rt_render_aov_device, 1 sample per pixel), the value plane is the visibility of 4 shadow samples — and as variance the
binomial V (1 - V) / 4 of that visibility, at --sizes (1024 and 4096 squared) and 1, 5 and 8 passes, default stops.  Per size
and pass count, in ms per call:
  variance          the variance call as it ships: passes of spacing <= 32 staged in LDS, the others from the caches
  variance_direct   a context made under UOB_RT_FILTER_FORM=direct: every pass takes its taps from the caches
  plain, plain_direct   rt_filter_plane_device on the same planes, in the same two contexts
  floor             60 bytes per pixel and pass (the pass reads a record 32, V 4, Var 4 and T 4 and writes V and Var 8; the
                    threshold launch reads Var 4 and writes T 4) at the measured HBM copy rate of the microarchitecture guide,
                    6.29 TB/s; `x_floor` = variance / floor.  The guide packing of a call (64 bytes per pixel, once) is part of
                    the measured times and not of the floor.
Device events on a stream of their own around each call; one unrecorded warm-up of every case, then the median of --samples
(7), with min and max.  The cases take turns sample by sample, so drift of the clocks hits all alike.

Quality: DESIGN.md 4.8a's protocol on the accumulated estimate — the default view at 256 x 256, shadow_samples 4, against the
64-sample light of the same points (render_direct_light of a 64-sample context), RMS error over the pixels whose primary hit
is diffuse, after 8 and after 32 frames of render_accumulated_light on the still view: of term * V_mean (unfiltered), of
V_mean under rt_filter_plane's defaults and under value_max_diff = 0.25, and of (V_mean, variance) under the variance-guided
filter at sigma_value 1, 2 and 4.  Reported whichever way it comes out.
  python tools/filter_variance_time.py [--sizes 1024 4096] [--samples 7] > profiles/filter_variance_time.txt"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uob_raytracer_amd import abi, runtime as rt   # noqa: E402

HBM_BYTES_PER_S = 6.29e12
FLOOR_BYTES = 60
CAM, LIGHT = [0.0, 0.0, -3.2], [0.0, -0.5, -0.7]


def view_of(size):
    return (rt.rotation_matrix(0.0, 0.0), CAM, LIGHT, 1100.0 * size / 1024)


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4), "max": round(float(ms.max()), 4)}


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
        var = (vis * (1.0 - vis) / 4.0).contiguous()
        out, out_var = torch.empty_like(vis), torch.empty_like(vis)
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
            for name, ctx in (("variance", tr), ("variance_direct", tr_direct)):
                cases.append(((name, passes), lambda p=passes, c=ctx: c.filter_plane_variance_device(
                    vis, var, pos, nrm, out=out, out_variance=out_var, stream=stream, passes=p)))
            for name, ctx in (("plain", tr), ("plain_direct", tr_direct)):
                cases.append(((name, passes), lambda p=passes, c=ctx: c.filter_plane_device(vis, pos, nrm, out=out, stream=stream, passes=p)))
        rows = {label: [] for label, _ in cases}
        for k in range(1 + a.samples):                        # the first round is the warm-up; the cases take turns
            for label, fn in cases:
                ms = timed(fn)
                if k:
                    rows[label].append(ms)
        for passes in (1, 5, 8):
            with torch.cuda.stream(stream):
                ours = tr.filter_plane_variance_device(vis, var, pos, nrm, stream=stream, passes=passes)
                other = tr_direct.filter_plane_variance_device(vis, var, pos, nrm, stream=stream, passes=passes)
            stream.synchronize()
            differs = sum(int((x.view(torch.int32) != y.view(torch.int32)).sum()) for x, y in zip(ours, other))
            floor = float(FLOOR_BYTES) * size * size * passes / HBM_BYTES_PER_S * 1e3
            v, p = stats(rows[("variance", passes)]), stats(rows[("plain", passes)])
            print(json.dumps({"size": size, "passes": passes, "variance_ms": v, "variance_direct_ms": stats(rows[("variance_direct", passes)]),
                              "plain_ms": p, "plain_direct_ms": stats(rows[("plain_direct", passes)]), "floor_ms": round(floor, 4),
                              "x_floor": round(v["median"] / floor, 2), "x_plain": round(v["median"] / p["median"], 2),
                              "words_direct_differs": differs, "filter_stats": tr.filter_variance_stats()}), flush=True)
        tr.close()
        tr_direct.close()
        del planes, pos, nrm, vis, var, out, out_var
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
    rms = lambda x: float(np.sqrt(np.mean((x.cpu().numpy().astype(np.float64)[diffuse] - ref[diffuse]) ** 2)))
    tr = ctx(4)
    planes = {k: torch.from_numpy(v).cuda() for k, v in tr.render_aov(view[0], view[1], view[3], planes=("position", "normal")).items()}
    pos, nrm = planes["position"], planes["normal"]
    hit = pos[..., 3] > 0
    frames = 0
    for target in (8, 32):
        while frames < target:
            out, term, vis, vis_m, var, count = tr.render_accumulated_light(*view, want_parts=True)
            frames += 1
        light = lambda v: term * torch.where(hit, v, torch.zeros_like(v))
        row = {"quality": "256x256 default view, shadow_samples 4", "frames": frames, "diffuse_pixels": int(diffuse.sum()),
               "rms_unfiltered": round(rms(out), 6),
               "rms_plain_defaults": round(rms(light(tr.filter_plane_device(vis_m, pos, nrm))), 6),
               "rms_plain_value_max_diff_0.25": round(rms(light(tr.filter_plane_device(vis_m, pos, nrm, value_max_diff=0.25))), 6)}
        for sigma in (1.0, 2.0, 4.0):
            v, _ = tr.filter_plane_variance_device(vis_m, var, pos, nrm, sigma_value=sigma)
            row["rms_variance_sigma_%g" % sigma] = round(rms(light(v)), 6)
            row["variance_stopped_sigma_%g" % sigma] = tr.filter_variance_stats()["variance_stopped"]
        row["mean_light_64"] = round(float(ref[diffuse].mean()), 6)
        row["penumbra_pixels"] = int(((vis_m > 0) & (vis_m < 1)).cpu().numpy()[diffuse].sum())
        row["mean_variance"] = round(float(var.cpu().numpy()[diffuse].mean()), 6)
        print(json.dumps(row), flush=True)
    tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--samples", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filter_variance_time.py measures on the GPU: no HIP device present")
    print(json.dumps({"hbm_bytes_per_s": HBM_BYTES_PER_S, "floor_bytes_per_pixel_and_pass": FLOOR_BYTES, "samples": a.samples,
                      "warmup": 1, "tile": [64, 4], "tiled_up_to_spacing": 32}), flush=True)
    timing(torch, a)
    quality(torch)


if __name__ == "__main__":
    main()
