"""Device time of the AOV pass (rt_render_aov_device) from stream events: warm-up 3, median of --reps (>= 10) single passes.

  mesh      box + a meshgen.write_sphere_obj(path, 256, 196) mesh (99 840 + 26 triangles), 2048^2, 1x1 AA, 1 shadow sample, no
            spheres: the pass (sample 0, all planes) next to rt_last_kernel_ms of the frame of the same view and next to
            rt_trace_rays_device fed the pass's own direction plane as rays (2^22 rays); and the pass with RT_FLAG_NO_TILE_BINS
  headline  the box at 4096^2, 4x2 AA: sample 0 with prim + depth only; all planes of all samples (8 x 72 B x 16.8 M written:
            bound by the stores), with the achieved store bandwidth
One JSON line per measurement.  usage: python tools/aov_time.py [--reps 10] [--only mesh|headline] > profiles/aov_time.txt"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from uob_raytracer_amd import abi, meshgen, runtime as rt  # noqa: E402

CAM = [0.0, 0.0, -3.2]
LIGHT = [0.0, -0.5, -0.7]
PLANES = ("prim", "depth", "position", "normal", "albedo", "direction")
BYTES = {"prim": 4, "depth": 4, "position": 16, "normal": 16, "albedo": 16, "direction": 16}


def median_ms(torch, stream, fn, reps, after=None):
    """Median over `reps` calls of fn (3 warm-up calls first), each between two events on `stream`; after() (e.g.
    rt_last_kernel_ms) replaces the events' figure when given."""
    ts = []
    for i in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        if i >= 3:
            ts.append(after() if after else e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def planes_on_device(torch, tr, names, sample):
    return {n: torch.empty(tr._aov_shape(n, sample), dtype=torch.int32 if n == "prim" else torch.float32, device="cuda")
            for n in names}


def focal_of(cfg):
    return 1100.0 * min(cfg.width, cfg.height) / 1024.0 * cfg.aa_x


def report(**kw):
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in kw.items()}), flush=True)


def run_mesh(torch, reps):
    box = rt.Scene.cornell_box()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.obj")
        meshgen.write_sphere_obj(path, 256, 196)
        scene = box + rt.Scene.load_obj(path)
    kw = dict(width=2048, height=2048, aa_x=1, aa_y=1, shadow_samples=1, spheres=())
    rot = rt.rotation_matrix(0.0, 0.0)
    s = torch.cuda.Stream()
    res = {}
    for label, flags in (("bins", 0), ("no_tile_bins", abi.RT_FLAG_NO_TILE_BINS)):
        cfg = abi.make_config(flags=flags, **kw)
        tr = rt.RayTracer(cfg, scene)
        out = planes_on_device(torch, tr, PLANES, 0)
        med, lo, hi = median_ms(torch, s, lambda: tr.render_aov_device(rot, CAM, focal_of(cfg), 0, out, stream=s), reps)
        res[label] = med
        report(config="box+mesh 2048^2 1x1", triangles=len(scene), what="aov pass, sample 0, all planes", context=label,
               median_ms=med, min_ms=lo, max_ms=hi, stats=tr.aov_stats())
        if flags == 0:
            argb = torch.empty((2048, 2048), dtype=torch.int32, device="cuda")
            fmed, flo, fhi = median_ms(torch, s, lambda: tr.render_device(rot, CAM, LIGHT, focal_of(cfg), argb.data_ptr(), stream=s.cuda_stream),
                                       reps, after=tr.last_kernel_ms)
            report(config="box+mesh 2048^2 1x1", what="frame, rt_last_kernel_ms (1 shadow sample)", median_ms=fmed, min_ms=flo, max_ms=fhi,
                   aov_over_frame=med / fmed)
            k = 2048 * 2048
            rays = torch.empty((k, 6), dtype=torch.float32, device="cuda")
            rays[:, 0:3] = torch.tensor(CAM, dtype=torch.float32, device="cuda")
            rays[:, 3:6] = out["direction"].reshape(k, 4)[:, 0:3]
            tri = torch.empty(k, dtype=torch.int32, device="cuda")
            out10 = torch.empty((k, 10), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            qmed, qlo, qhi = median_ms(torch, s, lambda: tr.query_device(abi.RT_TRACE_CLOSEST_HIT, rays, None, tri, out10, stream=s), reps)
            same = bool(torch.equal(tri, out["prim"].reshape(k)))
            report(config="box+mesh 2048^2 1x1", what="rt_trace_rays_device on the pass's direction plane (2^22 rays)", median_ms=qmed,
                   min_ms=qlo, max_ms=qhi, aov_over_query=med / qmed, same_prim=same, stats=tr.trace_stats())
        tr.close()


def run_headline(torch, reps):
    cfg = abi.make_config(width=4096, height=4096, aa_x=4, aa_y=2, shadow_samples=64)
    tr = rt.RayTracer(cfg, rt.Scene.cornell_box())
    rot = rt.rotation_matrix(0.0, 0.0)
    s = torch.cuda.Stream()
    for what, names, sample in (("sample 0, prim + depth", ("prim", "depth"), 0), ("all samples, all planes", PLANES, None)):
        out = planes_on_device(torch, tr, names, sample)
        med, lo, hi = median_ms(torch, s, lambda: tr.render_aov_device(rot, CAM, focal_of(cfg), sample, out, stream=s), reps)
        written = sum(BYTES[n] for n in names) * 4096 * 4096 * (8 if sample is None else 1)
        report(config="box 4096^2 4x2", what="aov pass, " + what, median_ms=med, min_ms=lo, max_ms=hi, bytes_written=written,
               store_GBps=written / med / 1e6)
        del out
    argb = torch.empty((4096, 4096), dtype=torch.int32, device="cuda")
    fmed, flo, fhi = median_ms(torch, s, lambda: tr.render_device(rot, CAM, LIGHT, focal_of(cfg), argb.data_ptr(), stream=s.cuda_stream),
                               reps, after=tr.last_kernel_ms)
    report(config="box 4096^2 4x2", what="frame, rt_last_kernel_ms (64 shadow samples)", median_ms=fmed, min_ms=flo, max_ms=fhi)
    tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=("mesh", "headline"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    if a.only != "headline":
        run_mesh(torch, a.reps)
    if a.only != "mesh":
        run_headline(torch, a.reps)


if __name__ == "__main__":
    main()
