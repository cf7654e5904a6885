"""rt_shade_points_device against what a caller could do before it existed: the jittered sample rays of every point built by
a torch expression on the device, rt_trace_rays_device(RT_TRACE_IN_SHADOW) on them, and a torch reduction of the answers.

Cases: the box, 1024^2 points taken from an AOV pass of the default view (2^20 points), and the box + a
meshgen.write_sphere_obj(path, 250, 201) mesh (100 026 triangles), 512^2 points (2^18); 64 shadow samples each.
One JSON line per case, device times from stream events, median of --reps after one warm-up call, one process:
  shade_ms         rt_shade_points_device (light only) / shade_counts_ms (light and counts)
  baseline_ms      rt_trace_rays_device + the reduction, the rays already in memory
  baseline_all_ms  the same with the ray construction
  frame_ms         rt_last_kernel_ms of rt_render of the same view (1x1 AA, the same samples), for orientation
  identical        the baseline's counts equal the new entry's
usage: python tools/shade_time.py [--reps 7] [--only mesh|box] [--samples 64]"""
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


def xorshift(torch, s):
    m = 0xFFFFFFFF
    s = s ^ ((s << 13) & m)
    s = s ^ (s >> 17)
    return s ^ ((s << 5) & m)


def build_rays(torch, p6, seeds, samples, spread):
    """direct_light's sample rays (kernels.cl:319-333) as torch expressions: rays float32 [k * samples, 6], radius_sq"""
    light = torch.tensor(LIGHT, dtype=torch.float32, device=p6.device)
    p = p6[:, 0:3]
    d = light - p
    start = p + 1e-4 * d
    rsq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    g = seeds.to(torch.int64)
    gf = seeds.to(torch.float32)
    r = torch.stack([g, (gf * 91.0).to(torch.int64), (gf * 19.0).to(torch.int64)], 1)
    r = xorshift(torch, r)
    rays = torch.empty((p6.shape[0], samples, 6), dtype=torch.float32, device=p6.device)
    rays[:, :, 0:3] = start[:, None, :]
    for i in range(samples):
        r = xorshift(torch, r)
        rays[:, i, 3:6] = d + (spread * r.to(torch.float32) / 4294967296.0 - spread / 2.0)
    return rays.reshape(-1, 6), rsq[:, None].expand(-1, samples).reshape(-1).contiguous()


def timed(torch, stream, fn, reps):
    """Median device ms of fn between two events on `stream`, after one warm-up call"""
    fn()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def run(name, scene, side, samples, reps, torch):
    cfg = abi.make_config(width=side, height=side, aa_x=1, aa_y=1, shadow_samples=samples)
    tr = rt.RayTracer(cfg, scene)
    rot, focal = rt.rotation_matrix(0.0, 0.0), 1100.0 * side / 1024.0
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        planes = {"position": torch.empty((side, side, 4), dtype=torch.float32, device="cuda"),
                  "normal": torch.empty((side, side, 4), dtype=torch.float32, device="cuda")}
        tr.render_aov_device(rot, CAM, focal, out=planes)
        p6 = torch.cat([planes["position"][..., :3], planes["normal"][..., :3]], -1).reshape(-1, 6).contiguous()
        k = p6.shape[0]
        seeds = torch.arange(k, dtype=torch.int32, device="cuda")
        out_light = torch.empty(k, dtype=torch.float32, device="cuda")
        out_cnt = torch.empty(k, dtype=torch.int32, device="cuda")
        shade_ms = timed(torch, stream, lambda: tr.shade_points_device(p6, LIGHT, seeds=seeds, out_light=out_light), reps)
        stats = tr.shade_stats()
        shade_counts_ms = timed(torch, stream, lambda: tr.shade_points_device(p6, LIGHT, seeds=seeds, out_light=out_light,
                                                                              out_counts=out_cnt), reps)
        stats_counts = tr.shade_stats()
        rays, r2 = build_rays(torch, p6, seeds, samples, cfg.light_spread)
        blocked = torch.empty(rays.shape[0], dtype=torch.int32, device="cuda")
        base = {}

        def baseline(construct):
            rr, r22 = build_rays(torch, p6, seeds, samples, cfg.light_spread) if construct else (rays, r2)
            tr.query_device(abi.RT_TRACE_IN_SHADOW, rr, r22, out_tri=blocked)
            base["cnt"] = samples - blocked.reshape(k, samples).sum(1)

        baseline_ms = timed(torch, stream, lambda: baseline(False), reps)
        qstats = tr.trace_stats()
        baseline_all_ms = timed(torch, stream, lambda: baseline(True), max(reps // 2, 1))
        stream.synchronize()
        identical = bool(torch.equal(base["cnt"].to(torch.int32), out_cnt))
    frame = []
    for _ in range(reps + 1):
        tr.render(rot, CAM, LIGHT, focal)
        frame.append(tr.last_kernel_ms())
    print(json.dumps({"scene": name, "triangles": len(scene), "points": k, "samples": samples,
                      "shade_ms": round(shade_ms, 3), "shade_counts_ms": round(shade_counts_ms, 3),
                      "baseline_ms": round(baseline_ms, 3), "baseline_all_ms": round(baseline_all_ms, 3),
                      "frame_ms": round(statistics.median(frame[1:]), 3), "identical": identical,
                      "shade_stats": stats, "shade_counts_stats": stats_counts, "query_stats": qstats}), flush=True)
    tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--only", choices=("mesh", "box"))
    a = ap.parse_args()
    import torch
    box = rt.Scene.cornell_box()
    if a.only != "mesh":
        run("box", box, 1024, a.samples, a.reps, torch)
    if a.only != "box":
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.obj")
            meshgen.write_sphere_obj(path, 250, 201)
            run("box+mesh", box + rt.Scene.load_obj(path), 512, a.samples, a.reps, torch)


if __name__ == "__main__":
    main()
