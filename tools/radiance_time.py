"""rt_radiance_rays_device against the frame and against the two calls it replaces.  Device times from events on the stream,
medians of --reps (>= 20) timed calls after warm-up calls, one process; one JSON line per case, also appended to
profiles/radiance_time.txt (--out).

  a. primary rays of the headline-like view (box + the reference's two spheres, 1024^2, 1x1 AA, 10 and 64 samples), the
     directions taken from an AOV pass: radiance_ms against frame_ms (rt_last_kernel_ms of rt_render of the same view);
  b. the same rays on an all-diffuse box without spheres: radiance_ms against the composition it replaces —
     rt_trace_rays_device(RT_TRACE_CLOSEST_HIT) + rt_shade_points_device on the hit plane (calls_ms: the two calls alone,
     the [k,6] point array handed over by a torch slice copy that is timed with them, because the shade call cannot read
     the ten-float plane in place; composed_ms: also the colour albedo * (0.5 + L) in torch);
  c. box + a meshgen.write_sphere_obj(path, 250, 201) mesh (100 026 triangles) made glass, 512^2 rays, 10 samples;
  d. a 2048 x 1024 panorama from the middle of the box (radiance_ms: the call on prepared rays; panorama_ms: render_panorama).
`identical` says that the colours of the compared paths are the same bits.
usage: python tools/radiance_time.py [--reps 20] [--only a|b|c|d] [--out profiles/radiance_time.txt]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from uob_raytracer_amd import abi, meshgen, runtime as rt  # noqa: E402

CAM = [0.0, 0.0, -3.2]
LIGHT = [0.0, -0.5, -0.7]


def timed(torch, stream, fn, reps, warm=2):
    """Median device ms of fn between two events on `stream`, after `warm` warm-up calls"""
    for _ in range(warm):
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


def frame_ms(tr, rot, focal, reps):
    ms = []
    for _ in range(reps + 2):
        tr.render(rot, CAM, LIGHT, focal)
        ms.append(tr.last_kernel_ms())
    return statistics.median(ms[2:])


def primary_rays(torch, tr, rot, focal, side):
    d = {"direction": torch.empty((side, side, 4), dtype=torch.float32, device="cuda")}
    tr.render_aov_device(rot, CAM, focal, out=d)
    start = torch.tensor(CAM, dtype=torch.float32, device="cuda").expand(side, side, 3)
    return torch.cat([start, d["direction"][..., :3]], -1).reshape(-1, 6).contiguous()


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def view_case(case, name, scene, side, samples, reps, torch, out, spheres=abi.REFERENCE_SPHERES, compose=False):
    cfg = abi.make_config(width=side, height=side, aa_x=1, aa_y=1, shadow_samples=samples, spheres=spheres)
    tr = rt.RayTracer(cfg, scene)
    rot, focal = rt.rotation_matrix(0.0, 0.0), 1100.0 * side / 1024.0
    stream = torch.cuda.Stream()
    rec = {"case": case, "scene": name, "triangles": len(scene), "rays": side * side, "samples": samples, "reps": reps}
    with torch.cuda.stream(stream):
        rays = primary_rays(torch, tr, rot, focal, side)
        k = rays.shape[0]
        seeds = torch.arange(k, dtype=torch.int32, device="cuda")
        rgba = torch.empty((k, 4), dtype=torch.float32, device="cuda")
        rec["radiance_ms"] = round(timed(torch, stream, lambda: tr.radiance_rays_device(rays, LIGHT, seeds=seeds, out=rgba), reps), 3)
        rec["radiance_stats"] = tr.radiance_stats()
        if compose:
            tri = torch.empty(k, dtype=torch.int32, device="cuda")
            out10 = torch.empty((k, 10), dtype=torch.float32, device="cuda")
            light = torch.empty(k, dtype=torch.float32, device="cuda")
            res = {}

            def calls(colour):
                tr.query_device(abi.RT_TRACE_CLOSEST_HIT, rays, out_tri=tri, out10=out10)
                tr.shade_points_device(out10[:, 0:6].contiguous(), LIGHT, seeds=seeds, out_light=light)
                if colour:
                    res["rgb"] = torch.where((tri != -1)[:, None], out10[:, 6:9] * (0.5 + light)[:, None], torch.zeros_like(out10[:, 6:9]))

            rec["calls_ms"] = round(timed(torch, stream, lambda: calls(False), reps), 3)
            rec["composed_ms"] = round(timed(torch, stream, lambda: calls(True), reps), 3)
            stream.synchronize()
            rec["identical"] = bool(torch.equal(res["rgb"].view(torch.int32), rgba[:, :3].contiguous().view(torch.int32)))
        stream.synchronize()
        got = rgba.cpu().numpy().reshape(side, side, 4)
    rec["frame_ms"] = round(frame_ms(tr, rot, focal, reps), 3)
    if not compose:
        _, rgb = tr.render(rot, CAM, LIGHT, focal, want_rgb=True)
        rec["identical"] = bool(np.array_equal(got[..., :3].view(np.uint32), np.ascontiguousarray(rgb[..., :3]).view(np.uint32)))
    emit(rec, out)
    tr.close()


def panorama_case(scene, reps, torch, out):
    W, H, cam = 2048, 1024, [0.0, 0.0, 0.0]
    tr = rt.RayTracer(abi.make_config(width=64, height=64, aa_x=1, aa_y=1, shadow_samples=10), scene)
    stream = torch.cuda.Stream()
    rec = {"case": "d", "scene": "box, panorama %dx%d" % (W, H), "triangles": len(scene), "rays": W * H, "samples": 10, "reps": reps}
    with torch.cuda.stream(stream):
        rec["panorama_ms"] = round(timed(torch, stream, lambda: tr.render_panorama(W, H, cam, LIGHT), reps), 3)
        import math
        f32 = dict(dtype=torch.float32, device="cuda")
        phi = (torch.arange(W, **f32) + 0.5) * torch.tensor(2.0 * math.pi, **f32) / W - math.pi
        theta = (torch.arange(H, **f32) + 0.5) * torch.tensor(math.pi, **f32) / H - math.pi / 2.0
        d = torch.stack([torch.sin(phi)[None, :] * torch.cos(theta)[:, None], torch.sin(theta)[:, None].expand(H, W),
                         torch.cos(phi)[None, :] * torch.cos(theta)[:, None]], -1)
        rays = torch.cat([torch.tensor(cam, **f32).expand(H, W, 3), d], -1).reshape(-1, 6).contiguous()
        seeds = torch.arange(W * H, dtype=torch.int32, device="cuda")
        rgba = torch.empty((W * H, 4), **f32)
        rec["radiance_ms"] = round(timed(torch, stream, lambda: tr.radiance_rays_device(rays, LIGHT, seeds=seeds, out=rgba), reps), 3)
        rec["radiance_stats"] = tr.radiance_stats()
    emit(rec, out)
    tr.close()


def all_diffuse(sc):
    for i in np.flatnonzero(sc.aos[:, 4, 3] <= 0):
        sc = sc.with_color([int(i)], tuple(sc.aos[i, 4, :3]) + (0.5,))
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("a", "b", "c", "d"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_time.txt"))
    a = ap.parse_args()
    import torch
    box = rt.Scene.cornell_box()
    if a.only in (None, "a"):
        for samples in (10, 64):
            view_case("a", "box + spheres", box, 1024, samples, a.reps, torch, a.out)
    if a.only in (None, "b"):
        for samples in (10, 64):
            view_case("b", "all-diffuse box", all_diffuse(box), 1024, samples, a.reps, torch, a.out, spheres=(), compose=True)
    if a.only in (None, "c"):
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.obj")
            meshgen.write_sphere_obj(path, 250, 201)
            view_case("c", "box + glass mesh", box + rt.Scene.load_obj(path, color=(0.9, 0.9, 0.9, -1.0)), 512, 10, a.reps, torch, a.out)
    if a.only in (None, "d"):
        panorama_case(box, a.reps, torch, a.out)


if __name__ == "__main__":
    main()
