#!/usr/bin/env python3
"""bench.py — headline benchmark: Cornell Box 4096x4096, 8xAA (4x2), 64 shadow rays (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of the hot path over one frame.  With N ranks the ONE frame is split into
interleaved row bands (rank r renders bands r, r+N, ...: the partition of include/uob_rt.h rt_config),
each rank renders its bands with the HIP kernel into its own HBM, the bands are gathered to rank 0 over
RCCL and rank 0 de-interleaves them into the final ARGB frame — total work is fixed, so "scaling" is
"strong".  `value` is nominal Mrays/s = W*H*AA*(1+S) / time, whole job, frame resident in HBM of rank 0.

Prints ONE JSON line (rank 0).  A plain run only warms up, times the K steps and reports the headline figure
(`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, `kernel_ms_per_launch`).  `--dump-outputs DIR`
writes the frame of the last timed step to DIR (dump_outputs).  `--full` adds everything else it measures and checks:
  `roofline`      hardware-side: the bounding unit of this path is the FP32 vector ALU's instruction issue;
                  frac = VALU wave-instructions the timed kernel EXECUTES per launch (rocprofv3 PMC pass of this command,
                  profiles/r02_pmc.json) x 2 issue cycles / (1024 SIMDs x 2.4 GHz x the kernel time measured live here)
  `roofline_hbm`  the HBM view the north star asks for (<< 1 % by construction)
  `algorithmic_speedup_vs_bruteforce`  the reference's brute-force flop / kernel time — NOT a hardware fraction
  `cpu_baseline`  the CPU oracle (and the reference's own kernel built for x86-64) timed on this host's cores
  and the work counters, host enqueue time, frame checksum, brute-force / host-buffer / animated-light legs, the
  reference's own kernel on this GPU and the oracle checks of the frame.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_VALU_TFLOPS = 157.3     # MI355X_MICROARCH.md, chip-level parameters: 1024 SIMDs x 64 FLOP/clk x 2.4 GHz
PEAK_HBM_GBPS = 8000.0
SIMDS, CLOCK_GHZ = 1024, 2.4       # 256 CUs x 4 SIMD-32; max clock
VALU_ISSUE_CYCLES = 2             # a wave64 VALU instruction occupies its SIMD-32 for 2 cycles (MI355X_MICROARCH.md)
PMC_FILE = "r03_pmc.json"         # profiles/: counters per launch from the rocprofv3 --pmc passes of this command
FLOP_PER_TRI_TEST = 46            # Moeller-Trumbore with e1,e2 precomputed
FLOP_PER_SPHERE_TEST = 30
DUMP_PIXELS = 1 << 21             # --dump-outputs: a frame with more pixels is sampled (4 float32 each: 32 MiB)
DUMP_SEED = 20261016

WORKLOADS = {
    # BASELINE.json configs[3] / metric: the headline frame
    "headline": dict(width=4096, height=4096, aa_x=4, aa_y=2, shadow_samples=64),
    # configs[1]
    "cfg2": dict(width=1024, height=1024, aa_x=2, aa_y=2, shadow_samples=16, spheres=()),
    # configs[2]: glass sphere + mirror wall, 1920x1080, 4xAA, recursion depth 5 (10 shadow rays: the reference's default)
    "cfg3": dict(width=1920, height=1080, max_bounces=5),
    # configs[4]: Loader.cpp-style OBJ mesh of ~100k triangles in the box, 2048x2048, 1 spp, 1 shadow ray, diffuse
    "cfg5": dict(width=2048, height=2048, aa_x=1, aa_y=1, shadow_samples=1, spheres=()),
    # the reference exactly as shipped
    "reference": dict(width=1024, height=1024),
}


def source_hash():
    """sha256 over the kernel sources the library is built from (tools/pmc_to_json.py stores the same hash with the
    counters it collects: counters of another build are flagged stale instead of being priced with this build's time)."""
    import hashlib
    d = os.path.join(ROOT, "uob_raytracer_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h", ".cpp")):
            h.update(name.encode())
            with open(os.path.join(d, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()[:16]


def dump_outputs(out_dir, frame):
    """`frame_argb.npy`: the ARGB8888 words the caller's buffer holds after the step, as float32 channel values
    [pixels, 4] = (A, R, G, B), pixels in row order.  A frame of more than DUMP_PIXELS pixels is represented by the same
    DUMP_PIXELS pixels on every run (seeded sample, kept in row order)."""
    import torch
    flat = frame.reshape(-1)
    if flat.numel() > DUMP_PIXELS:
        pix = np.sort(np.random.default_rng(DUMP_SEED).choice(flat.numel(), size=DUMP_PIXELS, replace=False))
        flat = flat[torch.from_numpy(pix).to(flat.device)]
    words = flat.cpu().numpy().view(np.uint32)
    argb = np.stack([(words >> sh) & 0xFF for sh in (24, 16, 8, 0)], axis=1).astype(np.float32)
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "frame_argb.npy"), argb)


def build_scene(workload, rt):
    """Cornell Box (LoadTestModel), plus what the named configuration adds to it."""
    scene = rt.Scene.cornell_box()
    if workload == "cfg3":      # back wall -> mirror (TestModelH.h:58)
        scene = scene.with_color([8, 9], (1.0, 1.0, 1.0, 0.0))
    if workload == "cfg5":      # synthetic OBJ in the syntax Loader.cpp accepts (bunny_200.obj is not in the reference)
        import tempfile
        from uob_raytracer_amd import meshgen
        path = os.path.join(tempfile.mkdtemp(), "mesh_100k.obj")
        meshgen.write_sphere_obj(path, 250, 201)
        scene = scene + rt.Scene.load_obj(path)
    return scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20,
                    help="untimed frames first (the device needs ~15 frames / 50 ms of load to reach its clocks, profiles/r02_wave_timeline.txt)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the frame the last one rendered to DIR/frame_argb.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beyond the headline figure: work counters, roofline, host enqueue time, "
                         "frame checksum, the brute-force / host-buffer / animated-light / CPU-baseline / reference legs, "
                         "the oracle checks.  --no-cpu-baseline, --no-brute-force and --timed-only trim it")
    ap.add_argument("--workload", default="headline", choices=list(WORKLOADS))
    ap.add_argument("--band-rows", type=int, default=16,
                    help="rows per band of the interleaved partition (N > 1).  16: the shares of the ranks of 8 cost the same within 1 %% "
                         "(32: the dearest rank of 8 took 10 %% longer than the cheapest, profiles/r03_emulated_ranks.txt)")
    ap.add_argument("--cpu-sample-pixels", type=int, default=0, help="0 = auto (about 10-30 s of CPU work)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-brute-force", action="store_true", help="skip the cull-off comparison leg (N=1 only)")
    ap.add_argument("--timed-only", action="store_true",
                    help="with --full: only the warm-up and the timed steps (no work counters, no comparison / host-buffer / "
                         "animated / CPU legs): what the rocprofv3 passes of tools/pmc_passes.sh run, so that every dispatch "
                         "of the kernel in the profile is the timed workload")
    ap.add_argument("--force-collective", action="store_true",
                    help="with one rank, still initialise the process group and run the band gather (exercises the "
                         "RCCL calls of the N>1 flow on a one-GPU box)")
    ap.add_argument("--emulate-rank", default=None, metavar="r/N",
                    help="ONE process renders rank r's bands of an N-rank split of the frame and goes through the whole N > 1 step "
                         "(two contexts on two streams, RCCL gather, the root's de-interleave over N stripes): what one rank of the "
                         "N-GPU job costs per step on the GPU and on the host (enqueue time), measured on a one-GPU box")
    ap.add_argument("--contexts", type=int, default=2,
                    help="N > 1: contexts (and render streams) a rank cycles through, i.e. frames in flight on its GPU")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo = rehearsal of the N>1 flow on a box with fewer GPUs than ranks (bands travel via host memory)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    import torch
    import torch.distributed as dist
    from uob_raytracer_amd import abi, bands, runtime as rt

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("launch with torch.distributed.run --nproc-per-node %d for --gpus %d" % (args.gpus, args.gpus))
        args.gpus = world
    if args.backend == "gloo":          # rehearsal: several ranks may share one GPU
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    emu = None
    if args.emulate_rank:
        er, en = (int(x) for x in args.emulate_rank.split("/"))
        if world != 1 or not (0 <= er < en <= 64):
            sys.exit("--emulate-rank r/N needs one process and 0 <= r < N")
        emu = (er, en)
        args.force_collective = True
    collective = world > 1 or args.force_collective
    part_world, part_rank = (emu[1], emu[0]) if emu else (world, rank)     # the band partition this process renders a part of
    saved_stdout = None

    def emit(out):
        sys.stdout.flush()
        if saved_stdout is not None:
            os.dup2(saved_stdout, 1)
            os.close(saved_stdout)
        print(json.dumps(out), flush=True)
        if collective:
            os.dup2(2, 1)           # (anything the teardown prints goes to stderr as well)
            dist.destroy_process_group()

    if collective:
        # RCCL prints a version banner on stdout when its first communicator is made: keep stdout for the ONE JSON line
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend="gloo")

    wl = WORKLOADS[args.workload]
    W, H = wl["width"], wl["height"]
    band_rows = args.band_rows if collective else H
    cfg = abi.make_config(band_rows=band_rows, band_index=part_rank, band_count=part_world, device=local_rank, **wl)
    scene = build_scene(args.workload, rt)
    tracer = rt.RayTracer(cfg, scene)
    rows = tracer.rows
    focal = 1100.0 * min(W, H) / 1024.0 * cfg.aa_x
    rot = rt.rotation_matrix(0.0, 0.0)
    cam, light = [0.0, 0.0, -3.2], [0.0, -0.5, -0.7]

    # every rank sends an equal-size stripe of whole bands (its own rows packed at the top): any height works
    prow = bands.padded_rows(H, part_world, band_rows) if collective else rows
    stripe = torch.zeros((prow, W), dtype=torch.int32, device=dev)
    gathered = frame_pad = frame = None
    if collective and rank == 0:    # one [world, prow, W] receive buffer; the gather list is its slices
        gathered = torch.zeros((part_world, prow, W), dtype=torch.int32, device=dev)
        frame_pad = torch.empty((prow * part_world, W), dtype=torch.int32, device=dev)
        frame = frame_pad[:H]

    # N > 1 over RCCL: the render of frame k+1 runs on its own stream into the other of two stripe buffers while
    # the bands of frame k are gathered and de-interleaved on the current stream (events order the hand-overs).
    # Consecutive frames come from TWO contexts on two streams: the next frame's workgroups take the slots the draining
    # one frees (a context runs its own frames one at a time).  Measured on one GPU with one rank's bands
    # (tools/band_pipeline.py): 2048 rows 1.97 -> 1.72 ms per frame, 1024 rows 1.04 -> 0.90, 512 rows 0.63 -> 0.63.
    pipelined = collective and args.backend == "nccl"
    if pipelined:
        M = max(1, args.contexts)
        render_streams = [torch.cuda.Stream(device=dev) for _ in range(M)]
        tracers = [tracer] + [rt.RayTracer(cfg, scene) for _ in range(M - 1)]
        # two stripe buffers per context: the render of frame k + M (same context) does not wait for the gather of frame k
        # (with one, the chain render -> gather -> next render of that context set the period: kernel trace of an emulated
        # rank, 0.4526 ms/step of which 0.15 ms were that wait)
        NS_ = M * max(1, int(os.environ.get("BENCH_STRIPES_PER_CONTEXT", "2")))
        stripes = [stripe] + [torch.zeros_like(stripe) for _ in range(NS_ - 1)]
        rendered = [torch.cuda.Event() for _ in range(NS_)]      # stripe j holds a finished frame
        consumed = [torch.cuda.Event() for _ in range(NS_)]      # the gather that read stripe j has finished
        consumed_valid = [False] * NS_
    state = {"k": 0}

    def step(ev=None):
        if pipelined:
            i = state["k"] % len(tracers)
            j = state["k"] % len(stripes)
            state["k"] += 1
            cur = torch.cuda.current_stream()
            render_stream = render_streams[i]
            if consumed_valid[j]:
                render_stream.wait_event(consumed[j])
            if ev:
                ev[0].record(render_stream)
            tracers[i].render_device(rot, cam, light, focal, stripes[j].data_ptr(), None, render_stream.cuda_stream)
            if ev:
                ev[1].record(render_stream)
            rendered[j].record(render_stream)
            cur.wait_event(rendered[j])
            bands.gather_frame(stripes[j], part_world, part_rank, band_rows, gathered, frame_pad, force=True, height=H, emulate=emu is not None)
            consumed[j].record(cur)
            consumed_valid[j] = True
            return
        # the HIP kernel, enqueued on torch's current stream through the C ABI
        if ev:
            ev[0].record()
        tracer.render_device(rot, cam, light, focal, stripe.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        if ev:
            ev[1].record()
        # gloo rehearsal of N > 1: the bands travel via host memory; N == 1: the stripe IS the frame
        if args.backend == "gloo" and collective:
            host = bands.gather_frame(stripe.cpu(), part_world, part_rank, band_rows, force=True, height=H, emulate=emu is not None)
            if rank == 0:
                frame.copy_(host)

    def sync():
        if collective:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce_(t, op):
        if args.backend == "gloo":
            c = t.cpu()
            dist.all_reduce(c, op=op)
            t.copy_(c)
        else:
            dist.all_reduce(t, op=op)

    # exact algorithmic work of this rank's bands (un-timed instrumented passes): `work` follows the
    # reference's loops literally (rt_count_work); `executed` is what the wave kernel really runs
    if args.timed_only or not args.full:
        args.no_cpu_baseline = args.no_brute_force = True
        work = {k: 0 for k, _ in abi.RtWork._fields_}
        executed = {}
    else:
        # (N > 1: every rank counts the WHOLE frame — no reduction needed, and the 0.3 s of load bring the device to its
        # clocks before the short warm-up of a 0.45 ms step)
        counter = tracer if not collective else rt.RayTracer(abi.make_config(device=local_rank, **wl), scene)
        work = counter.count_work(rot, cam, light, focal)
        try:
            executed = counter.count_executed(rot, cam, light, focal)
        except rt.RtError:
            executed = {}
        if counter is not tracer:
            counter.close()

    if collective:
        # A rank's step is a fraction of a millisecond: W warm-up steps are over before the device has left its idle clocks
        # (the first measurement of a fresh process reads 0.47-0.52 ms at N = 8 against 0.36 afterwards, whatever the build).
        # About 0.3 s of un-timed steps first — a fixed count, the same on every rank: the steps hold a collective.
        for _ in range(130 * part_world):
            step()
        sync()
    elif not args.full:
        # One GPU: --full's work-counting passes put ~0.3 s of load on the device before the warm-up; a plain run puts
        # as much in un-timed steps, so that a short --warmup starts from the same clocks.
        t_load = time.perf_counter()
        while time.perf_counter() - t_load < 0.3:
            for _ in range(4):
                step()
            sync()
    for _ in range(args.warmup):
        step()
    sync()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(ev[k])
    sync()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, frame if collective else stripe)
    if args.full:
        # the host's share of a step: a short burst enqueued into an EMPTY queue and not waited for (in the timed loop the
        # host runs ahead until the queue is full and then waits for the GPU, which says nothing about its own cost)
        burst = min(16, args.steps)
        t1 = time.perf_counter()
        for _ in range(burst):
            step()
        host_enqueue_s = (time.perf_counter() - t1) / burst * args.steps
        sync()
    kernel_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))

    keys, xkeys = list(work), list(executed)
    stats = torch.tensor([elapsed, kernel_ms] + [float(work[k]) for k in keys] + [float(executed[k]) for k in xkeys],
                         dtype=torch.float64, device=dev)
    if collective:
        mx = stats[:2].clone()
        reduce_(mx, dist.ReduceOp.MAX)
        stats = torch.cat([mx, stats[2:]])          # the work counters are whole-frame counts on every rank
    stats = stats.cpu().numpy()
    elapsed, kernel_ms = float(stats[0]), float(stats[1])
    total_work = {k: int(round(v)) for k, v in zip(keys, stats[2:2 + len(keys)])}
    total_exec = {k: int(round(v)) for k, v in zip(xkeys, stats[2 + len(keys):])}

    # frame integrity: rank 0 sums the final frame (N=1: the stripe is the frame)
    if rank == 0 and args.full:
        final = frame if collective else stripe
        frame_sum = int(final.to(torch.int64).bitwise_and(0xFFFFFFFF).sum().item())

    if rank != 0:
        if collective:
            dist.destroy_process_group()
        return

    aa = cfg.aa_x * cfg.aa_y
    nominal_rays = W * H * aa * (1 + cfg.shadow_samples)
    ms_per_step = elapsed * 1e3 / args.steps
    out = {
        "metric": "Mrays/sec (nominal = W*H*AA*(1+S)/t), " + (
            "Cornell Box 4096^2, 8xAA, 64 shadow rays" if args.workload == "headline" else
            "workload %s: %dx%d, %dxAA, %d shadow rays, %d triangles (not the headline frame)" % (args.workload, W, H, aa, cfg.shadow_samples, len(scene))),
        "value": nominal_rays / (ms_per_step * 1e-3) / 1e6,
        "unit": "Mrays/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "%s: Cornell Box %dx%d, %dx%d AA, %d shadow rays, %d spheres, <=%d bounces, %d triangles" % (
            args.workload, W, H, cfg.aa_x, cfg.aa_y, cfg.shadow_samples, cfg.num_spheres, cfg.max_bounces, len(scene)),
            "parallelism": "row bands of %d over %d GPU(s) + RCCL gather" % (band_rows, part_world) if collective else "1 GPU"},
        "kernel_ms_per_launch": kernel_ms,
    }
    if not args.full:
        emit(out)
        return

    traced_rays = total_work["primary_rays"] + total_work["bounce_rays"] + total_work["shadow_rays"]
    flops = (total_work["closest_tri_tests"] + total_work["shadow_tri_tests"]) * FLOP_PER_TRI_TEST + \
            (total_work["closest_sphere_tests"] + total_work["shadow_sphere_tests"]) * FLOP_PER_SPHERE_TEST
    # per launch = per rank: every rank runs the same kernel on 1/world of the frame
    flops_per_launch = flops / part_world
    achieved_tflops = flops_per_launch / (kernel_ms * 1e-3) / 1e12
    # algorithmic HBM bytes per launch: the rank's share of the ARGB frame + the scene once (workgroups re-read it from L2)
    hbm_bytes_per_launch = W * rows * 4 + len(scene) * 80
    achieved_gbps = hbm_bytes_per_launch / (kernel_ms * 1e-3) / 1e9

    # Counters of a timed step, from the rocprofv3 --pmc passes of this command committed under profiles/ (counters cannot
    # be collected from inside the run; the kernel TIME is measured live, above).  Quoted only for the workload they were
    # collected on AND the build they were collected on (hash of the kernel sources); with N ranks every rank runs the
    # same kernels on 1/N of the rows.
    pmc, stale = None, False
    try:
        with open(os.path.join(ROOT, "profiles", PMC_FILE)) as f:
            pmc = json.load(f).get(args.workload)
    except (OSError, ValueError):
        pass
    if pmc and pmc.get("source_sha256_16") != source_hash():
        stale = True
    # with two contexts in flight (N > 1) consecutive kernels overlap: a launch's share of the device is the frame period
    kernel_s = (min(kernel_ms, ms_per_step) if pipelined else kernel_ms) * 1e-3
    if pmc and not stale:
        ps = pmc["per_step"]
        traffic = ps["hbm_bytes"] / part_world
        valu = ps["valu_instructions"] / part_world
        fp32 = ps["fp32_flop_upper_bound"] / part_world / kernel_s / 1e12
        dom = pmc["kernels"][pmc["dominant_kernel"]]
        roofline = {
            "bound": "valu", "achieved": fp32, "peak": PEAK_FP32_VALU_TFLOPS, "unit": "TFLOP/s",
            "frac": fp32 / PEAK_FP32_VALU_TFLOPS, "traffic": traffic, "stale": False,
            "note": "hardware-side, FP32 vector ALU (the bounding unit of this path, SURVEY.md 8d; not HBM, not MFMA): achieved = FP32 "
                    "add + mul + 2 x fma + transcendental wave-instructions x 64 lanes executed per step (PMC, all lanes "
                    "counted active: an upper bound) / the step's kernel time measured live in this run.  The kernels "
                    "are built with -ffp-contract=off (bit-exact with the reference's operation order), so most FP32 "
                    "instructions deliver 1 flop of the 2 an FMA would: see issue_slot_utilisation for how busy the VALUs are",
            "issue_slot_utilisation": valu * VALU_ISSUE_CYCLES / (SIMDS * CLOCK_GHZ * 1e9 * kernel_s),
            "issue_slot_note": "VALU wave-instructions executed per step (SQ_INSTS_VALU%s) x 2 issue cycles / (1024 SIMDs x 2.4 GHz x "
                               "kernel time): the share of VALU issue slots that hold an instruction of any kind (FP32, compare, "
                               "select, lane read, integer)" % ("" if part_world == 1 else ", N=1 pass / %d ranks" % part_world),
            "valu_instructions_per_step": valu, "salu_instructions_per_step": ps.get("salu_instructions", 0) / part_world,
            "kernel": pmc["dominant_kernel"], "kernels_per_step": {k: v["trace"].get("launches_per_step") for k, v in pmc["kernels"].items()},
            "dominant_kernel_trace_avg_ms": dom["trace"].get("avg_ns", 0) / 1e6,
            "counters": "profiles/" + PMC_FILE, "source_sha256_16": pmc["source_sha256_16"],
            "lds_bank_conflict_fraction": dom.get("lds_bank_conflict_fraction"),
            "mean_waves_per_simd": dom.get("mean_waves_per_simd"), "wave_cycle_shares": dom.get("wave_cycle_shares")}
    else:
        traffic = None
        roofline = {"bound": "valu", "achieved": None, "peak": PEAK_FP32_VALU_TFLOPS, "unit": "TFLOP/s", "frac": None,
                    "traffic": None, "stale": stale,
                    "note": ("the counters under profiles/%s were collected on another build of the kernels (source hash %s, this tree %s): "
                             "not priced" % (PMC_FILE, pmc.get("source_sha256_16"), source_hash())) if stale else
                            "no PMC pass of this workload is committed under profiles/%s" % PMC_FILE}
    algorithmic = {"achieved": achieved_tflops, "unit": "TFLOP/s", "x_over_hardware_peak": achieved_tflops / PEAK_FP32_VALU_TFLOPS,
                   "note": "ALGORITHMIC rate, not a hardware fraction: (triangle tests*46 + sphere tests*30 flop) of the "
                           "reference's brute-force loops per launch / kernel time. The kernel decides most (surface point, "
                           "triangle) pairs by an exact interval bound instead of 64 per-sample tests, so this exceeds the "
                           "hardware peak; `executed` is what it really runs"}
    if total_exec and "stage1_wave_iterations" not in total_exec:      # tiled mesh kernel (n > 64)
        algorithmic["executed"] = dict({k: v for k, v in total_exec.items() if not k.startswith("_")},
                                       note="work the tiled mesh kernel really executes (rt_count_executed): (wave, tile) "
                                            "visits and the triangles its bounds leave, per pass")
    elif total_exec:
        algorithmic["executed"] = {
            "sample_triangle_tests": 64 * total_exec["stage1_wave_iterations"],
            "fraction_of_reference_tests": 64 * total_exec["stage1_wave_iterations"] / max(total_work["shadow_tri_tests"], 1),
            "surface_points_sampled": total_exec["surface_points"],
            "surface_points_decided_lit_by_bounds": total_exec["culled_pairs"],
            "tasks_decided_whole": total_exec["tasks_resolved_whole"],
            "lit_surface_points": total_work["lit_hits"],
            "note": "work the shipped kernel really executes (rt_count_executed): the 64-sample test runs only for "
                    "(surface point, triangle) pairs the interval bounds leave undecided"}

    out.update({
        "host_enqueue_ms_per_step": host_enqueue_s * 1e3 / args.steps,
        "traced_mrays_per_s": None if args.timed_only else traced_rays / (ms_per_step * 1e-3) / 1e6,
        "nominal_rays_per_frame": nominal_rays, "traced_rays_per_frame": None if args.timed_only else traced_rays,
        "work_per_frame": total_work,
        "frame_checksum": frame_sum,
        "parity": "bit-exact vs the CPU oracle (strict FP32, reference operation order); oracle and product vs the reference ITSELF "
                  "on this GPU's OpenCL device (kernels.cl built for gfx950 with AMD's OpenCL builtins and the reference's own options): "
                  ">= 99.17 % of the pixels of every fixture frame within 1 LSB of its 8-bit output (= 1e-4 in colour; 99.83 % on the "
                  "shipped 1024^2 frame, > 99.997 % from a general view), and every pixel beyond lies within 1 px of a ray/edge "
                  "discontinuity (tests/test_oracle_ref_gpu.py, tests/test_gpu_ref_gpu.py)",
        "roofline": roofline,
        "algorithmic_speedup_vs_bruteforce": algorithmic,
        "roofline_hbm": {"bound": "hbm", "achieved": achieved_gbps, "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                         "frac": achieved_gbps / PEAK_HBM_GBPS, "traffic": traffic,
                         "algorithmic_bytes_per_launch": hbm_bytes_per_launch,
                         "note": "algorithmic bytes = 4 B/pixel ARGB + 80 B/triangle once; <<1% by construction; "
                                 "traffic = HBM bytes per launch (2 x FETCH_SIZE + WRITE_SIZE, gfx950 correction) from the PMC "
                                 "passes in profiles/" + PMC_FILE},
    })

    if emu:
        out["emulated_rank"] = {
            "rank": emu[0], "of": emu[1], "rows": rows, "steps_per_s": args.steps / elapsed,
            "host_enqueue_ms_per_step": host_enqueue_s * 1e3 / args.steps, "gpu_kernel_ms_per_step": kernel_ms,
            "note": "ONE process playing rank %d of %d and the root: its bands rendered by two contexts on two streams, gathered over RCCL "
                    "into slot %d of the root's receive buffer, the root's de-interleave over all %d slots.  `value` is what the "
                    "%d-GPU job would deliver if every rank took this long per step — a budget, not a measurement of that job; "
                    "frame_checksum covers this rank's bands only" % (emu[0], emu[1], emu[0], emu[1], emu[1])}

    if not collective and not args.no_brute_force and "stage1_wave_iterations" in total_exec and args.workload == "headline":
        # the same frame with the interval cull switched off (every triangle tested for every surface point)
        bcfg = abi.make_config(flags=abi.RT_FLAG_NO_CULL, device=local_rank, **wl)
        bt = rt.RayTracer(bcfg, scene)
        bstripe = torch.empty((H, W), dtype=torch.int32, device=dev)
        bt.render_device(rot, cam, light, focal, bstripe.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            bt.render_device(rot, cam, light, focal, bstripe.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        bms = e0.elapsed_time(e1) / 3
        out["brute_force"] = {"kernel_ms_per_launch": bms, "value": nominal_rays / (bms * 1e-3) / 1e6,
                              "algorithmic_frac_of_fp32_peak": flops / (bms * 1e-3) / 1e12 / PEAK_FP32_VALU_TFLOPS,
                              "identical_frame": bool(torch.equal(bstripe, stripe)),
                              "note": "RT_FLAG_NO_CULL: same kernel, all triangles tested for every surface point"}
        bt.close()

    if not collective and not args.timed_only:
        # the drop-in call itself (rt_render = offload_rendering): kernel + blocking read-back into host memory
        host_frame = np.empty((H, W), np.uint32)
        host_frame.fill(0)                       # touch the pages once, as a live screen->buffer would be
        tracer.render(rot, cam, light, focal, out=host_frame)
        t0 = time.perf_counter()
        for _ in range(10):
            tracer.render(rot, cam, light, focal, out=host_frame)
        pms = (time.perf_counter() - t0) / 10 * 1e3
        # the same call with the framebuffer registered (rt_register_output): the kernel's stores cross PCIe themselves
        copied = host_frame.copy()
        host_frame.fill(0)
        tracer.register_output(host_frame)
        tracer.render(rot, cam, light, focal, out=host_frame)
        t0 = time.perf_counter()
        for _ in range(10):
            tracer.render(rot, cam, light, focal, out=host_frame)
        rms = (time.perf_counter() - t0) / 10 * 1e3
        tracer.unregister_output()
        registered_same = bool(np.array_equal(host_frame, copied))
        out["host_buffer_path"] = {"ms_per_frame": pms, "value": nominal_rays / (pms * 1e-3) / 1e6, "unit": "Mrays/s",
                                   "identical_frame": bool(np.array_equal(host_frame.view(np.int32), stripe.cpu().numpy())),
                                   "registered": {"ms_per_frame": rms, "value": nominal_rays / (rms * 1e-3) / 1e6,
                                                  "identical_frame": registered_same,
                                                  "note": "the same call after rt_register_output(framebuffer): the device "
                                                          "writes the pixels into host memory as they are finished"},
                                   "note": "rt_render with a pageable host framebuffer (PCIe read-back included); "
                                           "never the headline value"}

    if not collective and not args.timed_only:
        # the light animated as the reference's update() moves it (skeleton.cpp:290-298): every frame differs from the
        # one before, so the frame-to-frame scheduling state of the context (last frame's expensive jobs first) works
        # from a neighbouring frame instead of an identical one
        import numpy as _np
        lx, lor = _np.float32(0.0), True
        lights = []
        for _ in range(24):
            diff = (_np.float32(-0.5) if lor else _np.float32(0.5)) - lx
            if lor and diff > _np.float32(-0.001):
                lor = False
            elif not lor and diff < _np.float32(0.001):
                lor = True
            lx = _np.float32(lx + diff / _np.float32(20.0))
            lights.append([float(lx), -0.5, -0.7])
        aev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in lights]
        for (a, b), li in zip(aev, lights):
            a.record()
            tracer.render_device(rot, cam, li, focal, stripe.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
            b.record()
        torch.cuda.synchronize()
        ams = [a.elapsed_time(b) for a, b in aev][4:]
        out["animated_light"] = {"kernel_ms_per_frame": float(np.mean(ams)), "max_ms": float(np.max(ams)), "frames": len(ams),
                                 "value": nominal_rays / (float(np.mean(ams)) * 1e-3) / 1e6, "unit": "Mrays/s",
                                 "note": "light x animated by update() (skeleton.cpp:290-298), 20 consecutive frames after 4 "
                                         "warm-up frames; not the headline value (that is the static frame above)"}
        tracer.render_device(rot, cam, light, focal, stripe.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()          # the static frame again: the oracle check below looks at `stripe`

    if not args.no_cpu_baseline and collective:
        # N > 1: no CPU baseline (it is reported at N=1 only); spot-check the gathered frame against the oracle
        from oracle import pyref
        rng = np.random.default_rng(12345)
        pix = rng.choice(W * H, size=4000, replace=False).astype(np.int32)
        if emu:     # only this rank's bands were rendered
            pix = pix[((pix // W) // band_rows) % part_world == part_rank]
        v, n, c = scene.packed()
        o_argb, _ = pyref.Oracle().render(abi.make_config(**wl), v, n, c, rot, cam, light, focal, pix=pix,
                                          nthreads=min(len(os.sched_getaffinity(0)), 16))
        got = frame.view(-1)[torch.from_numpy(pix.astype(np.int64)).to(dev)].cpu().numpy().view(np.uint32)
        out["gathered_frame_matches_oracle_on_sample"] = bool(np.array_equal(got, o_argb))

    if not args.no_cpu_baseline and not collective:
        from oracle import pyref   # checker, used here only as the timed CPU baseline
        # the GPU box gives one-GPU jobs a 16-core share: never use more host threads than that
        cores = min(len(os.sched_getaffinity(0)), 16)
        rng = np.random.default_rng(12345)
        full = abi.make_config(**wl)
        v, n, c = scene.packed()
        orc = pyref.Oracle()
        npx = args.cpu_sample_pixels
        if not npx:     # calibrate on 4000 pixels, then size the sample for about 12 s of CPU work
            cal = rng.choice(W * H, size=4000, replace=False).astype(np.int32)
            t0 = time.perf_counter()
            orc.render(full, v, n, c, rot, cam, light, focal, pix=cal, nthreads=cores)
            npx = int(min(W * H, max(4000, 12.0 / max(time.perf_counter() - t0, 1e-4) * 4000)))
        pix = rng.choice(W * H, size=npx, replace=False).astype(np.int32)
        t0 = time.perf_counter()
        o_argb, _ = orc.render(full, v, n, c, rot, cam, light, focal, pix=pix, nthreads=cores)
        dt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": npx * aa * (1 + cfg.shadow_samples) / dt / 1e6, "unit": "Mrays/s", "cores": cores,
                               "kind": "port", "seconds": dt,
                               "sample": "%d random pixels of the same %dx%d frame (%.3g nominal rays), CPU oracle "
                                         "(oracle/rt_oracle.c, OpenMP, %d threads)" % (
                                             npx, W, H, npx * aa * (1 + cfg.shadow_samples), cores)}
        # the reference kernel itself (oracle/_ref, built from the reference's kernels.cl for x86-64), where it can
        # express the workload; for the headline (4x2 AA is not expressible) its 2x2-AA variant next to the port
        refv = {"reference": "default", "cfg2": "cfg2", "headline": "s64_4096"}.get(args.workload)
        if refv and pyref.have_ref(refv) and len(scene) == 26:
            rk = pyref.RefKernel(refv)
            rcfg = full if refv != "s64_4096" else abi.make_config(**dict(wl, aa_x=2, aa_y=2))
            raa = rcfg.aa_x * rcfg.aa_y
            rfocal = 1100.0 * min(W, H) / 1024.0 * rcfg.aa_x
            rpix = pix[:max(2000, min(npx, int(npx * aa / raa / 2)))]
            t0 = time.perf_counter()
            r_argb, _ = rk.render(v, n, c, rot, cam, light, rfocal, pix=rpix, nthreads=cores, want_rgb=False)
            rdt = time.perf_counter() - t0
            t0 = time.perf_counter()
            p_argb, _ = orc.render(rcfg, v, n, c, rot, cam, light, rfocal, pix=rpix, nthreads=cores)
            pdt = time.perf_counter() - t0
            rrays = rpix.size * raa * (1 + rcfg.shadow_samples)
            out["cpu_baseline"]["reference_kernel"] = {
                "value": rrays / rdt / 1e6, "unit": "Mrays/s", "cores": cores, "kind": "reference", "seconds": rdt,
                "sample": "%d random pixels, %dx%d, %dx%d AA, %d shadow rays: the reference's kernels.cl compiled for "
                          "x86-64 (oracle/_ref/libref_%s.so)" % (rpix.size, W, H, rcfg.aa_x, rcfg.aa_y, rcfg.shadow_samples, refv),
                "port_on_same_sample": rrays / pdt / 1e6,
                "port_matches_reference_kernel": bool(np.array_equal(r_argb, p_argb))}
        # Is there an OpenCL CPU device on this box (the reference enumerates devices at skeleton.cpp:516-573)?
        # And the reference's own kernel on the OpenCL device that IS here — this GPU: kernels.cl built for gfx950 against
        # AMD's OpenCL builtins with the reference's options (oracle/_ref/*.co), launched through the OpenCL runtime in a
        # process of its own (oracle/ref_cl_host.c), next to this library on the SAME configuration.
        from oracle import ref_gpu
        probe = ref_gpu.probe()
        out["cpu_baseline"]["opencl_cpu_devices"] = probe.get("opencl_cpu_devices", probe.get("error", "probe failed"))
        out["cpu_baseline"]["opencl_platforms"] = probe.get("platforms", probe.get("error"))
        refg = {"reference": ("default", {}), "cfg2": ("cfg2", {}), "cfg3": ("cfg3", {}),
                "headline": ("s64_4096", dict(aa_x=2, aa_y=2))}.get(args.workload)
        if refg and len(scene) == 26 and ref_gpu.have(refg[0]) and probe.get("opencl_gpu_devices", 0) > 0:
            variant, over = refg
            gcfg = abi.make_config(**dict(wl, **over))
            gaa = gcfg.aa_x * gcfg.aa_y
            gfocal = 1100.0 * min(W, H) / 1024.0 * gcfg.aa_x
            torch.cuda.synchronize()
            try:
                g_argb, info = ref_gpu.run(variant, W, H, v, n, c, rot, cam, light, gfocal, reps=3)
                gt = rt.RayTracer(abi.make_config(device=local_rank, **dict(wl, **over)), scene)
                gbuf = torch.empty((H, W), dtype=torch.int32, device=dev)
                for _ in range(6):
                    gt.render_device(rot, cam, light, gfocal, gbuf.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    gt.render_device(rot, cam, light, gfocal, gbuf.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
                e1.record()
                torch.cuda.synchronize()
                oms = e0.elapsed_time(e1) / 10
                gt.close()
                ours = gbuf.cpu().numpy().view(np.uint32).ravel()
                chd = np.zeros(ours.shape, np.int32)
                for sh in (0, 8, 16):
                    chd = np.maximum(chd, np.abs(((ours >> sh) & 255).astype(np.int32) - ((g_argb >> sh) & 255).astype(np.int32)))
                grays = W * H * gaa * (1 + gcfg.shadow_samples)
                out["reference_opencl_on_this_gpu"] = {
                    "kernel_ms": info["kernel_ms_mean"], "value": grays / (info["kernel_ms_mean"] * 1e-3) / 1e6, "unit": "Mrays/s",
                    "device": info["device"], "work_group": info["local"], "kind": "reference",
                    "config": "%dx%d, %dx%d AA, %d shadow rays (%s)" % (W, H, gcfg.aa_x, gcfg.aa_y, gcfg.shadow_samples,
                              "the workload itself" if not over else "2x2 AA: the reference cannot express the headline's 4x2 grid"),
                    "this_library_same_config": {"kernel_ms": oms, "value": grays / (oms * 1e-3) / 1e6, "speedup": info["kernel_ms_mean"] / oms},
                    "pixels_within_1_lsb": float((chd <= 1).mean()), "pixels_identical": float((chd == 0).mean()),
                    "note": "the reference's kernels.cl compiled for gfx950 against AMD's own OpenCL builtin library with its own "
                            "options (-cl-fast-relaxed-math -cl-mad-enable), run through the OpenCL runtime on this MI355X by "
                            "oracle/ref_cl_host (128x2 work-groups: AMD's OpenCL refuses the reference's 128x4); pixels beyond 1 LSB "
                            "sit on ray/edge discontinuities (tests/refgpu_check.py)"}
            except Exception as e:      # noqa: BLE001 - a baseline leg must not take the bench line down
                out["reference_opencl_on_this_gpu"] = {"error": "%s: %s" % (type(e).__name__, e)}
        # the sampled pixels double as an in-bench parity check of the frame just timed
        got = (stripe if world == 1 else frame).view(-1)[torch.from_numpy(pix.astype(np.int64)).to(dev)].cpu().numpy().view(np.uint32)
        out["cpu_baseline"]["gpu_frame_matches_oracle_on_sample"] = bool(np.array_equal(got, o_argb))

    emit(out)


if __name__ == "__main__":
    main()
