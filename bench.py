#!/usr/bin/env python3
"""bench.py -- frames/sec (+ p50/p99 latency with --full) of the fused detector path, 640x640 batch-1, on N MI355X.

    python bench.py --gpus 1 --steps 2000 --warmup 200 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is ONE frame through the whole hot path on one GPU, as ONE hipGraph launch: stem (reads the fp32 NCHW frame
already resident in HBM) -> fused C3k2 block kernels, fused / paired head launches -> decode / sort / NMS ->
detections left in HBM (DESIGN.md section 4 lists the launches). Weak scaling: every rank processes K frames of its own
(frames shard embarrassingly); the only collective is the RCCL all-gather of the fixed-size
detection slots, issued every GATHER_EVERY frames on a dedicated comm stream behind the events of exactly those
frames (gather.SlotRing: double-buffered banks, inference never waits on the collective it just fed).
value = N*K / max-over-ranks(time of ONE block of exactly K steps); ms_per_step = that time / K. A short block is mostly
ramp (20 frames = 3 ms): pick K for a block of a second or more.

A plain run sets up, warms up, times the K steps, writes the last step's detections (--dump-outputs DIR) and prints the
line. --full adds what takes runs of its own: the serial latency (inside the C ABI and through ctypes; with the gather at
N > 1), the roofline of the dominant kernel (live per-op timing) and the CPU baseline (--no-cpu-baseline drops it).

Workload = BASELINE.json configs[1]: unina-yolo-dla-m (graph A), fp16, batch 1, 640x640, NMS on GPU; synthetic
frames (N(0,1), seeds 1234..), seeded synthetic weights (no checkpoints exist for the reference).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4, assigned round-robin at
# stream creation): with the default, the two per-frame streams can land on ONE queue and serialise (measured:
# 2 560 vs 4 340 frames/s). Must be set before the runtime initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402

FLOPS_PER_FRAME = {640: 35_664_691_200, 1280: 142_658_764_800}   # SURVEY.md section 8d (2 x MACs, conv only)
# dense MFMA peaks (MI355X_MICROARCH.md); int8 = 2x the fp16 matrix rate. "f16x2" = the STRICT mode's split-fp16 operands:
# priced against the fp16 peak on ALGORITHMIC flops (the kernels execute 3 fp16 MFMAs per algorithmic one)
PEAK_TFLOPS = {"f16": 2500.0, "f32": 157.3, "i8": 5000.0, "f16x2": 2500.0}
PEAK_HBM_GBS = 8000.0
PMC_TRAFFIC = os.path.join(ROOT, "profiles", "r03", "pmc_traffic.json")   # tools/pmc_traffic.sh: {config key: {kernel: bytes}} from rocprofv3 --pmc passes
N_FRAMES = 2048          # distinct synthetic frames in the stream (>= 2 000), generated on the device
N_SEEDED = 16            # the first of them are the seeded host frames (seeds 1234..) every parity test uses
IN_FLIGHT = int(os.environ.get("UNINA_IN_FLIGHT", "2"))   # engine handles per GPU = frames in flight
GATHER_EVERY = 16        # frames per RCCL all-gather of detection slots
GATHER_BANKS = 3         # slot banks of the ring (>= 2: the gather of one bank overlaps inference into the next)


def launcher_command(n_gpus, argv, port):
    """The command that starts `n_gpus` ranks of this script on one node (one process per GPU, RCCL rendezvous on 127.0.0.1)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *argv]


def launch_ranks(n_gpus, argv):
    """`python bench.py --gpus N` without a launcher around it (no WORLD_SIZE in the environment): start the N ranks here, as
    children, BEFORE anything in this process touches the GPU (a process that has initialised HIP must not be replaced or
    forked), relay their output (rank 0 prints the JSON line) and return their exit status. Fails loudly when the node has
    fewer than N GPUs instead of silently measuring one."""
    import socket
    import subprocess
    import torch
    backend = os.environ.get("UNINA_BENCH_BACKEND", "nccl")
    have = torch.cuda.device_count()          # (does not initialise the runtime on this image)
    if backend == "nccl" and have < n_gpus:
        print(f"bench.py: --gpus {n_gpus} needs {n_gpus} visible GPUs, this node has {have}; nothing was measured "
              f"(UNINA_BENCH_BACKEND=gloo rehearses the N-rank control flow on one GPU)", file=sys.stderr)
        return 2
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(launcher_command(n_gpus, argv, port), env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the serial latency, the roofline and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the detections of the last timed step to DIR/detections.npy (float32 [n, 6]: x1, y1, x2, y2, "
                         "confidence, class_id; other ranks: detections_rank<r>.npy)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="--full: time budget of the CPU baseline")
    ap.add_argument("--latency-frames", type=int, default=300, help="--full: frames of the serial latency loop")
    ap.add_argument("--precision", choices=["fp16", "fp32", "int8", "strict"], default="fp16",
                    help="fp16 = BASELINE configs[1] (headline); strict = split-fp16 operands (fp16 hi/lo pairs, 3 MFMAs per k block): "
                         "the north-star tolerance on every detection at the fp16 matrix rate; fp32 = native fp32-MFMA mode (same tolerance, 1/16 of the rate)")
    ap.add_argument("--calib-frames", type=int, default=64)
    ap.add_argument("--calibrator", choices=["max", "percentile", "entropy", "mse"], default="mse", help="INT8 activation range selection")
    ap.add_argument("--variant", choices=["A", "B"], default="A",
                    help="A = model.py's graph (BASELINE configs); B = qat.py's topology (stride-32 stage, third FPN level)")
    ap.add_argument("--tune-cache", default=os.environ.get("UNINA_TUNE_CACHE", ""), help="tactic cache file (JSON)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={os.environ.get('WORLD_SIZE')} ranks")

    import torch
    import torch.distributed as dist
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import export, gather
    from unina_yolo_dla_amd.engine import Engine, MAX_DETECTIONS

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal on a one-GPU box: UNINA_BENCH_BACKEND=gloo with every rank on device 0 (RCCL refuses two ranks per GPU)
    backend = os.environ.get("UNINA_BENCH_BACKEND", "nccl")
    local = local % max(torch.cuda.device_count(), 1)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    assert world == args.gpus, (world, args.gpus)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    S = args.size

    # ---- engine(s): seeded synthetic weights -> engine file -> IN_FLIGHT handles on this GPU ----
    g = u.graph.Graph(in_h=S, in_w=S, variant=args.variant)
    sd = u.synth.make_state_dict(7, g)
    fd, path = tempfile.mkstemp(suffix=f".rank{rank}.une")
    os.close(fd)
    prec = {"fp32": export.FP32, "int8": export.INT8, "strict": export.STRICT}.get(args.precision, export.FP16)
    amax = None
    if prec == export.INT8:   # BASELINE configs[2]: |x| histograms over 64 synthetic frames (seeds 5000..5063), range = the
        # mse-optimal threshold (the best of max / percentile / entropy / mse in profiles/r02/int8_drift_table.txt)
        from unina_yolo_dla_amd.engine import calibrate_amax
        amax = calibrate_amax(sd, g, (u.rng.frame(5000 + i, S, S) for i in range(args.calib_frames)), device=local, method=args.calibrator)
    export.export_engine(sd, path, g, prec, amax)
    engines = [Engine(path, device=local) for _ in range(IN_FLIGHT)]
    os.unlink(path)
    streams = [torch.cuda.Stream(device=dev) for _ in range(IN_FLIGHT)]
    # the input stream: N_FRAMES distinct N(0,1) frames resident in HBM (10 GB at 640^2 of the 288). The first N_SEEDED are the
    # package's seeded frames (rng.frame: what every test and the latency loop use), the rest come from a seeded device generator
    n_frames = max(N_SEEDED, min(N_FRAMES, int(11e9 // (12 * S * S))))
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + 100 * rank)
    stream_buf = torch.empty((n_frames, 1, 3, S, S), dtype=torch.float32, device=dev)
    stream_buf.normal_(generator=gen)
    for i in range(N_SEEDED):
        stream_buf[i].copy_(torch.from_numpy(u.rng.frame(1234 + i + 100 * rank, S, S)))
    frames = [stream_buf[i] for i in range(n_frames)]
    slot_words = 8 + 8 * MAX_DETECTIONS
    results = torch.zeros((GATHER_EVERY, slot_words), dtype=torch.int32, device=dev)
    conf = (0.5 if S == 640 else 0.6) if args.variant == "A" else 0.75   # keeps the seeded synthetic heads under MAX_DETECTIONS
    for e in engines:                      # engine build step: per-op tile selection by timing (outside the timed region)
        e.autotune(frames[0], iters=10, cache=args.tune_cache or None)
    torch.cuda.synchronize()

    ring = None
    gathered_frames = [0]
    if world > 1:
        local = torch.zeros((GATHER_BANKS, GATHER_EVERY, slot_words), dtype=torch.int32, device=dev)
        gathered = torch.zeros((GATHER_BANKS, world, GATHER_EVERY, slot_words), dtype=torch.int32, device=dev)

        def on_gathered(first_frame, bank):          # rank-0 consumer of a finished bank (here: count the frames)
            gathered_frames[0] += bank.shape[0] * bank.shape[1]
        ring = gather.SlotRing(gather.CudaRuntime(dev), local, gathered, GATHER_EVERY, on_gathered=on_gathered)
    next_frame = [0]
    last_slot = [None]                     # result slot of the last frame run() enqueued (what --dump-outputs writes)

    def infer_into(i, k, slot):
        with torch.cuda.stream(streams[k]):
            engines[k].infer_async(frames[i % n_frames], conf, 0.45, 0.1, out=slot, stream=streams[k])

    def run(n_frames):
        """n_frames frames, IN_FLIGHT of them overlapping on separate streams; N > 1: detections gathered with RCCL
        every GATHER_EVERY frames on the comm stream (gather.run_frames / SlotRing), off the inference streams' path."""
        if n_frames < 1:
            return
        if ring is None:
            for i in range(n_frames):
                infer_into(i, i % IN_FLIGHT, results[i % GATHER_EVERY])
            last_slot[0] = results[(n_frames - 1) % GATHER_EVERY]
            return
        gather.run_frames(n_frames, IN_FLIGHT, ring, infer_into, streams, start=next_frame[0])
        next_frame[0] += n_frames
        last = next_frame[0] - 1           # SlotRing.slot: frame i -> bank (i // k) % banks, slot i % k
        last_slot[0] = ring.local[(last // GATHER_EVERY) % GATHER_BANKS, last % GATHER_EVERY]

    def fence():
        if ring is not None:
            nxt = ring.flush()            # (a partly filled bank is gathered as it stands: exactly --steps frames are timed)
            if nxt is not None:
                next_frame[0] = nxt
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_block():
        fence()
        t0 = time.perf_counter()
        run(args.steps)
        fence()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    run(args.warmup)
    dt = timed_block()                     # exactly --steps timed frames per rank, one block
    fps = world * args.steps / dt
    n_det = int((ring.local[0, 0, 0] if ring is not None else results[0, 0]).item())
    if args.dump_outputs:
        dump_detections(args.dump_outputs, last_slot[0], rank)

    # ---- N > 1: per-frame latency INCLUDING the gather (every rank takes part: one collective per frame) ----
    lat_gather = None
    if world > 1 and args.full:
        one = torch.zeros((1, slot_words), dtype=torch.int32, device=dev)
        allr = torch.zeros((world, 1, slot_words), dtype=torch.int32, device=dev)
        samples = []
        for i in range(20 + 100):
            torch.cuda.synchronize()
            a = time.perf_counter()
            engines[0].infer_async(frames[i % n_frames], conf, 0.45, 0.1, out=one[0])
            gather.gather_slots(one, out=allr)
            torch.cuda.synchronize()
            if i >= 20:
                samples.append((time.perf_counter() - a) * 1e3)
        lat_gather = np.array(samples)

    dname = {"fp32": "f32", "int8": "i8", "strict": "f16x2"}.get(args.precision, "f16")
    full = {}                              # --full: the fields after "config" in the line
    if rank == 0 and args.full:
        # ---- per-frame latency: submit -> detections on the host, one frame at a time (no overlap) ----
        lat = []
        e0 = engines[0]
        for i in range(20 + args.latency_frames):
            f = frames[i % N_SEEDED]
            torch.cuda.synchronize()
            a = time.perf_counter()
            e0.infer(f, conf, 0.45, 0.1)
            if i >= 20:
                lat.append((time.perf_counter() - a) * 1e3)
        lat_py = np.array(lat)
        # the same serial loop timed INSIDE the C ABI (unina_serial_latency): what a C / C++ caller of the drop-in library sees.
        # The ctypes call above adds ~12 us per frame of binding cost (argument conversion, record copy into a fresh array).
        torch.cuda.synchronize()
        lat = e0.serial_latency(frames[:N_SEEDED], 20 + args.latency_frames, conf, 0.45, 0.1)[20:]

        # ---- roofline of the dominant kernel: live HIP-event timing of every op on the launch stream ----
        ops = e0.profile_ops(iters=20)
        post_ms = e0.profile_post(20, conf, 0.45, 0.1)
        by_kernel = {}
        for o in ops:
            if o["ms"] <= 0.0:
                continue                     # runs inside another op's launch (fused / dual / folded into the post-process)
            k = by_kernel.setdefault(o["kernel"], dict(ms=0.0, flops=0.0, bytes=0.0, launches=0))
            k["ms"] += o["ms"]; k["flops"] += o["flops"]; k["bytes"] += o["bytes"]; k["launches"] += 1
        # the post-process launches (decode incl. the folded head output convs: their flops; pair tiles + scan + output)
        for name, ms, fl in (("post_decode_kernel", post_ms[0], 0.0), ("post_nms_kernel", post_ms[1], 0.0)):
            if ms > 0.0:
                by_kernel[name] = dict(ms=ms, flops=fl, bytes=0.0, launches=1)
        dom_name, dom = max(by_kernel.items(), key=lambda kv: kv[1]["ms"])
        top = sorted(by_kernel.items(), key=lambda kv: -kv[1]["ms"])[:6]
        achieved_tf = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
        total_ms = sum(o["ms"] for o in ops)
        roofline = {
            "bound": "mfma", "kernel": dom_name, "launches_per_frame": dom["launches"],
            "avg_launch_us": round(1e3 * dom["ms"] / dom["launches"], 3),
            "flops_per_launch": dom["flops"] / dom["launches"],
            "achieved": round(achieved_tf, 2), "peak": PEAK_TFLOPS[dname], "unit": "TFLOP/s",
            "frac": round(achieved_tf / PEAK_TFLOPS[dname], 4), "traffic": pmc_traffic(f"{args.variant}:{args.precision}:{S}", dom_name),
            "algorithmic_bytes_per_launch": round(dom["bytes"] / dom["launches"]),
            "algorithmic_gbs": round(dom["bytes"] / (dom["ms"] * 1e-3) / 1e9, 1),
            "sum_of_ops_ms": round(total_ms, 4), "post_process_ms": [round(post_ms[0], 4), round(post_ms[1], 4)],
            "whole_frame_tflops": round(fps / world * 2 * g.macs() / 1e12, 2),
            # the six kernel instantiations with the largest share of the frame (same live timing)
            "top_kernels": [{"kernel": k, "launches": v["launches"], "us_per_frame": round(1e3 * v["ms"], 2),
                             "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["ms"] > 0 else 0.0,
                             "frac": round(v["flops"] / (v["ms"] * 1e-3) / 1e12 / PEAK_TFLOPS[dname], 4) if v["ms"] > 0 else 0.0}
                            for k, v in top],
        }

        # Where the dominant launch's time goes: for the dual conv launches a stamped twin of the kernel records every
        # workgroup's start / end on the 100 MHz wall clock (unina_debug_dual_timeline). `workgroups_span_us` = first start ->
        # last end, i.e. the launch WITHOUT the dispatch gap on either side; `frac` above stays the event-timed launch.
        try:
            lead = [i for i, o in enumerate(ops) if o["kernel"] == dom_name and o["ms"] > 0.0]
            if lead and dom_name.startswith("conv_dual_head3x3"):
                spans = []
                for i in lead:
                    for _ in range(5):
                        e0.forward(frames[0])                                  # replay the frame: cold weights, fresh inputs
                        tl = e0.dual_timeline(i)[:-1].astype(np.float64) * 0.01
                        spans.append(float(tl[:, 1].max() - tl[:, 0].min()))
                span = float(np.median(spans))
                roofline["workgroups_span_us"] = round(span, 2)
                roofline["frac_of_workgroups_span"] = round(dom["flops"] / dom["launches"] / (span * 1e-6) / 1e12 / PEAK_TFLOPS[dname], 4)
        except Exception as ex:                                                # debug API: never fail the bench line over it
            roofline["workgroups_span_us"] = None
            roofline["workgroups_span_note"] = str(ex)[:120]

        cpu = None
        if not args.no_cpu_baseline and world == 1:      # (rank 0 at N = 1 only: at N > 1 the other ranks would wait on it)
            cpu = cpu_baseline(u, sd, S, conf, args.cpu_seconds, args.variant)

        full = {
            "latency_ms": {"p50": round(float(np.percentile(lat, 50)), 4), "p99": round(float(np.percentile(lat, 99)), 4),
                           "mean": round(float(lat.mean()), 4), "frames": len(lat),
                           "mode": "serial, submit->detections on host, timed inside the C ABI (unina_serial_latency)",
                           "through_python_ctypes": {"p50": round(float(np.percentile(lat_py, 50)), 4), "p99": round(float(np.percentile(lat_py, 99)), 4)}},
            "roofline": roofline,
            "cpu_baseline": cpu,
        }
        if lat_gather is not None:
            full["latency_ms"]["with_gather"] = {"p50": round(float(np.percentile(lat_gather, 50)), 4), "p99": round(float(np.percentile(lat_gather, 99)), 4),
                                                 "frames": len(lat_gather), "mode": "serial, submit -> frame's slot all-gathered over RCCL -> sync"}
        if cpu:
            full["gpu_over_cpu"] = round(fps / world / cpu["value"], 1)
            full["gpu_over_one_cpu_core"] = round(fps / world / cpu["one_core"]["value"], 1)

    line = None
    if rank == 0:
        line = {
            "metric": "frames/sec, 640x640 batch-1 (p99 latency alongside)" if S == 640 else f"frames/sec, {S}x{S} batch-1",
            "value": round(fps, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 5), "block_ms": round(1e3 * dt, 3),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dname, "data": "synthetic",
            "config": {"workload": f"unina-yolo-dla-m graph {args.variant} {args.precision}, batch=1, {S}x{S}, NMS on-GPU" + (" (BASELINE configs[1])" if args.variant == "A" and S == 640 and args.precision == "fp16" else ""),
                       "frames_in_flight_per_gpu": IN_FLIGHT, "parallelism": f"replica x{world}, RCCL all-gather of detection slots every {GATHER_EVERY} frames on a comm stream ({GATHER_BANKS} banks)" if world > 1 else "1 GPU",
                       "distinct_frames": n_frames,
                       "thresholds": {"conf": conf, "iou": 0.45, "conformal_q": 0.1}, "detections_last_frame": n_det},
            **full,
        }
        if world > 1:
            line["config"]["gathered_frames"] = gathered_frames[0]
    for e in engines:
        e.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if line is not None:
        print(json.dumps(line))


def dump_detections(out_dir, slot, rank=0):
    """The detections a caller of the timed path receives for its last frame (the int32 result slot unina_infer_async
    filled: count, then GpuDetection records) -> out_dir/detections.npy, float32 [n, 6] = x1, y1, x2, y2, confidence,
    class_id in the kernel's output order (rank r > 0: detections_rank<r>.npy)."""
    from unina_yolo_dla_amd.engine import Engine
    det = Engine.unpack(slot)
    arr = np.stack([det[f].astype(np.float32) for f in ("x1", "y1", "x2", "y2", "confidence", "class_id")], axis=1)
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "detections.npy" if rank == 0 else f"detections_rank{rank}.npy"), arr.reshape(-1, 6))


def _kernel_key(name: str):
    """(function name, integer template arguments) of a kernel, from the engine's display name
    ('conv_glds<f16,32,64,64,1,4,4>', 'c3k2_fused<128,4x8,2,256,8w>'), the Itanium-mangled symbol or the demangled
    signature rocprofv3 reports ('void unina::c3k2_fused_kernel<128, 4, 8, 2, 256, 8, 16>(unina::C3k2Params)')."""
    import re
    m = re.match(r"_ZN5unina(\d+)", name)
    if m:
        n = int(m.group(1))
        fn = name[m.end():m.end() + n]
        return fn, tuple(int(x) for x in re.findall(r"Li(\d+)E", name))
    name = name.replace("void ", "").replace("unina::", "")
    fn = name.split("<")[0].split("(")[0].strip()
    args = name.split("<", 1)[1].rsplit(">", 1)[0] if "<" in name else ""
    return fn, tuple(int(x) for x in re.findall(r"\d+", re.sub(r"\bf16\b|\bf32\b|\bi8\b", "", args)))


def pmc_traffic(config: str, kernel: str):
    """HBM-side bytes per launch of `kernel` IN THE CONFIGURATION `config` ("variant:precision:size") from the committed
    rocprofv3 PMC summary (FETCH_SIZE x2 + WRITE_SIZE, MI355X_MICROARCH.md HBM section; tools/pmc_traffic.sh), or None when
    that configuration was not profiled -- a kernel name alone does not identify the launch (the same instantiation runs on
    other shapes in other configs). Names are matched on (function, leading template integers)."""
    try:
        with open(PMC_TRAFFIC) as f:
            table = json.load(f).get("configs", {}).get(config)
    except (OSError, ValueError):
        return None
    if not table:
        return None
    fn, nums = _kernel_key(kernel)
    for k, v in table.items():
        kfn, knums = _kernel_key(k)
        if (kfn.startswith(fn) and nums and knums[:len(nums)] == nums) or (kfn == fn and not knums):
            return v.get("hbm_bytes_per_launch")
    return None


def cpu_baseline(u, sd, S, conf, budget_s, variant="A"):
    """The CPU oracle (a port of the reference's fp32 forward + greedy NMS: AVX2 / AVX-512 register-tiled conv, OpenMP)
    timed on this box's host cores, on a bounded sample of the same workload: one core, then 8 / 16 / 32 / 64 threads;
    `value` is the best of them. Checker code, timed here only as the reported baseline. For scale: the reference
    model.py under torch / oneDNN in the dev container took 87-130 ms on 8 threads and 352 ms on one;
    this port took 102-111 ms and 555-680 ms there."""
    from oracle import oracle
    oracle.build()
    osd = oracle.StateDict(sd)
    ncpu = oracle.usable_cpus()          # affinity + cgroup quota, not the host's count
    x = u.rng.frame(1234, S, S)

    def timed(threads, max_frames, seconds, min_frames=1):
        def one():
            o = oracle.forward(osd, x, nthreads=threads, variant=variant)
            oracle.postprocess([o[n] for n in u.graph.OUTPUT_NAMES], conf, 0.45, 0.1)
        one()                                           # warm-up (scratch growth, thread pool)
        times = []
        t_end = time.perf_counter() + seconds
        while len(times) < max_frames and (len(times) < min_frames or time.perf_counter() < t_end):
            a = time.perf_counter()
            one()
            times.append(time.perf_counter() - a)
        return np.array(times)

    one_core = timed(1, 10, 0.25 * budget_s, min_frames=10 if S <= 640 else 3)      # (~0.2 s per frame at 640^2)
    sweep = {}
    for t in sorted({t for t in (8, 16, 32, 64) if t <= ncpu} | {min(ncpu, 64)}):
        sweep[t] = timed(t, 5, 0.1 * budget_s)
    best_t = min(sweep, key=lambda t: float(sweep[t].mean()))
    times = np.concatenate([sweep[best_t], timed(best_t, 50, 0.4 * budget_s)])
    osd.close()
    return {"value": round(1.0 / float(times.mean()), 3), "unit": "frames/s", "cores": best_t, "kind": "port",
            "sample": f"{len(times)} frames of {S}x{S} (same weights/frame), fp32 forward + decode/NMS, best of {sorted(sweep)} threads on {ncpu} usable CPUs",
            "ms_per_frame": round(1e3 * float(times.mean()), 2), "p99_ms": round(1e3 * float(np.percentile(times, 99)), 2),
            "one_core": {"value": round(1.0 / float(one_core.mean()), 3), "ms_per_frame": round(1e3 * float(one_core.mean()), 1),
                         "frames": len(one_core)},
            "by_threads_ms": {str(t): round(1e3 * float(v.mean()), 2) for t, v in sweep.items()}}


if __name__ == "__main__":
    main()
