#!/usr/bin/env python3
"""Do the two frame streams of a two-frames-in-flight set-up run at the same time in THIS process's environment?

    python tools/stream_queues.py [--size 640] [--reps 3]

Loads two engine handles and then creates two torch.cuda.Stream()s, in bench.py's order, runs one frame on each, and prints
the overlap matrix of {null stream, stream 0, stream 1} (unina_debug_streams_overlap: repetitions of `reps` in which the 300 us
probe kernels of the two streams ran concurrently; the diagonal is the negative control and must be 0) and the number of streams
the library holds (unina_debug_owned_streams: 0). A 0 off the diagonal means the two streams share a hardware queue: see
INTEGRATION.md "Runtime settings" (GPU_MAX_HW_QUEUES). Exit status 1 when stream 0 and stream 1 do not overlap."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import engine as E, export

    torch.cuda.set_device(args.device)
    dev = torch.device("cuda", args.device)
    S = args.size
    g = u.graph.Graph(in_h=S, in_w=S)
    sd = u.synth.make_state_dict(7, g)
    fd, path = tempfile.mkstemp(suffix=".une")
    os.close(fd)
    try:
        export.export_engine(sd, path, g, export.FP16, None)
        engines = [E.Engine(path, device=args.device) for _ in range(2)]
    finally:
        os.unlink(path)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    frames = [torch.from_numpy(u.rng.frame(1234 + k, S, S)).to(dev) for k in range(2)]
    outs = [torch.zeros((8 + 8 * E.MAX_DETECTIONS,), dtype=torch.int32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            engines[k].infer_async(frames[k], 0.5, 0.45, 0.1, out=outs[k], stream=streams[k])
    torch.cuda.synchronize()

    names = ["null", "stream 0", "stream 1"]
    handles = [None, streams[0], streams[1]]
    print(f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', '(unset: the runtime default, 4)')}")
    print(f"repetitions of {args.reps} in which the two probe kernels overlapped:")
    print(" " * 10 + "".join(f"{n:>10}" for n in names))
    matrix = []
    for a, na in zip(handles, names):
        row = [E.streams_overlap(a, b, args.reps, args.device)[0] for b in handles]
        matrix.append(row)
        print(f"{na:>10}" + "".join(f"{v:>10}" for v in row))
    print(f"streams held by the library: {E.owned_streams()}")
    for e in engines:
        e.close()
    ok = matrix[1][2] == args.reps and matrix[2][1] == args.reps and all(matrix[i][i] == 0 for i in range(3))
    print("stream 0 and stream 1 overlap" if ok else "stream 0 and stream 1 do NOT overlap (or the control failed)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
