#!/usr/bin/env python3
"""In-kernel phase stamps of the two stand-alone stride-2 stage convs (backbone.stage2_conv, backbone.stage3_conv) under the
register-queue configurations the frame runs them in: the mid workgroup's shader clock at entry, requests issued, patch landed
(barrier passed), first MFMA issued, K loop end, stores drained (conv3x3_regq's stamped twin,
unina_debug_conv_stamps). Medians over REPS launches, in shader-clock ticks and in us at the measured clock; next to them the
event-timed duration of the product kernel.
usage: regq_phases.py [height width] [config substring ...]   (default 640 640 and the two configurations of the 640^2 frame)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import unina_yolo_dla_amd as u
from unina_yolo_dla_amd.engine import Engine

REPS = 15
OPS = {"backbone.stage2_conv": ["<f16,8x8,64,64,8w,s2>", "<f16,8x16,64,64,8w,s2>"],
       "backbone.stage3_conv": ["<f16,8x8,32,128,8w,s2>", "<f16,8x8,64,128,8w,s2>", "<f16,4x8,64,128,8w,s2>"]}
PHASES = ("requests", "patch landed", "first MFMA", "K loop", "stores drained")

args = sys.argv[1:]
h, w = (int(args[0]), int(args[1])) if len(args) >= 2 and args[0].isdigit() else (640, 640)
g = u.graph.Graph(in_h=h, in_w=w)
e = Engine.from_state_dict(u.synth.make_state_dict(7, g), g)
e.set_fusion(True)
e.forward(torch.from_numpy(u.rng.frame(1234, h, w)).cuda())
names = e.conv_configs()
infos = e.op_infos()
print(f"regq_phases: {h}x{w} frame, fp16, medians of {REPS} stamped launches")
for op, wanted in OPS.items():
    i = [k for k, o in enumerate(infos) if o["name"] == op][0]
    print(f"op {i}: {op}  M{infos[i]['m']} N{infos[i]['n']} K{infos[i]['k']}")
    for sub in wanted:
        cfg = [c for c, n in enumerate(names) if n.startswith("conv3x3_regq") and n.endswith(sub)]
        if not cfg or not e.set_op_config(i, cfg[0]):
            continue
        info = e.profile_ops(50)[i]
        rows = []
        for _ in range(REPS):
            st = e.conv_stamps(i)
            if st[7] == 0 or st[4] == 0:
                continue
            t = [st[0], st[1], st[2], st[7], st[3], st[4]]
            ghz = (st[4] - st[0]) / max(1, st[6] - st[5]) * 0.1
            rows.append([t[k + 1] - t[k] for k in range(5)] + [t[5] - t[0], ghz])
        if not rows:
            print(f"   {names[cfg[0]]}: no stamps (no stamped twin for this configuration)")
            continue
        med = np.median(np.array(rows, dtype=np.float64), axis=0)
        ghz = med[6]
        print(f"   {names[cfg[0]]:40s} grid {info['grid']:4d}  event-timed {info['ms'] * 1e3:6.2f} us | mid workgroup {med[5]:6.0f} ticks = {med[5] / ghz / 1e3:5.2f} us at {ghz:.2f} GHz")
        for name, v in zip(PHASES, med[:5]):
            print(f"        {name:15s} +{v:6.0f} ticks  {v / ghz / 1e3:5.2f} us")
    e.set_op_config(i, -1)
e.close()
