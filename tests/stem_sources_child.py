"""Run as a script by tests/test_gpu_stem_sources.py: stem_source_cases.child_cases() in a fresh process, because UNINA_STEM_V1
(the one-thread-per-pixel stem) is read once per process.

  python tests/stem_sources_child.py <out.npz>   runs every child case through its camera call on the seed-7 FP16 engine of its
                                                 network size and stores, per case k, the detection records (det<k>) and the stem
                                                 buffer (stem<k>; a tiled call leaves its last tile's), and per size the stem
                                                 kernel's name (kernel_<H>x<W>)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, ROOT)
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import camera as twin, engine
    import stem_source_cases as S
    sd = u.synth.make_state_dict(7, u.graph.Graph())
    out = {}
    engines = {}
    try:
        for k, c in enumerate(S.child_cases()):
            if c.size not in engines:
                e = engines[c.size] = engine.Engine.from_state_dict(sd, u.graph.Graph(in_h=c.size[0], in_w=c.size[1]))
                out["kernel_" + S.SIZE_ID(c.size)] = np.array([o["kernel"] for o in e.op_infos() if o["kernel"].startswith("stem_")][0])
            e = engines[c.size]
            out[f"det{k}"] = S.call(e, c, S.device_frame(torch, engine, twin, c))
            out[f"stem{k}"] = e.read_buffer("backbone.stem")
    finally:
        for e in engines.values():
            e.close()
    np.savez(sys.argv[1], **out)
    print("STEM_SOURCES_CHILD_OK")


if __name__ == "__main__":
    main()
