#!/usr/bin/env python3
"""Stores what the REFERENCE's own decode / NMS header returns on the reference model's 640x640 head tensors, so that
the oracle's restatement is held to it bit for bit wherever the tests run (tests/test_oracle_golden.py).

    make -C oracle ref && python tests/golden/make_golden_ref_post.py     (needs oracle/_ref, i.e. the reference tree)

Input: the six heads of tests/golden/frame640_seed1234.npz (made by make_golden.py with the reference model.py).
Output (data only): tests/golden/ref_post_frame640_seed1234.npz -- for every (conf, iou, conformal_q) of SETTINGS the
reference header's detection records (x1, y1, x2, y2, confidence, class_id) in its own output order and its candidate
count, under the keys dets_<tag> / ncand_<tag> (tag() below).
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
OUT = "ref_post_frame640_seed1234.npz"
SETTINGS = [(0.5, 0.45, 0.1), (0.3, 0.2, 0.0), (0.2, 0.6, 0.25)]     # (conf, iou, conformal_q)


def tag(conf, iou, q):
    return f"conf{conf}_iou{iou}_q{q}"


def main():
    import unina_yolo_dla_amd as u
    from oracle import oracle
    if not oracle.have_ref():
        sys.exit("oracle/_ref absent: build it first (make -C oracle ref, needs the reference tree)")
    gold = np.load(os.path.join(GOLD, "frame640_seed1234.npz"), allow_pickle=False)
    heads = [gold[f"head/{n}"] for n in u.graph.OUTPUT_NAMES]
    blob = {}
    for conf, iou, q in SETTINGS:
        dets, ncand = oracle.ref_postprocess(heads, conf, iou, q)
        blob[f"dets_{tag(conf, iou, q)}"] = dets
        blob[f"ncand_{tag(conf, iou, q)}"] = np.array(ncand)
        print(f"{tag(conf, iou, q)}: {len(dets)} detections of {ncand} candidates")
    np.savez_compressed(os.path.join(GOLD, OUT), **blob)


if __name__ == "__main__":
    main()
