"""csrc/post_math.h without a GPU: the arithmetic csrc/postprocess.hip calls for the tile layout, the confidence bins, the packed
(class | enumeration index) field and the key ranges of the top-MAX_DETECTIONS cut, compiled for the host
(tests/post_math_host.cpp, also under -fsanitize=address,undefined as the stand-alone program it is) and held against
definitions written out here and against cut_model of tests/test_post_cases_cpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import post_cases as pc
from test_post_cases_cpu import cut_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "post_math_host.cpp")
F = np.float32
CLASSES = (-1, 0, 1, 16382)
INDICES = (0, 1, 2 ** 18 - 1)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """The driver's output by line tag; both builds must exit 0 and print the same."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/post_math_host.cpp"
    d = tmp_path_factory.mktemp("post_math_host")
    outs = []
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", *extra, SRC, "-o", exe], check=True, cwd=ROOT)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    got = {}
    for line in outs[0].splitlines():
        tag, *v = line.split()
        got.setdefault(tag, []).append(tuple(int(x) for x in v))
    return got


def test_tile_of_walks_the_triangle_row_major(rows):
    want = []
    for nw in range(1, 17):
        pairs = [(c, w) for c in range(nw) for w in range(c, nw)]
        off = np.concatenate([[0], np.cumsum([64 * (nw - c) for c in range(nw)])])
        want += [(nw, t, c, w, int(off[c])) for t, (c, w) in enumerate(pairs)]
    assert rows["tile"] == want and len(want) == sum(nw * (nw + 1) // 2 for nw in range(1, 17))


def test_conf_bin_edges(rows):
    assert pc.BINS == 4096
    assert rows["bin"] == [(k, min(k, 4095), k - 1) for k in range(4097)]
    assert rows["one"] == [(4095,)]


def test_pack_ce_round_trip_and_class_equality(rows):
    assert rows["ce"] == [(c, e, c, e) for c in CLASSES for e in INDICES]
    assert rows["same"] == [(a, b, int(a == b)) for a in CLASSES for b in CLASSES for _ in INDICES for _ in INDICES]


def test_cut_arithmetic_is_cut_models(rows):
    """MAX_DET + 1 equal confidences at the bottom of bin T put the cut into bin T with more members than are ranked exactly:
    the model takes the bin's key range and splits it."""
    assert [r[0] for r in rows["cut"]] == list(range(pc.BINS))
    for T, klo, khi, wdt in rows["cut"]:
        model, bins, _ = cut_model(np.full(pc.MAX_DET + 1, F(T) / F(pc.BINS), F))
        assert model["T"] == T and bins[0] == T and model["cnt"] > pc.MEM_CAP
        assert (model["klo0"], model["khi0"], model["wdt0"]) == (klo, khi, wdt), T
    assert rows["cut"][-1][2] == 0x3F800001 and rows["cut"][0][1] == 0
