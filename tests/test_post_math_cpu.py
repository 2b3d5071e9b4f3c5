"""csrc/post_math.h without a GPU: the arithmetic csrc/postprocess.hip calls for the tile layout, the confidence bins, the packed
(class | enumeration index) field and the key ranges of the top-MAX_DETECTIONS cut, compiled for the host
(tests/post_math_host.cpp, also under -fsanitize=address,undefined as the stand-alone program it is) and held against
definitions written out here and against cut_model of tests/test_post_cases_cpu.py."""
import numpy as np
import pytest

import hostprog
import post_cases as pc
from test_post_cases_cpu import cut_model

F = np.float32
CLASSES = (-1, 0, 1, 16382)
INDICES = (0, 1, 2 ** 18 - 1)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("post_math_host")
    return hostprog.build_pair(d, "post_math_host.cpp"), d


@pytest.fixture(scope="module")
def rows(drivers):
    """The driver's output by line tag; both builds must exit 0 and print the same."""
    got = {}
    for line in hostprog.run_pair(*drivers, None, stdout=True)[1].splitlines():
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
