"""csrc/cloud_io.h without a GPU: its host checks -- cloud_ok, extrinsic_ok, cloud_vec16 -- compiled by g++ (tests/cloud_io_host.cpp,
also under -fsanitize=address,undefined as the stand-alone program it is) on the bad clouds and extrinsics of tests/clouds.py and on
the good edges, against the same predicates written here."""
import struct

import numpy as np

import clouds
import hostprog
from lidar_cases import MOUNTED

BASE = 0x30000                      # a 16-byte boundary


def test_host_checks_equal_the_predicates_on_every_bad_argument_and_good_edge(tmp_path):
    bad = clouds.bad_cloud_args(MOUNTED) + [dict(n_points=1, points=0)]
    good = [dict(), dict(n_points=0, points=0), dict(n_points=0), dict(n_points=clouds.MAX_POINTS), dict(n_points=1, stride=12),
            *[dict(points=BASE + off, stride=stride) for off in (0, 4, 8, 12) for stride in (12, 16, 32, 48)],
            dict(m=[3e38] * 12), dict(m=[-0.0] * 12), dict(m=[1e-45] * 12)]
    cases = [dict(dict(clouds.CLOUD, m=MOUNTED), **kw) for kw in bad + good]
    payload = struct.pack("<2i", 0x434c4431, len(cases))
    for c in cases:
        payload += struct.pack("<2iq2i12f", c["n_points"], c["stride"], c["points"], clouds.MAX_POINTS, 0, *c["m"])
    _, said = hostprog.run_pair(hostprog.build_pair(tmp_path, "cloud_io_host.cpp"), tmp_path, payload, dtype=None, stdout=True)
    lines = [tuple(int(v) for v in line.split()) for line in said.splitlines()]
    assert lines.pop() == (0, 0) and len(lines) == len(cases)                      # NULL is neither a cloud nor an extrinsic
    for c, got in zip(cases, lines):
        n, stride, points = c["n_points"], c["stride"], c["points"]
        cloud_ok = 0 <= n <= clouds.MAX_POINTS and (n == 0 or points != 0) and stride >= 12 and stride % 4 == 0 and points % 4 == 0
        extrinsic_ok = all(np.isfinite(np.float32(v)) for v in c["m"])
        assert got == (int(cloud_ok), int(extrinsic_ok), int(stride % 16 == 0 and points % 16 == 0)), c
    assert not any(a and b for a, b, _ in lines[:len(bad)]) and all(a and b for a, b, _ in lines[len(bad):])
    taken = [(c["points"] - BASE, c["stride"]) for c, got in zip(cases, lines) if got[2] and c["points"] >= BASE]
    assert taken == [(0, 16), (0, 32), (0, 48)]                                    # only these take the 16-byte loads
