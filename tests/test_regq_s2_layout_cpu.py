"""The LDS image of the stride-2 register-queue 3x3 tiles (csrc/regq_s2.h), checked on the host for every stride-2 fp16 / int8
row of conv_igemm.hip's table: tests/regq_s2_layout_host.cpp enumerates the 64 lanes' addresses of every fragment read and
finds no two lanes of a ds_read_b128 lane group on one bank slot, every patch chunk fetched once into a slot of its own and every
read slot holding what the MFMA wants. Plain and sanitised build."""
import os
import re
import subprocess

import pytest

import hostprog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV = os.path.join(ROOT, "unina-yolo-dla_amd", "csrc", "conv_igemm.hip")
ESZ = {"half_t": 2, "signed char": 1}


def s2_tiles():
    """(element bytes, TH, TW, Cin, threads) of every stride-2 row that takes its patch through registers (not split fp16)."""
    rows = re.findall(r"t\.add<RegqTile<([\w ]+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), 2>>", open(CONV).read())
    assert any(r[0] == "s16_t" for r in rows)          # the split-fp16 rows exist and keep the stride-1 image
    return sorted({(ESZ[t], int(th), int(tw), int(cin), 64 * int(nw)) for t, th, tw, bn, cin, nw, d in rows if t in ESZ})


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return hostprog.build_pair(tmp_path_factory.mktemp("s2layout"), "regq_s2_layout_host.cpp")


def test_the_table_has_the_stage_convs_tiles():
    tiles = s2_tiles()
    assert (2, 8, 8, 64, 512) in tiles and (2, 8, 8, 128, 512) in tiles      # stage2_conv, stage3_conv (fp16)
    assert {t[0] for t in tiles} == {1, 2} and len(tiles) >= 9


def test_every_fragment_read_is_conflict_free_and_reads_what_was_stored(exes):
    tiles = s2_tiles()
    args = [str(v) for t in tiles for v in t]
    outs = []
    for exe in exes:
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        print(r.stdout)
        assert r.returncode == 0, r.stdout + r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].splitlines()
    assert len(lines) == len(tiles)
    for line in lines:
        m = re.search(r"extra LDS cycles per read: ([\d.]+) \(worst (\d+)\); stride-1 image: ([\d.]+)", line)
        assert m and float(m.group(1)) == 0.0 and int(m.group(2)) == 0, line
        assert float(m.group(3)) >= 4.0, line          # what the image replaces: 2-way or worse in every lane group


def test_a_tile_outside_the_scheme_is_reported(exes):
    for exe in exes:
        r = subprocess.run([exe, "2", "8", "12", "64", "512"], capture_output=True, text=True)
        assert r.returncode == 1 and "not covered" in r.stdout
