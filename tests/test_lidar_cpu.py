"""unina_locate_lidar_async without a GPU: csrc/lidar_project.h compiled for the host (tests/lidar_project_host.cpp, also under
-fsanitize=address,undefined as the stand-alone program it is) against localize.project_lidar_numpy; localize.locate_lidar_numpy
(the definition) against the depth route on the map a cloud rasterises to, and on constructed cases whose content is asserted
here; the argument checks of the entry points; the record layouts in C."""
import ctypes as C
import struct

import numpy as np
import pytest

import clouds
import hostprog
import lidar_cases as lc
import locate_cases
from clouds import ulp

F = np.float32


def twin(c):
    from unina_yolo_dla_amd import localize
    return localize.locate_lidar_numpy(c["dets"], c["count"], c["points"], c["m"], c["cam"], c["width"], c["height"], c["params"])


def pixels_of(c):
    from unina_yolo_dla_amd import localize
    p = c["params"]
    return localize.project_lidar_numpy(c["points"], c["m"], c["cam"], c["width"], c["height"], p["min_depth"], p["max_depth"])


# ---------------------------------------------------------------- csrc/lidar_project.h on the host
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("lidar_project_host")
    return hostprog.build_pair(d, "lidar_project_host.cpp"), d


def host_project(drivers, points, m, cam, width, height, min_depth, max_depth):
    """-> (LIDAR_PIXEL_DTYPE records, cells) from both builds of the host program."""
    from unina_yolo_dla_amd import engine
    pts = np.ascontiguousarray(points, dtype=np.float32)
    payload = struct.pack("<2i", 0x4c445231, len(pts)) + struct.pack("<16f2i2f", *m, *cam, width, height, min_depth, max_depth) + pts.tobytes()
    got = hostprog.run_pair(*drivers, payload).reshape(-1, 5)
    assert len(got) == len(pts)
    return np.ascontiguousarray(got[:, :4]).view(engine.LIDAR_PIXEL_DTYPE).reshape(-1), got[:, 4]


def test_host_projection_equals_the_twin_on_every_special_value(pkg, drivers):
    """Through the identity and fx = fy = 1, cx = cy = 0 a point (x, y, 1) has u = x and v = y, and (0, 0, z) has zc = z: NaN and
    +-inf coordinates; zc of -0.0, 0, negative, denormal and tiny positive (u overflows); u of -0.0, exactly integer, the largest
    float below `width`, exactly `width`; zc on and one ulp outside both depth bounds. Byte equality with project_lidar_numpy, and
    the content of each row."""
    from unina_yolo_dla_amd import localize
    nan, inf = np.nan, np.inf
    width, height, lo, hi = 100, 70, F(0.3), F(40.0)
    rows = [
        ((nan, 1, 1), None), ((1, nan, 1), None), ((1, 1, nan), None), ((inf, 1, 1), None), ((1, -inf, 1), None), ((1, 1, inf), None),
        ((1, 1, -inf), None), ((3e38, 3e38, 1), None),
        ((1, 1, -0.0), None), ((1, 1, 0.0), None), ((1, 1, -2.0), None), ((0, 0, 1e-40), (0, 0, 0)), ((1, 1, 1e-40), None),
        ((1e-3, 1e-3, 1e-37), None),                                              # u = 1e34: off the image; with x = 1 it overflows
        ((1, 1, 1e-37), None), ((3e38, 0, 0.5), None),
        ((-0.0, -0.0, 1), (0, 0, 1)), ((0.0, 0.0, 1), (0, 0, 1)), ((5.0, 7.0, 1), (5, 7, 1)), ((ulp(5, 0), ulp(7, 0), 1), (4, 6, 1)),
        ((ulp(100, 0), ulp(70, 0), 1), (99, 69, 1)), ((100.0, 1, 1), None), ((1, 70.0, 1), None), ((ulp(0, -1), 1, 1), None),
        ((-1e-30, 1, 1), None), ((99.5, 69.5, 1), (99, 69, 1)),
        ((0, 0, lo), (0, 0, 1)), ((0, 0, ulp(lo, 0)), (0, 0, 0)), ((0, 0, ulp(lo, 1)), (0, 0, 1)),
        ((0, 0, hi), (0, 0, 1)), ((0, 0, ulp(hi, 100)), (0, 0, 0)), ((0, 0, ulp(hi, 0)), (0, 0, 1)), ((0, 0, 3e38), (0, 0, 0)),
    ]
    pts = np.array([r[0] for r in rows], dtype=np.float32)
    for cam in ((1.0, 1.0, 0.0, 0.0), (1.0, 1.0, -0.0, -0.0)):
        want = localize.project_lidar_numpy(pts, lc.IDENTITY, cam, width, height, lo, hi)
        got, cells = host_project(drivers, pts, lc.IDENTITY, cam, width, height, lo, hi)
        assert got.tobytes() == want.tobytes()
        for (xyz, expect), w, cell in zip(rows, want, cells):
            if expect is None:
                assert w.tolist() == (0, 0, 0, 0) and cell == -1, xyz
            else:
                u, v, has_key = expect
                assert (w["u"], w["v"], w["projectable"]) == (u, v, 1) and cell == (v // 32) * 4 + u // 32, xyz
                assert w["key"] == (F(xyz[2]).view(np.uint32) if has_key else 0), xyz
    # a width that the float test and the integer conversion must agree on at the limit
    big = np.array([(ulp(16384, 0), ulp(16384, 0), 1), (16384.0, 0, 1), (16383.0, 16383.0, 1)], dtype=np.float32)
    want = localize.project_lidar_numpy(big, lc.IDENTITY, (1.0, 1.0, 0.0, 0.0), 16384, 16384, lo, hi)
    got, cells = host_project(drivers, big, lc.IDENTITY, (1.0, 1.0, 0.0, 0.0), 16384, 16384, lo, hi)
    assert got.tobytes() == want.tobytes() and want["u"].tolist() == [16383, 0, 16383] and want["projectable"].tolist() == [1, 0, 1]
    assert cells.tolist() == [512 * 512 - 1, -1, 512 * 512 - 1]


def test_host_projection_equals_the_twin_through_a_mounted_lidar(pkg, drivers):
    """LiDAR x forward / z up -> camera z forward / y down, rotated and translated: a point 10 m ahead, 1 m to the left and 0.3 m
    above the LiDAR's origin is at (-0.98, 0, 9.9) in the camera; then random clouds, spoiled points included, through the mounted
    extrinsic, through one with no zero element, and on three image sizes."""
    from unina_yolo_dla_amd import localize
    one = np.array([[10.0, 1.0, 0.3]], dtype=np.float32)
    px = localize.project_lidar_numpy(one, lc.MOUNTED, lc.CAM, lc.W, lc.H, 0.3, 40.0)[0]
    assert px["key"] == F(F(10.0) + F(-0.1)).view(np.uint32) and px["projectable"] == 1
    assert px["u"] == int(F(70.0) * F(-0.98) / F(9.9) + F(48.25)) and px["v"] == 30
    a, b = np.deg2rad(7.0), np.deg2rad(-3.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    base = np.asarray(lc.MOUNTED).reshape(3, 4)
    tilted = np.concatenate([rx @ rz @ base[:, :3], [[0.031], [0.287], [-0.113]]], axis=1).reshape(-1).tolist()
    n_seen = 0
    for m in (lc.MOUNTED, tilted):
        for (w, h, cam) in ((lc.W, lc.H, lc.CAM), (1920, 1080, (1400.0, 1399.0, 959.5, 539.5)), (33, 1, (20.0, 20.0, 16.0, 0.5))):
            pts = lc.random_cloud(5, 4000, w, h, cam=cam)
            want = localize.project_lidar_numpy(pts, m, cam, w, h, 0.3, 40.0)
            got, cells = host_project(drivers, pts, m, cam, w, h, 0.3, 40.0)
            assert got.tobytes() == want.tobytes(), (m, w, h)
            ok = want["projectable"] == 1
            assert (cells[ok] == (want["v"][ok] // 32) * ((w + 31) // 32) + want["u"][ok] // 32).all() and (cells[~ok] == -1).all()
            n_seen += ok.sum()
            assert (want["key"][ok] == 0).sum() > 10 or h == 1                   # some members are out of the depth range
    assert n_seen > 8000


# ---------------------------------------------------------------- the definition against the depth route
def test_a_rasterised_cloud_gives_the_depth_routes_records(pkg):
    """A 96 x 80 depth map (tests/locate_cases.py: 13 % of the pixels are holes of every kind), one point per pixel whose depth is
    finite and positive, in shuffled order, identity extrinsic, 40 random boxes: x, y, z, u, v, n_valid and valid are bit-equal to
    locate_numpy's on the map. Only n_samples differs: the depth route counts the holes."""
    from unina_yolo_dla_amd import engine, localize
    w, h = 96, 80
    cam = (64.0, 64.0, 0.0, 0.0)
    depth = locate_cases.depth_map(9, engine.DEPTH_F32, h, w, holes=0.13)
    vv, uu = np.nonzero(np.isfinite(depth) & (depth > 0))
    order = np.random.RandomState(3).permutation(len(uu))
    pts, placed = lc.place(np.stack([uu, vv, depth[vv, uu].astype(np.float64)], axis=1)[order])
    assert 6800 < len(pts) < 7100
    px = localize.project_lidar_numpy(pts, lc.IDENTITY, cam, w, h, 0.3, 40.0)
    assert (px["projectable"] == 1).all() and (px["u"] == placed[:, 0]).all() and (px["v"] == placed[:, 1]).all()
    dets = locate_cases.random_boxes(17, 40, w, h)
    common = dict(sx=1.0, sy=1.0, shrink=0.6, min_depth=0.3, max_depth=40.0, min_valid=2)
    got = localize.locate_lidar_numpy(dets, 40, pts, lc.IDENTITY, cam, w, h, common)
    want = localize.locate_numpy(dets, 40, depth, engine.DEPTH_F32, 1.0, cam, dict(common, max_side=256))
    for name in ("x", "y", "z", "u", "v", "n_valid", "valid"):
        assert got[name].tobytes() == want[name].tobytes(), name
    assert (got["n_samples"] <= want["n_samples"]).all() and (got["n_samples"] < want["n_samples"]).sum() > 10
    assert (got["valid"] == 1).sum() > 20 and (got["valid"][:40] == 0).sum() > 2 and not got[40:].view(np.uint8).any()


# ---------------------------------------------------------------- the constructed cases contain what their names say
def test_placed_points_land_where_they_were_put(pkg):
    for c in (lc.members_case(), lc.keys_case()):
        px = pixels_of(c)
        assert (px["projectable"] == 1).all()
        assert (px["u"] == c["placed"][:, 0]).all() and (px["v"] == c["placed"][:, 1]).all()
        z = c["placed"][:, 2].astype(np.uint32).view(np.float32)
        in_range = (z >= F(0.3)) & (z <= F(40.0))
        assert (px["key"] == np.where(in_range, c["placed"][:, 2], 0)).all()


def candidates(c, px, i):
    """Points in the 32 x 32 cells that record i's window touches: what csrc/lidar.hip's select kernel reads for it."""
    from unina_yolo_dla_amd import localize
    d, p = c["dets"][i], c["params"]
    w = localize.window_numpy((d["x1"], d["y1"], d["x2"], d["y2"]), p["sx"], p["sy"], p["shrink"], c["width"], c["height"], 16384)
    ok = px["projectable"] == 1
    cu, cv = px["u"] >> 5, px["v"] >> 5
    return int((ok & (cu >= w["u0"] >> 5) & (cu <= w["u1"] >> 5) & (cv >= w["v0"] >> 5) & (cv <= w["v1"] >> 5)).sum())


def test_members_case_sits_on_every_threshold(pkg):
    c = lc.members_case()
    cones, px = twin(c), pixels_of(c)
    assert len(c["points"]) > 90000
    assert cones["n_samples"][:6].tolist() == [0, 1, 2, 63, 64, 65] and cones["n_valid"][:6].tolist() == [0, 1, 2, 63, 64, 65]
    assert cones["valid"][:6].tolist() == [0, 1, 1, 1, 1, 1] and cones["u"][0] == 7.75 and cones["z"][0] == 0
    assert [candidates(c, px, i) for i in range(6)] == [0, 1, 2, 63, 64, 65]
    assert [candidates(c, px, i) for i in (6, 7, 8, 9)] == [lc.WAVE_CANDIDATES, lc.WAVE_CANDIDATES + 1, 100, 64]
    assert cones["n_samples"][6:10].tolist() == [10, 10, 0, 64] and cones["n_valid"][6:10].tolist() == [10, 10, 0, 0]
    assert cones["valid"][6:10].tolist() == [1, 1, 0, 0]
    k = lc.CACHE_KEYS
    assert cones["n_valid"][10:13].tolist() == [k - 1, k, k + 1] and cones["n_samples"][10:13].tolist() == [k + 4, k + 5, k + 6]
    assert cones["n_samples"][13] == 66000 == cones["n_valid"][13] and (cones["valid"][10:14] == 1).all()
    for i in (3, 5, 11, 13):               # the median is the lower median of the depths that were put into the region
        z = np.sort(c["placed"][:, 2][(c["placed"][:, 0] // 64 == i % 8) & (c["placed"][:, 1] // 64 == i // 8)].astype(np.uint32).view(np.float32))
        z = z[(z >= F(0.3)) & (z <= F(40.0))]
        assert cones["z"][i] == z[(len(z) - 1) // 2], i
    assert not cones[14:].view(np.uint8).any()


def test_keys_case_selects_what_it_was_built_to_select(pkg):
    c = lc.keys_case()
    cones, px = twin(c), pixels_of(c)
    top = lc.bits_to_z([(b << 24) | 0x00123456 for b in (0x3f, 0x40, 0x41, 0x42)]).astype(np.float32)
    low = lc.bits_to_z([0x41200000 | b for b in range(256)]).astype(np.float32)
    for base, n in ((0, 40), (6, 600)):
        assert (candidates(c, px, base) <= lc.WAVE_CANDIDATES) == (n == 40)
        assert cones["z"][base] == 12.5 and cones["n_valid"][base] == n                   # all equal
        assert cones["z"][base + 1] == 3.0                                                    # two values, even count: the lower
        assert cones["z"][base + 2] == np.sort(np.resize(top, n))[(n - 1) // 2]
        assert cones["z"][base + 3] == np.sort(np.resize(low, n))[(n - 1) // 2]
        mixed = cones[base + 4]
        assert mixed["n_samples"] == n and mixed["n_valid"] < n // 2 and mixed["z"] == 7.0 and mixed["valid"] == 1
        assert cones["n_samples"][base + 5] == n and cones["n_valid"][base + 5] == n // 10
    assert cones["valid"][5] == 0 and cones["z"][5] == 0 and cones["u"][5] != 0              # 4 valid members, min_valid = 5
    assert cones["valid"][11] == 1 and cones["z"][11] == 6.0


def test_geometry_case_contains_its_windows(pkg):
    from unina_yolo_dla_amd import localize
    c = lc.geometry_case()
    cones, px = twin(c), pixels_of(c)
    n_proj = int((px["projectable"] == 1).sum())
    assert 1500 < n_proj < 2700 and ((px["projectable"] == 1) & (px["key"] == 0)).sum() > 100
    assert cones["n_samples"][7] == n_proj == cones["n_samples"][8]                          # the whole image, twice
    assert cones[9].tobytes() == cones[10].tobytes() and cones["n_samples"][9] > 100         # identical records share their points
    assert not cones[13:21].view(np.uint8).any()                                             # inverted, NaN, infinite, off the image
    assert cones["n_samples"][4] == ((px["projectable"] == 1) & (px["u"] >= 96)).sum() > 0   # the last partial cell column
    assert cones["n_samples"][5] == ((px["projectable"] == 1) & (px["v"] >= 64)).sum() > 0
    assert cones["u"][21] == 99.625 and cones["n_samples"][21] <= 2                          # one pixel in the image's corner
    w = localize.window_numpy((60, 60, 70, 68), 1.0, 1.0, 1.0, lc.W, lc.H, 16384)
    assert (w["u0"], w["u1"], w["v0"], w["v1"]) == (60, 70, 60, 68)                          # cells 1 .. 2 x 1 .. 2 of 32, 0 .. 1 x 0 .. 1 of 64


def test_scan_edge_cases_have_the_cell_counts_they_name(pkg):
    cases = lc.scan_edge_cases()
    assert tuple(((c["width"] + 31) // 32) * ((c["height"] + 31) // 32) for c in cases) == lc.SCAN_CELLS
    for c in cases:
        cones, px = twin(c), pixels_of(c)
        assert cones["n_samples"][20] == (px["projectable"] == 1).sum() > 100, c["name"]      # the whole image
        assert cones["valid"][20] == 1 and cones["u"][20] == c["width"] / 2


def test_empty_cloud_and_counts(pkg):
    c = lc.cloud_size_cases()[0]
    cones = twin(c)
    assert len(c["points"]) == 0 and (cones["n_samples"] == 0).all() and (cones["valid"] == 0).all()
    assert cones["u"][:3].tolist() == [50.0, 35.0, 74.5] and not cones[3:].view(np.uint8).any()
    got = {c["name"]: twin(c) for c in lc.count_cases()}
    assert not got["count0"].view(np.uint8).any() and not got["count_negative"].view(np.uint8).any()
    assert (got["count1"]["u"][:2] == [1.5, 0]).all() and got["count5000"].tobytes() == got["count1024"].tobytes()
    assert (got["count1024"]["u"] != 0).all() and (got["count1024"]["valid"] == 1).sum() > 200


def test_the_result_does_not_depend_on_the_order_of_the_cloud(pkg):
    c = lc.random_case(60, 3000)
    want = twin(c)
    shuffled = dict(c, points=c["points"][np.random.RandomState(1).permutation(len(c["points"]))])
    assert twin(shuffled).tobytes() == want.tobytes() and (want["valid"] == 1).sum() > 20


# ---------------------------------------------------------------- the entry points' argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the checks
    would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    h = C.c_void_p()
    for kw in (dict(device=-1), dict(points=0), dict(points=(1 << 22) + 1), dict(w=0), dict(w=16385), dict(h=0), dict(h=16385), dict(points=-1)):
        a = dict(dict(device=0, points=1000, w=1920, h=1080), **kw)
        assert L.unina_lidar_create(a["device"], a["points"], a["w"], a["h"], C.byref(h)) == 4 and not h.value, kw
    assert L.unina_lidar_create(0, 1000, 1920, 1080, None) == 4
    assert L.unina_lidar_create(0, 1 << 22, 16384, 16384, C.byref(h)) == 0 and h.value      # host only: no device is needed
    L.unina_lidar_destroy(h)
    L.unina_lidar_destroy(None)
    assert L.unina_lidar_create(0, clouds.MAX_POINTS, 1920, 1080, C.byref(h)) == 0
    assert L.unina_lidar_buffers(h, C.byref(C.c_void_p())) == 5 and L.unina_lidar_buffers(None, None) == 4   # UNINA_ERR_STATE: no call yet
    DETS, COUNT, OUT = 0x10000, 0x20000, 0x50000

    def invoke(f, mm, handle=h, dets=DETS, count=COUNT, out=OUT, cloud=True, ext=True, cam=True, par=True, width=640, height=480):
        ss, cc, pp = engine.Cloud(**f["cloud"]), engine.Pinhole(**f["cam"]), engine.LidarParams(**f["par"])
        return L.unina_locate_lidar_async(handle, dets, count, C.byref(ss) if cloud else None, C.byref(mm) if ext else None,
                                          C.byref(cc) if cam else None, width, height, C.byref(pp) if par else None, out, None)

    call = clouds.caller(invoke, lc.MOUNTED, cam=dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0),
                         par=dict(sx=1.0, sy=1.0, shrink=0.5, min_depth=0.5, max_depth=40.0, min_valid=1))
    bad = [dict(handle=None), dict(dets=None), dict(count=None), dict(out=None), dict(cloud=False), dict(ext=False), dict(cam=False), dict(par=False),
           dict(points=None), dict(out=OUT + 8), dict(dets=DETS + 4), dict(count=COUNT + 2), *clouds.bad_cloud_args(lc.MOUNTED),
           dict(width=0), dict(width=-3), dict(width=1921), dict(height=0), dict(height=1081),
           *[{k: v} for k in ("fx", "fy", "sx", "sy") for v in (0.0, -1.0, nan, inf)],
           *[{k: v} for k in ("cx", "cy") for v in (nan, inf, -inf)],
           dict(shrink=0.0), dict(shrink=-0.5), dict(shrink=1.0001), dict(shrink=nan),
           dict(min_depth=0.0), dict(min_depth=-1.0), dict(min_depth=nan), dict(min_depth=40.0), dict(min_depth=50.0),
           dict(max_depth=inf), dict(max_depth=nan), dict(min_valid=-1)]
    for kw in bad:
        assert call(**kw) == 4, kw
    import torch
    if not torch.cuda.is_available():
        # good calls reach HIP, which has no device here: the checks above sit in front of it
        assert call() == 3 and call(n_points=0, points=None) == 3 and call(n_points=1000, stride=12) == 3
        assert call(width=1920, height=1080, stride=48, min_valid=0) == 3
        assert L.unina_lidar_buffers(h, C.byref(C.c_void_p())) == 5                         # still no workspace
    L.unina_lidar_destroy(h)


def test_twin_refuses_malformed_input(pkg):
    from unina_yolo_dla_amd import localize
    pts = np.zeros((4, 3), dtype=np.float32)
    for bad in (dict(points=pts.astype(np.float64)), dict(points=pts[:, :2]), dict(width=0), dict(height=16385), dict(m=lc.IDENTITY[:11])):
        a = dict(dict(points=pts, m=lc.IDENTITY, width=10, height=10), **bad)
        with pytest.raises(ValueError):
            localize.project_lidar_numpy(a["points"], a["m"], lc.CAM, a["width"], a["height"], 0.3, 40.0)


def test_records_are_plain_c_of_the_stated_sizes(pkg, tmp_path):
    from unina_yolo_dla_amd import engine
    assert engine.LIDAR_PIXEL_DTYPE.itemsize == 16
    assert [engine.LIDAR_PIXEL_DTYPE.fields[n][1] for n in ("u", "v", "key", "projectable")] == [0, 4, 8, 12]
    assert C.sizeof(engine.LidarParams) == 24 and C.sizeof(engine.Cloud) == 16
    assert (engine.LIDAR_MAX_DIM, engine.LIDAR_MAX_POINTS) == (16384, 1 << 22)
    hostprog.compile_c99(tmp_path, 'typedef char pixel16[(sizeof(unina_lidar_pixel) == 16) ? 1 : -1];\n'
                                   'typedef char key8[(offsetof(unina_lidar_pixel, key) == 8) ? 1 : -1];\n'
                                   'typedef char par24[(sizeof(unina_lidar_params) == 24) ? 1 : -1];\n'
                                   'typedef char points8[(offsetof(unina_cloud, points) == 8) ? 1 : -1];\n'
                                   'typedef char lim[(UNINA_LIDAR_MAX_DIM == 16384 && UNINA_LIDAR_MAX_POINTS == 4194304) ? 1 : -1];\n'
                                   'int use(unina_lidar_t *l, const GpuDetection *d, const int *n, const void *sweep, unina_cone3d *o) {\n'
                                   '  unina_cloud c = {131072, 16, 0};\n'
                                   '  const float m[12] = {0, -1, 0, 0, 0, 0, -1, 0.3f, 1, 0, 0, -0.1f};\n'
                                   '  unina_pinhole k = {1400.0f, 1400.0f, 959.5f, 539.5f};\n'
                                   '  unina_lidar_params p = {1.0f, 1.0f, 0.5f, 0.5f, 40.0f, 3};\n'
                                   '  const unina_lidar_pixel *px;\n'
                                   '  c.points = sweep;\n'
                                   '  if (unina_locate_lidar_async(l, d, n, &c, m, &k, 1920, 1080, &p, o, 0)) return 1;\n'
                                   '  return unina_lidar_buffers(l, &px);\n}\n')
