"""unina_ground_filter_async without a GPU: csrc/ground_cell.h compiled for the host (tests/ground_cell_host.cpp, also under
-fsanitize=address,undefined as the stand-alone program it is) against ground.ground_numpy, byte for byte, on special values, on
every threshold and on the constructed cases of tests/ground_cases.py, whose content is asserted here on the twin; the scene that
justifies the stage, on the twins of the two stages; the argument checks of the entry points; the record layouts in C."""
import ctypes as C
import struct

import numpy as np
import pytest

import clouds
import ground_cases as gc
import hostprog
from clouds import ulp

F = np.float32
EMPTY = 0xffffffff
NAN_WORD = 0x7fc00000
OUTSIDE, UNKNOWN, GROUND, OBJECT, ABOVE = range(5)


def twin(c):
    from unina_yolo_dla_amd import ground
    return ground.ground_numpy(c["points"], c["m"], c["params"])


def key(v):
    b = int(F(v).view(np.uint32))
    return b ^ (0xffffffff if b >> 31 else 0x80000000)


# ---------------------------------------------------------------- csrc/ground_cell.h on the host
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("ground_cell_host")
    return hostprog.build_pair(d, "ground_cell_host.cpp"), d


def host_ground(drivers, c):
    """Both builds of the host program on one case -> what ground_numpy returns, and the bits of zl and of h per point."""
    from unina_yolo_dla_amd import engine, ground
    pts = np.ascontiguousarray(c["points"][:, :3], dtype=np.float32)
    p = ground.as_ground_params(c["params"])
    payload = struct.pack("<2i", 0x47524e31, len(pts)) + struct.pack("<12f", *c["m"]) + bytes(p) + pts.tobytes()
    words = hostprog.run_pair(*drivers, payload).view(np.uint32)
    n, cells = len(pts), p.nx * p.ny
    assert len(words) == 8 + 4 * n + 2 * cells + 4 * n
    per_point = words[8:8 + 4 * n].reshape(n, 4)
    at = 8 + 4 * n
    return {"header": words[:8].view(engine.GROUND_HEADER_DTYPE), "cell": per_point[:, 0].astype(np.int32), "z_bits": per_point[:, 1],
            "labels": per_point[:, 2].astype(np.uint8), "h_bits": per_point[:, 3], "cellmin": words[at:at + cells].reshape(p.ny, p.nx),
            "ground": words[at + cells:at + 2 * cells].reshape(p.ny, p.nx), "out": words[at + 2 * cells:].reshape(n, 4).view(np.float32)}


def assert_host_equals_twin(drivers, c):
    got, want = host_ground(drivers, c), twin(c)
    for name in ("labels", "cell", "cellmin", "ground", "header", "out"):
        assert got[name].tobytes() == want[name].tobytes(), (c["name"], name)
    return want, got


def test_host_cells_equal_the_twin_on_every_special_value(pkg, drivers):
    """Through an identity whose zeros are negative (a product with them is a zero of the coordinate's sign, so -0.0 survives the
    sums) and a unit grid at the origin fx = x, fy = y and zl = z: NaN and +-inf in each coordinate; fx of -0.0,
    exactly integer, the largest float below nx, exactly nx, a negative denormal; zl on and one ulp beside z_lo and z_hi, which a
    cell of its own shows as a cellmin or as none. Byte equality with ground_numpy, and the content of each row."""
    nan, inf = np.nan, np.inf
    nx, ny, lo, hi = 100, 70, F(-0.75), F(0.375)
    rows = [
        ((nan, 1, 0), None), ((1, nan, 0), None), ((1, 1, nan), None), ((inf, 1, 0), None), ((1, -inf, 0), None), ((1, 1, inf), None),
        ((1, 1, -inf), None), ((3e38, 3e38, 0), None),
        ((-0.0, 0.5, 0), (0, 0, True)), ((0.5, -0.0, 0), (0, 0, True)), ((5.0, 7.0, 0), (5, 7, True)), ((ulp(5, 0), ulp(7, 0), 0), (4, 6, True)),
        ((ulp(100, 0), ulp(70, 0), 0), (99, 69, True)), ((100.0, 1, 0), None), ((1, 70.0, 0), None), ((ulp(0, -1), 1, 0), None),
        ((-1e-30, 1, 0), None), ((99.5, 0.5, 0), (99, 0, True)), ((0.5, 69.5, 0), (0, 69, True)),
        ((10.5, 10.5, lo), (10, 10, True)), ((11.5, 10.5, ulp(lo, -1)), (11, 10, False)), ((12.5, 10.5, ulp(lo, 0)), (12, 10, True)),
        ((13.5, 10.5, hi), (13, 10, True)), ((14.5, 10.5, ulp(hi, 1)), (14, 10, False)), ((15.5, 10.5, ulp(hi, 0)), (15, 10, True)),
        ((16.5, 10.5, 3e38), (16, 10, False)), ((17.5, 10.5, -3e38), (17, 10, False)),
    ]
    c = gc.case("special", [r[0] for r in rows], m=gc.NEGATIVE_ZEROS, nx=nx, ny=ny, z_lo=lo, z_hi=hi, reach=0, keep_unknown=1)
    want, got = assert_host_equals_twin(drivers, c)
    inside = [i for i, r in enumerate(rows) if r[1]]
    assert got["z_bits"][inside].tobytes() == c["points"][inside, 2].tobytes()
    with np.errstate(all="ignore"):
        fx, fy = (c["points"][:, 0] - F(0)) / F(1), (c["points"][:, 1] - F(0)) / F(1)
    assert np.signbit(fx[8]) and fx[8] == 0 and np.signbit(fy[9]) and fy[9] == 0           # -0.0 reaches the comparison with 0
    assert np.signbit(np.asarray(gc.NEGATIVE_ZEROS)).sum() == 9
    for i, (xyz, expect) in enumerate(rows):
        if expect is None:
            assert want["cell"][i] == -1 and want["labels"][i] == OUTSIDE, xyz
        else:
            cx, cy, seed = expect
            assert want["cell"][i] == cy * nx + cx, xyz
            if (cx, cy) not in ((0, 0), (5, 7)):
                assert want["cellmin"][cy, cx] == (key(xyz[2]) if seed else EMPTY), xyz
                assert want["labels"][i] == (GROUND if seed else UNKNOWN), xyz
    n_unknown = sum(1 for _, e in rows if e and not e[2])
    assert want["header"]["n_kept"][0] == n_unknown == 4 and (want["out"][:4, 3].view(np.uint32) == NAN_WORD).all()
    assert want["out"][:4, :3].tobytes() == c["points"][[20, 23, 25, 26]].tobytes() and (want["out"][4:].view(np.uint32) == NAN_WORD).all()
    # a cell size that is no power of two: the divide decides the column
    for cell, x_min in ((0.3, -7.0), (0.1, 0.05), (3.0, 1e6)):
        xs = (x_min + cell * np.arange(0, 41)).astype(np.float32)
        pts = np.stack([np.concatenate([xs, np.nextafter(xs, F(-1e9)), np.nextafter(xs, F(1e9))]), np.full(123, F(x_min) + F(cell) * F(0.5)),
                        np.zeros(123)], axis=1)
        want, _ = assert_host_equals_twin(drivers, gc.case(f"cell{cell}", pts, x_min=x_min, y_min=x_min, cell=cell, nx=40, ny=2))
        assert (want["cell"] == -1).sum() >= 1 and len(np.unique(want["cell"])) >= 35


def test_label_thresholds_one_ulp_apart(pkg, drivers):
    """One cell whose only seed is 0.25 (z_hi = 0.25), reach 0, band 0.0625, max_height 0.5: heights on 0.3125 and 0.75 and one ulp
    on either side of each; then the same with a band and a height whose sums with g round."""
    g = F(0.25)
    for band, height in ((F(0.0625), F(0.5)), (F(0.1), F(0.7))):
        t1, t2 = g + band, g + height
        zs = [g, ulp(t1, 0), t1, ulp(t1, 9), ulp(t2, 0), t2, ulp(t2, 9), F(-5.0)]
        c = gc.case("thresholds", gc.place([(1, 1, z) for z in zs]), nx=3, ny=3, z_lo=0.25, z_hi=0.25, band=band, max_height=height, reach=0)
        want, got = assert_host_equals_twin(drivers, c)
        assert want["labels"].tolist() == [GROUND, GROUND, GROUND, OBJECT, OBJECT, OBJECT, ABOVE, GROUND]
        assert want["cellmin"][1, 1] == key(g) == want["ground"][1, 1] and want["header"]["n_cells_seeded"][0] == 1
        assert want["header"]["n_label"][0].tolist() == [0, 0, 4, 3, 1] and want["header"]["n_kept"][0] == 3
        assert want["out"][:3, 2].tolist() == zs[3:6] and want["out"][:3, 3].tolist() == [z - g for z in zs[3:6]]
        assert got["h_bits"].view(np.float32).tolist() == [z - g for z in zs]


def test_negative_zero_orders_below_positive_zero(pkg, drivers):
    """-0.0 and +0.0 as two seeds of one cell (through the identity whose zeros are negative, which keeps the sign of a zero height): the minimum is -0.0 (key 0x7fffffff). The envelope's term adds (float)0 * rise to it,
    so g is +0.0 there, as the header states."""
    c = gc.case("zeros", gc.place([(0, 0, 0.0), (0, 0, -0.0), (1, 0, 0.0), (2, 0, -0.0), (2, 0, 0.0)]), m=gc.NEGATIVE_ZEROS, nx=3, ny=1, reach=0)
    want, _ = assert_host_equals_twin(drivers, c)
    assert want["cellmin"][0].tolist() == [0x7fffffff, 0x80000000, 0x7fffffff]
    assert want["ground"][0].tolist() == [0x80000000] * 3 and (want["labels"] == GROUND).all()
    assert key(-0.0) < key(0.0) < key(1e-45) and key(-1e-45) < key(-0.0) and key(-3e38) < key(-1.0) < key(3e38) < EMPTY


@pytest.mark.parametrize("reach", [0, 1, 2, 3, 4])
def test_envelope_at_every_corner_and_edge(pkg, drivers, reach):
    """Nine seeds -- the corners, the middle of every side, the centre of an 11 x 9 grid -- and a probe in every cell; rise 0 (a
    plain minimum filter), 0.125 (exact products) and 0.1 (3 * 0.1f rounds). g of every cell against a scalar loop over the seeds."""
    assert np.float64(F(3) * F(0.1)) != np.float64(F(0.1)) * 3                                 # the product with k = 3 rounds
    for rise in (0.0, 0.125, 0.1):
        c, seeds = gc.envelope_case(reach, rise)
        want, got = assert_host_equals_twin(drivers, c)
        nx, ny = c["params"]["nx"], c["params"]["ny"]
        assert want["header"]["n_cells_seeded"][0] == 9 and want["header"]["n_label"][0][OUTSIDE] == 0
        n_unknown = 0
        for cy in range(ny):
            for cx in range(nx):
                terms = [F(F(z) + F(max(abs(sx - cx), abs(sy - cy))) * F(rise)) for sx, sy, z in seeds if max(abs(sx - cx), abs(sy - cy)) <= reach]
                probe = 9 + cy * nx + cx
                if terms:
                    assert want["ground"][cy, cx] == key(min(terms)), (reach, rise, cx, cy)
                    assert got["h_bits"][probe] == (F(4.0) - min(terms)).view(np.uint32)
                else:
                    n_unknown += 1
                    assert want["ground"][cy, cx] == EMPTY and want["labels"][probe] == UNKNOWN and got["h_bits"][probe] == NAN_WORD
        assert n_unknown == want["header"]["n_label"][0][UNKNOWN] == max(0, nx * ny - {0: 9, 1: 49, 2: 99}.get(reach, 99))
        if reach == 0:
            assert (want["ground"] == want["cellmin"]).all()


def test_host_equals_the_twin_through_a_tilted_mount(pkg, drivers):
    """A LiDAR pitched by 4 degrees and rolled by -2.5, 1.1 m above the road, no element of the extrinsic zero; cells of 0.3 m off
    the origin. Every label occurs."""
    a, b = np.deg2rad(4.0), np.deg2rad(-2.5)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    rz = np.array([[np.cos(0.01), -np.sin(0.01), 0], [np.sin(0.01), np.cos(0.01), 0], [0, 0, 1]])
    r = rz @ rx @ ry
    level = gc.random_cloud(41, 6000, 16, 12) * np.array([0.3, 0.3, 1.0], dtype=np.float32) + np.array([2.0, -1.8, 0.0], dtype=np.float32)
    t = np.array([0.21, -0.07, 1.1])
    with np.errstate(all="ignore"):
        pts = ((level.astype(np.float64) - t) @ r).astype(np.float32)                    # the sweep in the LiDAR frame: R^T (p - t)
    m = np.concatenate([r, t[:, None]], axis=1).reshape(-1).tolist()
    assert all(v != 0 for v in m)
    want, _ = assert_host_equals_twin(drivers, gc.case("tilted", pts, m=m, x_min=2.0, y_min=-1.8, cell=0.3, reach=2))
    assert (want["header"]["n_label"][0] >= [200, 0, 2500, 900, 100]).all() and want["header"]["n_cells_seeded"][0] == 16 * 12


# ---------------------------------------------------------------- the constructed cases contain what their names say
def test_cloud_size_and_kept_pattern_cases(pkg, drivers):
    cases = gc.cloud_size_cases()
    assert tuple(len(c["points"]) for c in cases) == (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 70001)
    for c in cases:
        want, _ = assert_host_equals_twin(drivers, c)
        n, hdr = len(c["points"]), want["header"][0]
        assert hdr["n_points"] == n == hdr["n_label"].sum() and want["out"].shape == (n, 4)
        kept = (want["labels"] == OBJECT) | ((want["labels"] == UNKNOWN) & (c["params"]["keep_unknown"] != 0))
        assert hdr["n_kept"] == kept.sum() and want["out"][:hdr["n_kept"], :3].tobytes() == c["points"][kept].tobytes()
        assert (want["out"][hdr["n_kept"]:].view(np.uint32) == NAN_WORD).all()
        if n > 1000:
            assert (hdr["n_label"][[OUTSIDE, GROUND, OBJECT, ABOVE]] > 5).all() and 0 < hdr["n_kept"] < n
    empty = twin(cases[0])
    assert not empty["header"].view(np.uint8).any() and (empty["ground"] == EMPTY).all()
    got = {c["name"]: twin(c) for c in gc.kept_pattern_cases()}
    n = 3 * gc.POINT_BLOCK + 100
    assert got["all_kept"]["header"]["n_kept"][0] == n and got["all_kept"]["header"]["n_label"][0][UNKNOWN] == n
    assert (got["all_kept"]["out"][:, 3].view(np.uint32) == NAN_WORD).all() and got["none_kept"]["header"]["n_kept"][0] == 0
    assert (got["none_kept"]["out"].view(np.uint32) == NAN_WORD).all()
    assert got["alternating"]["labels"].tolist() == [GROUND, OBJECT] * (n // 2)
    assert (got["alternating"]["out"][:n // 2, 3] == 0.25).all()
    last = got["last_workgroup"]["labels"]
    assert (last[:n - 50] == GROUND).all() and (last[n - 50:] == OBJECT).all() and n - 50 > 3 * gc.POINT_BLOCK


def test_atomic_target_cases(pkg, drivers):
    c = gc.one_cell_case()
    want, _ = assert_host_equals_twin(drivers, c)
    assert (want["cell"] == 4).all() and want["header"]["n_cells_seeded"][0] == 1
    assert want["cellmin"][1, 1] == key(c["points"][:, 2].min()) and want["header"]["n_label"][0][OBJECT] == 1000
    c = gc.distinct_cells_case()
    want, _ = assert_host_equals_twin(drivers, c)
    assert want["cell"].tolist() == list(range(4096)) and want["header"]["n_cells_seeded"][0] == 4096
    assert (want["cellmin"].reshape(-1) == [key(z) for z in c["points"][:, 2]]).all()
    c, runs = gc.shared_lanes_case()
    want, _ = assert_host_equals_twin(drivers, c)
    assert len(runs) == 3 * (32 + 22 + 1) == want["header"]["n_cells_seeded"][0]
    lengths = np.bincount(want["cell"])
    assert sorted(set(lengths.tolist())) == [1, 2, 3, 64]                                 # 64 = 21 * 3 + 1
    for cell, low in runs:
        assert want["cellmin"].reshape(-1)[cell] == key(low)


def test_grid_cases(pkg, drivers):
    cases = gc.grid_cases()
    assert sorted(set((c["params"]["nx"], c["params"]["ny"]) for c in cases)) == sorted(gc.THIN_GRIDS + gc.TILE_GRIDS)
    assert sorted(set(c["params"]["reach"] for c in cases)) == [0, 4] and sorted(set(c["params"]["keep_unknown"] for c in cases)) == [0, 1]
    n_object = 0
    for c in cases:
        want, _ = assert_host_equals_twin(drivers, c)
        assert want["header"]["n_cells_seeded"][0] >= 1
        n_object += want["header"]["n_label"][0][OBJECT]
    assert n_object > 1000
    for reach in (0, 4):
        c = gc.corners_case(reach)
        want, _ = assert_host_equals_twin(drivers, c)
        last = gc.MAX_SIDE - 1
        assert want["header"]["n_cells_seeded"][0] == 4 and (want["ground"] != EMPTY).sum() == 4 * (reach + 1) ** 2
        assert [want["cellmin"][y, x] != EMPTY for y, x in ((0, 0), (0, last), (last, 0), (last, last))] == [True] * 4
        assert want["labels"].tolist() == [GROUND, OBJECT, GROUND if reach else UNKNOWN] * 4 + [UNKNOWN] * 5
        assert want["header"]["n_kept"][0] == (9 if reach else 13)


def test_labels_and_grids_do_not_depend_on_the_order_of_the_cloud(pkg):
    c = gc.random_case(9, 5000, reach=2)
    want = twin(c)
    order = np.random.RandomState(1).permutation(5000)
    got = twin(dict(c, points=c["points"][order]))
    assert got["labels"].tobytes() == want["labels"][order].tobytes()
    for name in ("cellmin", "ground", "header"):
        assert got[name].tobytes() == want[name].tobytes()


# ---------------------------------------------------------------- the scene that justifies the stage
def scene_results(s, cloud):
    from unina_yolo_dla_amd import localize
    return localize.locate_lidar_numpy(s["dets"], s["count"], cloud, s["to_cam"], s["cam"], s["width"], s["height"], s["lidar_params"])


def test_a_cone_on_a_road_is_located_on_the_road_without_the_filter_and_on_the_cone_with_it(pkg):
    """A level road, a ring LiDAR 0.8 m above it, a 0.325 m cone 15 m ahead: 16 returns from the cone, 29 from the road seen past its
    flanks inside the record's shrunk box. The lower median of the raw cloud is a road return 4.8 m behind the cone; after
    ground_numpy it is a cone return. Every cone return is OBJECT, every road return GROUND."""
    s = gc.cone_scene()
    g = twin(s)
    assert s["is_cone"].sum() == 16 and s["is_road"].sum() > 20000 and (s["is_cone"] ^ s["is_road"]).all()
    assert (g["labels"][s["is_cone"]] == OBJECT).all() and (g["labels"][s["is_road"]] == GROUND).all()
    assert g["header"]["n_kept"][0] == 16
    raw, filtered = scene_results(s, s["points"]), scene_results(s, g["out"])
    gc.assert_scene(s, raw, filtered, g["out"])
    assert raw["n_samples"][0] == 45 and filtered["n_samples"][0] == 16 and 19.0 < raw["z"][0] < 20.5
    assert (raw["u"][0], raw["v"][0]) == (filtered["u"][0], filtered["v"][0])


# ---------------------------------------------------------------- the entry points' argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the checks
    would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    h = C.c_void_p()
    for device, points in ((-1, 1000), (0, 0), (0, -1), (0, (1 << 22) + 1)):
        assert L.unina_ground_create(device, points, C.byref(h)) == 4 and not h.value
    assert L.unina_ground_create(0, 1000, None) == 4
    assert L.unina_ground_create(0, 1 << 22, C.byref(h)) == 0 and h.value                   # host only: no device is needed
    L.unina_ground_destroy(h)
    L.unina_ground_destroy(None)
    assert L.unina_ground_create(0, clouds.MAX_POINTS, C.byref(h)) == 0
    four = [C.byref(C.c_void_p()) for _ in range(4)]
    assert L.unina_ground_buffers(h, *four) == 5 and L.unina_ground_buffers(None, *four) == 4   # UNINA_ERR_STATE: no call yet
    OUT = 0x50000

    def invoke(f, mm, handle=h, out=OUT, cloud=True, ext=True, par=True):
        ss, pp = engine.Cloud(**f["cloud"]), engine.GroundParams(**f["par"])
        return L.unina_ground_filter_async(handle, C.byref(ss) if cloud else None, C.byref(mm) if ext else None, C.byref(pp) if par else None,
                                           out, None)

    call = clouds.caller(invoke, gc.LIDAR_TO_LEVEL, par=gc.params())
    bad = [dict(handle=None), dict(out=None), dict(cloud=False), dict(ext=False), dict(par=False), dict(points=None),
           dict(out=OUT + 8), dict(out=OUT + 4), *clouds.bad_cloud_args(gc.LIDAR_TO_LEVEL),
           *[{k: v} for k in ("x_min", "y_min", "z_lo", "z_hi", "rise", "band", "max_height") for v in (nan, inf, -inf)],
           *[dict(cell=v) for v in (0.0, -1.0, nan, inf)],
           *[{k: v} for k in ("nx", "ny") for v in (0, -1, 1025)],
           dict(z_lo=0.5, z_hi=0.25), dict(rise=-0.125), dict(band=-0.01), dict(band=0.25, max_height=0.125), dict(reach=-1), dict(reach=5),
           # d_out inside, over the start of, and over the end of the 500 * 16 bytes of the cloud
           dict(out=0x30010), dict(out=0x30000 - 7984), dict(out=0x30000 + 7984), dict(points=0x4ff00, stride=48), dict(points=OUT)]
    for kw in bad:
        assert call(**kw) == 4, kw
    import torch
    if not torch.cuda.is_available():
        # good calls reach HIP, which has no device here: the checks above sit in front of it
        assert call() == 3 and call(n_points=0, points=None) == 3 and call(n_points=1000, stride=12) == 3
        assert call(out=0x30000 + 8016) == 3 and call(out=0x30000 - 8000) == 3              # the output beside the cloud
        assert call(nx=1024, ny=1, reach=4, rise=0.0, band=0.0, max_height=0.0, z_lo=0.0, z_hi=0.0, keep_unknown=7) == 3
        assert L.unina_ground_buffers(h, *four) == 5                                        # still no workspace
    L.unina_ground_destroy(h)


def test_twin_refuses_malformed_input(pkg):
    from unina_yolo_dla_amd import ground
    pts = np.zeros((4, 3), dtype=np.float32)
    for bad in (dict(points=pts.astype(np.float64)), dict(points=pts[:, :2]), dict(m=gc.IDENTITY[:11]), dict(nx=0), dict(ny=1025), dict(cell=0.0),
                dict(reach=5), dict(z_lo=2.0), dict(band=1.0), dict(rise=-1.0), dict(m=(np.inf,) * 12)):
        a = dict(points=pts, m=gc.IDENTITY)
        a.update({k: v for k, v in bad.items() if k in a})
        with pytest.raises(ValueError):
            ground.ground_numpy(a["points"], a["m"], gc.params(**{k: v for k, v in bad.items() if k not in a}))


def test_records_are_plain_c_of_the_stated_sizes(pkg, tmp_path):
    from unina_yolo_dla_amd import engine
    assert engine.GROUND_HEADER_DTYPE.itemsize == 32 and C.sizeof(engine.GroundParams) == 48
    assert [engine.GROUND_HEADER_DTYPE.fields[n][1] for n in ("n_points", "n_kept", "n_label", "n_cells_seeded")] == [0, 4, 8, 28]
    assert (engine.GROUND_MAX_SIDE, engine.GROUND_MAX_REACH) == (1024, 4)
    hostprog.assert_header_is_c99()
    hostprog.compile_c99(tmp_path, 'typedef char header32[(sizeof(unina_ground_header) == 32) ? 1 : -1];\n'
                                   'typedef char seeded28[(offsetof(unina_ground_header, n_cells_seeded) == 28) ? 1 : -1];\n'
                                   'typedef char par48[(sizeof(unina_ground_params) == 48) ? 1 : -1];\n'
                                   'typedef char zlo20[(offsetof(unina_ground_params, z_lo) == 20) ? 1 : -1];\n'
                                   'typedef char reach40[(offsetof(unina_ground_params, reach) == 40) ? 1 : -1];\n'
                                   'typedef char lim[(UNINA_GROUND_MAX_SIDE == 1024 && UNINA_GROUND_MAX_REACH == 4) ? 1 : -1];\n'
                                   'int use(unina_ground_t *g, unina_lidar_t *l, const GpuDetection *d, const int *n, const void *sweep,\n'
                                   '        void *filtered, unina_cone3d *o) {\n'
                                   '  unina_cloud c = {131072, 16, 0}, kept = {131072, 16, 0};\n'
                                   '  const float level[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.8f};\n'
                                   '  const float m[12] = {0, -1, 0, 0, 0, 0, -1, 0.3f, 1, 0, 0, -0.1f};\n'
                                   '  unina_ground_params gp = {0.0f, -32.0f, 0.5f, 128, 128, -0.3f, 0.3f, 0.05f, 0.03f, 0.6f, 2, 0};\n'
                                   '  unina_pinhole k = {1400.0f, 1400.0f, 959.5f, 539.5f};\n'
                                   '  unina_lidar_params p = {1.0f, 1.0f, 0.5f, 0.5f, 40.0f, 3};\n'
                                   '  const uint8_t *labels;\n  const uint32_t *cellmin, *ground;\n  const unina_ground_header *header;\n'
                                   '  c.points = sweep;\n  kept.points = filtered;\n'
                                   '  if (unina_ground_filter_async(g, &c, level, &gp, filtered, 0)) return 1;\n'
                                   '  if (unina_locate_lidar_async(l, d, n, &kept, m, &k, 1920, 1080, &p, o, 0)) return 1;\n'
                                   '  return unina_ground_buffers(g, &labels, &cellmin, &ground, &header);\n}\n')
