"""unina_cluster_async without a GPU: csrc/cluster_cell.h compiled for the host (tests/cluster_cell_host.cpp, also under
-fsanitize=address,undefined as the stand-alone program it is) against cluster.cluster_numpy, byte for byte, on every grid edge,
on every threshold of the gate and on the constructed cases of tests/cluster_cases.py, whose content is asserted here on the twin;
the twin's components against scipy.ndimage.label; the scenes that justify the stage; the argument checks of the entry points;
the record layouts in C."""
import ctypes as C
import struct

import numpy as np
import pytest

import clouds
import cluster_cases as cc
import ground_cases as gc
import hostprog
from clouds import ulp

F = np.float32


def twin(c):
    from unina_yolo_dla_amd import cluster
    return cluster.cluster_numpy(c["points"], c["m"], c["params"])


# ---------------------------------------------------------------- csrc/cluster_cell.h on the host
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_cell_host")
    return hostprog.build_pair(d, "cluster_cell_host.cpp"), d


def host_cluster(drivers, c):
    """Both builds of the host program on one case -> what cluster_numpy returns, and the per-point keys and offsets and the sums."""
    from unina_yolo_dla_amd import cluster, engine
    pts = np.ascontiguousarray(c["points"][:, :3], dtype=np.float32)
    p = cluster.as_cluster_params(c["params"])
    payload = struct.pack("<2i", 0x434c5531, len(pts)) + struct.pack("<12f", *c["m"]) + bytes(p) + pts.tobytes()
    words = hostprog.run_pair(*drivers, payload).view(np.uint32)
    n, k = len(pts), int(words[3])
    assert len(words) == 8 + 7 * n + 12 * k + 16 * cc.MAXD + 1 + 4 * k
    at = 8
    per_point = words[at:at + 7 * n].reshape(n, 7)
    at += 7 * n
    table = words[at:at + 12 * k].view(engine.CLUSTER_DTYPE)
    at += 12 * k
    dets = words[at:at + 8 * cc.MAXD].view(engine.DET_DTYPE)
    cones = words[at + 8 * cc.MAXD:at + 16 * cc.MAXD].view(engine.CONE3D_DTYPE)
    at += 16 * cc.MAXD
    sums = words[at + 1:].reshape(k, 4).astype(np.uint64)
    return {"header": words[:8].view(engine.CLUSTER_HEADER_DTYPE), "cell": per_point[:, 0].astype(np.int32), "keys": per_point[:, 1:4],
            "q": per_point[:, 4:6].astype(np.int64), "point_component": per_point[:, 6].astype(np.int32), "components": table, "dets": dets,
            "cones": cones, "count": words[at:at + 1].astype(np.int32), "sx": sums[:, 0] + (sums[:, 1] << np.uint64(32)),
            "sy": sums[:, 2] + (sums[:, 3] << np.uint64(32))}


def assert_host_equals_twin(drivers, c):
    got, want = host_cluster(drivers, c), twin(c)
    for name in ("header", "cell", "point_component", "components", "dets", "cones", "count"):
        assert got[name].tobytes() == want[name].tobytes(), (c["name"], name)
    return want, got


def test_host_cells_and_offsets_equal_the_twin_on_every_grid_edge(pkg, drivers):
    """Through an identity whose zeros are negative and a unit grid at the origin fx = x and fy = y: each coordinate at and one ulp
    beside 0, an inner cell edge and the far edge of the grid, -0.0, NaN and infinities. The cell and the offset (int)(fx * 256) of
    every row, and byte equality with cluster_numpy."""
    nan, inf = np.nan, np.inf
    nx, ny = 100, 70
    rows = [((nan, 1, 0), None), ((1, nan, 0), None), ((1, 1, nan), None), ((inf, 1, 0), None), ((1, -inf, 0), None), ((1, 1, -inf), None),
            ((-0.0, 0.5, 0), (0, 0, 0, 128)), ((0.5, -0.0, 0), (0, 0, 128, 0)), ((0.0, 0.0, 0), (0, 0, 0, 0)),
            ((ulp(0, -1), 1, 0), None), ((1, ulp(0, -1), 0), None), ((ulp(0, 1), ulp(0, 1), 0), (0, 0, 0, 0)),
            ((5.0, 7.0, 0), (5, 7, 1280, 1792)), ((ulp(5, 0), ulp(7, 0), 0), (4, 6, 1279, 1791)), ((ulp(5, 9), ulp(7, 9), 0), (5, 7, 1280, 1792)),
            ((ulp(100, 0), ulp(70, 0), 0), (99, 69, 25599, 17919)), ((100.0, 1, 0), None), ((1, 70.0, 0), None),
            ((ulp(100, 1e9), 1, 0), None), ((1, ulp(70, 1e9), 0), None), ((99.99609375, 0.00390625, 0), (99, 0, 25599, 1)),
            ((3e38, 1, 0), None), ((-3e38, 1, 0), None)]
    c = cc.case("edges", [r[0] for r in rows], m=gc.NEGATIVE_ZEROS, nx=nx, ny=ny)
    want, got = assert_host_equals_twin(drivers, c)
    for i, (xyz, expect) in enumerate(rows):
        if expect is None:
            assert want["cell"][i] == -1 and want["point_component"][i] == -1, xyz
        else:
            cx, cy, qx, qy = expect
            assert want["cell"][i] == cy * nx + cx and tuple(got["q"][i]) == (qx, qy), xyz
    assert want["header"]["n_in_grid"][0] == sum(1 for r in rows if r[1]) == 9
    # cell (0, 0) holds four points, of which two have a -0.0: it keeps its key below +0.0. (4, 6) and (5, 7) touch at a corner
    first, second = want["components"][[0, 2]]                                           # between them: cell (99, 0)
    assert first["root"] == 0 and first["n_points"] == 4 and np.signbit(first["x_lo"]) and np.signbit(first["y_lo"])
    assert (second["root"], second["n_points"], second["n_cells"]) == (6 * nx + 4, 3, 2) and want["header"]["n_components"][0] == 4
    # a cell size that is no power of two: the divide decides the column, and the offset follows it
    for cell, x_min in ((0.3, -7.0), (0.1, 0.05), (3.0, 1e6)):
        xs = (x_min + cell * np.arange(0, 41)).astype(np.float32)
        pts = np.stack([np.concatenate([xs, np.nextafter(xs, F(-1e9)), np.nextafter(xs, F(1e9))]), np.full(123, F(x_min) + F(cell) * F(0.5)),
                        np.zeros(123)], axis=1)
        want, got = assert_host_equals_twin(drivers, cc.case(f"cell{cell}", pts, x_min=x_min, y_min=x_min, cell=cell, nx=40, ny=2))
        inside = want["cell"] >= 0
        assert (~inside).sum() >= 1 and len(np.unique(want["cell"])) >= 35 and (got["q"][inside, 0] // 256 == want["cell"][inside] % 40).all()


def test_gate_thresholds_one_ulp_apart(pkg, drivers):
    """max_width, min_height, max_height at equality and one ulp beside, min_points and max_points at equality and one beside."""
    c, cones = cc.gate_case()
    want, _ = assert_host_equals_twin(drivers, c)
    t = want["components"]
    assert len(t) == len(cones) == 14 and t["cone"].tolist() == [int(v) for v in cones]
    assert t["n_points"].tolist() == [2] * 11 + [1, 4, 5] and (t["n_cells"] == 1).all()
    w, lo, hi = F(0.5), F(0.125), F(0.5)
    assert (t["x_hi"] - t["x_lo"])[1] == w and (t["x_hi"] - t["x_lo"])[2] < w < (t["x_hi"] - t["x_lo"])[3]
    assert (t["y_hi"] - t["y_lo"])[4] == w and (t["y_hi"] - t["y_lo"])[5] < w < (t["y_hi"] - t["y_lo"])[6]
    h = t["z_hi"] - t["z_lo"]
    assert h[7] == lo and h[8] < lo and h[9] == hi and h[10] > hi
    assert want["count"][0] == sum(cones) == 8 and (want["dets"]["valid"][:8] == 1).all() and not want["dets"][8:].view(np.uint8).any()
    assert (want["dets"]["confidence"][:8] == F(0.75)).all() and (want["dets"]["class_id"][:8] == 2).all()
    assert want["cones"]["z"][:8].tolist() == [0.25] * 8 and (want["cones"]["n_valid"][:8] == t["n_points"][t["cone"] == 1]).all()


def test_sums_above_32_bits_and_the_position(pkg, drivers):
    """70 001 points in the last cell of a 1024-wide row: Sx > 2^32; x is the truncated mean offset, within 1/256 cell of the mean."""
    c = cc.wall_case()
    want, got = assert_host_equals_twin(drivers, c)
    t = want["components"]
    assert len(t) == 1 and t["n_points"][0] == 70001 and t["n_cells"][0] == 1 and t["root"][0] == 1023
    assert int(got["sx"][0]) == int(got["q"][:, 0].sum()) > 2 ** 32 and int(got["sy"][0]) == int(got["q"][:, 1].sum())
    assert t["x"][0] == F(int(got["sx"][0]) // 70001) * F(1 / 256) and abs(t["x"][0] - c["points"][:, 0].astype(np.float64).mean()) < 1 / 128


# ---------------------------------------------------------------- the components
@pytest.mark.parametrize("fill", [0.05, 0.3, 0.6])
def test_twin_partition_equals_scipy_label(pkg, fill):
    ndimage = pytest.importorskip("scipy").ndimage
    from unina_yolo_dla_amd import cluster
    for seed, shape in enumerate(((97, 131), (1, 50), (64, 64))):
        occupied = np.random.RandomState(seed).rand(*shape) < fill
        label, k = ndimage.label(occupied, structure=np.ones((3, 3)))
        root = cluster.components_numpy(occupied)
        assert ((root >= 0) == occupied).all() and len(np.unique(root[occupied])) == k
        smallest = ndimage.minimum(np.arange(occupied.size).reshape(shape), label, index=np.arange(1, k + 1)) if k else np.zeros(0)
        assert (root[occupied] == smallest[label[occupied] - 1]).all()      # same partition, and root = the smallest cell index


def test_constructed_cases_contain_what_their_names_say(pkg, drivers):
    sizes = cc.cloud_size_cases()
    assert tuple(len(c["points"]) for c in sizes) == (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
    for c in sizes + cc.grid_cases():
        want, _ = assert_host_equals_twin(drivers, c)
        hdr = want["header"][0]
        assert hdr["n_points"] == len(c["points"]) and hdr["n_components"] == len(want["components"]) <= hdr["n_cells"] <= hdr["n_in_grid"]
        assert want["components"]["n_points"].sum() == hdr["n_in_grid"] and want["components"]["n_cells"].sum() == hdr["n_cells"]
    assert all(twin(c)["header"]["n_components"][0] > 2 * cc.SLOTS for c in sizes[-3:])   # more components than LDS slots in one workgroup
    assert not twin(sizes[0])["header"].view(np.uint8).any() and twin(sizes[0])["count"][0] == 0
    assert sorted(set((c["params"]["nx"], c["params"]["ny"]) for c in cc.grid_cases())) == sorted(cc.THIN_GRIDS + cc.TILE_GRIDS)
    assert sum(twin(c)["header"]["n_components"][0] for c in cc.grid_cases()) > 300
    want, _ = assert_host_equals_twin(drivers, cc.corners_case())
    last = cc.MAX_SIDE - 1
    assert want["components"]["root"].tolist() == [0, last, last * cc.MAX_SIDE, cc.MAX_SIDE ** 2 - 1] and (want["components"]["n_points"] == 3).all()
    c, cells = cc.straddle_case()
    want, _ = assert_host_equals_twin(drivers, c)
    assert want["components"]["root"].tolist() == sorted(min(a[1] * 96 + a[0], b[1] * 96 + b[0]) for a, b in zip(cells[0::2], cells[1::2]))
    assert (want["components"]["n_cells"] == 2).all() and (want["components"]["n_points"] == 6).all()
    shapes = {c["name"]: twin(c) for c in cc.shape_cases()}
    for name, n_cells in (("serpentine32", 16 * 32 + 16), ("serpentine33", 17 * 33 + 16), ("serpentine96", 48 * 96 + 48), ("full64", 4096)):
        assert shapes[name]["header"]["n_components"][0] == 1 and shapes[name]["components"]["n_cells"][0] == n_cells, name
    assert shapes["spiral96"]["header"]["n_components"][0] == 1 and shapes["spiral96"]["components"]["n_cells"][0] > 4000
    assert shapes["checkerboard"]["header"]["n_components"][0] == 33 * 33 == shapes["checkerboard"]["header"]["n_cones"][0]
    counts = [twin(c)["header"][0] for c in cc.count_cases()]
    assert [(h["n_cones"], h["n_written"], h["n_dropped"]) for h in counts] == [(1023, 1023, 0), (1024, 1024, 0), (1025, 1024, 1), (0, 0, 0), (10, 10, 0)]
    late = twin(cc.count_cases()[4])["components"]
    assert len(late) == 2500 and np.nonzero(late["cone"])[0].min() >= 2 * cc.ROW_BLOCK


def test_table_does_not_depend_on_the_order_of_the_cloud(pkg):
    c = cc.random_case(9, 5000, max_width=3.0)
    want = twin(c)
    order = np.random.RandomState(1).permutation(5000)
    got = twin(dict(c, points=c["points"][order]))
    assert got["point_component"].tobytes() == want["point_component"][order].tobytes()
    for name in ("header", "components", "dets", "cones", "count"):
        assert got[name].tobytes() == want[name].tobytes()


# ---------------------------------------------------------------- the scenes that justify the stage
def test_the_cone_of_the_ground_scene_is_one_cone_candidate(pkg):
    """gc.cone_scene() filtered by ground_numpy, on 512 x 512 cells of 0.1 m: one component of 16 points in 2 cells, root 130709,
    x = 14.935, |y| < 0.001, 0.040 .. 0.272 m high, 0.081 x 0.156 m wide -- and it is a cone. The UNFILTERED cloud gives 25
    components: the road under the LiDAR is one of 10 200 points in 1037 cells, the rings further out are arcs of their own, and
    one component passes the gate -- the cone together with the road returns of its two cells -- with z_lo on the road."""
    from unina_yolo_dla_amd import ground
    s = gc.cone_scene()
    par = dict(x_min=0.0, y_min=-25.6, cell=0.1, nx=512, ny=512)
    kept = ground.ground_numpy(s["points"], s["m"], s["params"])["out"]
    r = twin(dict(points=kept, m=s["m"], params=par))
    assert r["header"][0].tolist() == (len(s["points"]), 16, 2, 1, 1, 1, 0, 0)
    t = r["components"][0]
    assert (t["n_points"], t["n_cells"], t["root"], t["cone"]) == (16, 2, 130709, 1)
    assert abs(t["x"] - 14.935) < 1e-3 and abs(t["y"]) < 1e-3 and abs(t["z_lo"] - 0.040) < 1e-3 and abs(t["z_hi"] - 0.272) < 1e-3
    assert abs((t["x_hi"] - t["x_lo"]) - 0.081) < 1e-3 and abs((t["y_hi"] - t["y_lo"]) - 0.156) < 1e-3
    assert r["count"][0] == 1 and abs(r["cones"]["x"][0] - 15.0) < 0.15 and abs(r["cones"]["y"][0]) < 0.05
    assert (r["point_component"][:16] == 0).all() and (r["point_component"][16:] == -1).all()          # the NaN entries are not IN_GRID
    raw = twin(dict(points=s["points"], m=s["m"], params=par))
    assert raw["header"]["n_components"][0] == 25
    road = raw["components"][np.argmax(raw["components"]["n_points"])]
    assert (road["n_points"], road["n_cells"], road["cone"]) == (10200, 1037, 0)


def test_two_rows_of_cones_pass_the_gate_a_wall_and_a_pole_do_not(pkg):
    from unina_yolo_dla_amd import ground
    s = cc.two_row_scene()
    kept = ground.ground_numpy(s["points"], s["m"], s["params"])
    assert 12 * 20 < kept["header"]["n_kept"][0] < 1200
    r = twin(dict(points=kept["out"], m=s["m"], params=s["cluster"]))
    t = r["components"]
    assert r["count"][0] == 12 == r["header"]["n_cones"][0] and len(t) > 12
    found = sorted(zip(r["cones"]["x"][:12].tolist(), r["cones"]["y"][:12].tolist()), key=lambda c: (round(c[0]), c[1]))
    for (x, y), (cx, cy) in zip(found, sorted(s["cones"])):
        assert abs(x - cx) < 0.1 and abs(y - cy) < 0.1
    others = t[t["cone"] == 0]
    wall = others[np.argmax(others["n_points"])]
    assert wall["x_hi"] - wall["x_lo"] > 1.0 and abs(wall["y"] - 6.0) < 0.1
    pole = others[(np.abs(others["x"] - 10.0) < 0.1) & (np.abs(others["y"] + 5.0) < 0.1)]
    assert len(pole) == 1 and pole["z_hi"][0] - pole["z_lo"][0] > 0.45 and pole["x_hi"][0] - pole["x_lo"][0] < 0.4


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
        assert L.unina_cluster_create(device, points, C.byref(h)) == 4 and not h.value
    assert L.unina_cluster_create(0, 1000, None) == 4
    assert L.unina_cluster_create(0, 1 << 22, C.byref(h)) == 0 and h.value                  # host only: no device is needed
    L.unina_cluster_destroy(h)
    L.unina_cluster_destroy(None)
    assert L.unina_cluster_create(0, clouds.MAX_POINTS, C.byref(h)) == 0
    three = [C.byref(C.c_void_p()) for _ in range(3)]
    assert L.unina_cluster_buffers(h, *three) == 5 and L.unina_cluster_buffers(None, *three) == 4   # UNINA_ERR_STATE: no call yet
    DETS, COUNT, CONES = 0x50000, 0x60000, 0x70000

    def invoke(f, mm, handle=h, dets=DETS, count=COUNT, cones=CONES, cloud=True, ext=True, par=True):
        ss, pp = engine.Cloud(**f["cloud"]), engine.ClusterParams(**f["par"])
        return L.unina_cluster_async(handle, C.byref(ss) if cloud else None, C.byref(mm) if ext else None, C.byref(pp) if par else None,
                                     dets, count, cones, None)

    call = clouds.caller(invoke, gc.LIDAR_TO_LEVEL, par=cc.params())
    end = clouds.POINTS + 500 * 16                                                         # the cloud is 0x30004 .. 0x31f44
    bad = [dict(handle=None), dict(dets=None), dict(count=None), dict(cones=None), dict(cloud=False), dict(ext=False), dict(par=False),
           dict(points=None), dict(dets=DETS + 8), dict(dets=DETS + 4), dict(cones=CONES + 8), dict(count=COUNT + 2), dict(count=COUNT + 1),
           *clouds.bad_cloud_args(gc.LIDAR_TO_LEVEL),
           *[{k: v} for k in ("x_min", "y_min", "min_height", "max_height", "max_width") for v in (nan, inf, -inf)],
           *[dict(cell=v) for v in (0.0, -1.0, nan, inf)],
           *[{k: v} for k in ("nx", "ny") for v in (0, -1, 1025)],
           dict(min_points=0), dict(min_points=-3), dict(min_points=5, max_points=4), dict(min_height=-0.125), dict(min_height=0.5, max_height=0.25),
           dict(max_width=-0.5), dict(confidence=nan),
           # an output inside, over the start of, and over the end of the cloud
           dict(dets=0x30010), dict(cones=0x30010), dict(count=0x30010), dict(dets=0x30000 - 32768 + 16), dict(cones=0x30000 - 32768 + 16),
           dict(dets=(end - 1) & ~15), dict(count=end - 4), dict(count=clouds.POINTS)]
    for kw in bad:
        assert call(**kw) == 4, kw
    import torch
    if not torch.cuda.is_available():
        # good calls reach HIP, which has no device here: the checks above sit in front of it
        assert call() == 3 and call(n_points=0, points=None) == 3 and call(n_points=1000, stride=12) == 3
        assert call(count=end) == 3 and call(count=clouds.POINTS - 4) == 3 and call(dets=0x30000 - 32768) == 3   # the outputs beside the cloud
        assert call(nx=1024, ny=1, min_points=1, max_points=1, min_height=0.0, max_height=0.0, max_width=0.0, confidence=inf, class_id=-7) == 3
        assert L.unina_cluster_buffers(h, *three) == 5                                      # still no workspace
    L.unina_cluster_destroy(h)


def test_twin_refuses_malformed_input(pkg):
    from unina_yolo_dla_amd import cluster
    pts = np.zeros((4, 3), dtype=np.float32)
    for bad in (dict(points=pts.astype(np.float64)), dict(points=pts[:, :2]), dict(m=gc.IDENTITY[:11]), dict(nx=0), dict(ny=1025), dict(cell=0.0),
                dict(min_points=0), dict(max_points=0), dict(min_height=-1.0), dict(max_height=-1.0), dict(max_width=-1.0),
                dict(confidence=float("nan")), dict(m=(np.inf,) * 12)):
        a = dict(points=pts, m=gc.IDENTITY)
        a.update({k: v for k, v in bad.items() if k in a})
        with pytest.raises(ValueError):
            cluster.cluster_numpy(a["points"], a["m"], cc.params(**{k: v for k, v in bad.items() if k not in a}))


def test_records_are_plain_c_of_the_stated_sizes(pkg, tmp_path):
    from unina_yolo_dla_amd import engine
    assert engine.CLUSTER_DTYPE.itemsize == 48 and engine.CLUSTER_HEADER_DTYPE.itemsize == 32 and C.sizeof(engine.ClusterParams) == 48
    assert [engine.CLUSTER_DTYPE.fields[n][1] for n in ("x", "z_lo", "x_lo", "n_points", "root", "cone")] == [0, 8, 16, 32, 40, 44]
    assert [engine.CLUSTER_HEADER_DTYPE.fields[n][1] for n in ("n_points", "n_components", "n_dropped")] == [0, 12, 24]
    hostprog.assert_header_is_c99()
    hostprog.compile_c99(tmp_path, 'typedef char rec48[(sizeof(unina_cluster) == 48) ? 1 : -1];\n'
                                   'typedef char root40[(offsetof(unina_cluster, root) == 40) ? 1 : -1];\n'
                                   'typedef char header32[(sizeof(unina_cluster_header) == 32) ? 1 : -1];\n'
                                   'typedef char dropped24[(offsetof(unina_cluster_header, n_dropped) == 24) ? 1 : -1];\n'
                                   'typedef char par48[(sizeof(unina_cluster_params) == 48) ? 1 : -1];\n'
                                   'typedef char height28[(offsetof(unina_cluster_params, min_height) == 28) ? 1 : -1];\n'
                                   'typedef char class44[(offsetof(unina_cluster_params, class_id) == 44) ? 1 : -1];\n'
                                   'int use(unina_ground_t *g, unina_cluster_t *c, unina_tracker_t *t, const void *sweep, void *filtered,\n'
                                   '        GpuDetection *d, int *n, unina_cone3d *o) {\n'
                                   '  unina_cloud raw = {131072, 16, 0}, kept = {131072, 16, 0};\n'
                                   '  const float level[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.8f};\n'
                                   '  unina_ground_params gp = {0.0f, -32.0f, 0.5f, 128, 128, -0.3f, 0.3f, 0.05f, 0.03f, 0.6f, 2, 0};\n'
                                   '  unina_cluster_params cp = {0.0f, -25.6f, 0.1f, 512, 512, 5, 300, 0.1f, 0.45f, 0.4f, 0.9f, 1};\n'
                                   '  unina_track_params tp = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, 0.5f, 0.5f, 0.0f, 1, 3, 5};\n'
                                   '  const unina_cluster *table;\n  const int *component;\n  const unina_cluster_header *header;\n'
                                   '  raw.points = sweep;\n  kept.points = filtered;\n'
                                   '  if (unina_ground_filter_async(g, &raw, level, &gp, filtered, 0)) return 1;\n'
                                   '  if (unina_cluster_async(c, &kept, level, &cp, d, n, o, 0)) return 1;\n'
                                   '  if (unina_track_update_async(t, d, n, o, &tp, 0, 0)) return 1;\n'
                                   '  return unina_cluster_buffers(c, &table, &component, &header);\n}\n')
