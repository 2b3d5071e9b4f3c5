"""unina_locate_async without a GPU: localize.locate_numpy (the definition) against an independent brute-force restatement,
csrc/locate_window.h compiled for the host (tests/locate_window_host.cpp, also under -fsanitize=address,undefined as the
stand-alone program it is) against the numpy twin, the argument checks of the entry point, and the record layout in C."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import hostprog
import locate_cases as lc

F = np.float32


# ---------------------------------------------------------------- the brute-force restatement
def brute_force(c):
    """The header's definition with python loops over every pixel of the map and sorted(): a pixel i covers [i, i + 1), so it
    belongs to the window iff lo < i + 1 and i <= hi -- no floor, no slicing, no numpy reductions."""
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DEPTH_F32
    p, depth, fmt = c["params"], c["depth"], c["fmt"]
    h, w = depth.shape
    sx, sy, hs = F(p["sx"]), F(p["sy"]), F(0.5) * F(p["shrink"])
    unit, lo_z, hi_z = F(c["unit"]), F(p["min_depth"]), F(p["max_depth"])
    fx, fy, cx, cy = (F(v) for v in c["cam"])
    out = np.zeros(lc.MAXD, dtype=CONE3D_DTYPE)
    n = min(max(c["count"], 0), lc.MAXD)

    def covered(centre, half, size, max_side):
        lo, hi = centre - half, centre + half
        if not (math.isfinite(lo) and math.isfinite(hi)):
            return []
        px = [i for i in range(size) if lo < F(i + 1) and F(i) <= hi]
        return px[::-(-len(px) // max_side)] if px else []

    with np.errstate(all="ignore"):
        for k in range(n):
            d = c["dets"][k]
            X1, X2, Y1, Y2 = d["x1"] * sx, d["x2"] * sx, d["y1"] * sy, d["y2"] * sy
            if not all(math.isfinite(v) for v in (X1, X2, Y1, Y2)) or X2 < X1 or Y2 < Y1:
                continue
            uc, vc = F(0.5) * (X1 + X2), F(0.5) * (Y1 + Y2)
            cols = covered(uc, hs * (X2 - X1), w, p["max_side"])
            rows = covered(vc, hs * (Y2 - Y1), h, p["max_side"])
            if not cols or not rows:
                continue
            good = []
            for v in rows:
                for u in cols:
                    raw = depth[v, u]
                    if (fmt == DEPTH_F32 and not math.isfinite(raw)) or (fmt != DEPTH_F32 and raw == 0):
                        continue
                    z = F(raw) * unit
                    if lo_z <= z <= hi_z:
                        good.append(raw)
            r = out[k]
            r["u"], r["v"], r["n_samples"], r["n_valid"] = uc, vc, len(cols) * len(rows), len(good)
            if len(good) >= max(1, p["min_valid"]):
                Z = F(sorted(good)[(len(good) - 1) // 2]) * unit
                r["x"], r["y"], r["z"], r["valid"] = ((uc - cx) * Z) / fx, ((vc - cy) * Z) / fy, Z, 1
    return out


def twin(c):
    from unina_yolo_dla_amd import localize
    return localize.locate_numpy(c["dets"], c["count"], c["depth"], c["fmt"], c["unit"], c["cam"], c["params"])


@pytest.mark.parametrize("fmt", lc.FORMATS)
def test_twin_equals_brute_force_on_random_boxes(pkg, fmt):
    c = lc.random_case(fmt, n=300)
    got, want = twin(c), brute_force(c)
    assert got.tobytes() == want.tobytes()
    v = got[:300]
    assert (v["valid"] == 1).sum() > 150 and (v["n_samples"] == 0).sum() > 5            # located, and off the map
    assert (v["n_valid"] < v["n_samples"]).sum() > 100                                   # holes were met
    assert (v["n_samples"] > 64).sum() >= 5 and v["n_samples"].max() <= 16 * 16          # strided windows too
    assert not got[300:].view(np.uint8).any()


@pytest.mark.parametrize("fmt", lc.FORMATS)
def test_twin_equals_brute_force_on_the_edge_cases(pkg, fmt):
    seen = {}
    for c in lc.edge_cases(fmt):
        got, want = twin(c), brute_force(c)
        assert got.tobytes() == want.tobytes(), c["name"]
        seen[c["name"]] = got
    # the cases are what their names say
    assert not seen["count0"].view(np.uint8).any()
    assert seen["count1"]["n_samples"][:2].tolist() == [9, 0]
    assert (seen["count1024_3x3"]["n_samples"] == 9).all() and seen["count5000_clamped"].tobytes() == seen["count1024_3x3"].tobytes()
    assert not seen["count_negative"].view(np.uint8).any()
    assert not seen["outside"].view(np.uint8).any()
    assert seen["clipped_edges"]["n_samples"][:5].tolist() == [11 * 21, 12 * 21, 21 * 13, 21 * 11, 49 * 61][:5]
    assert seen["degenerate_x2_eq_x1"]["n_samples"][:4].tolist() == [21, 21, 19, 1]
    assert seen["inverted"]["n_samples"][:3].tolist()[:2] == [0, 0] and seen["inverted"]["n_samples"][2] > 0
    assert seen["non_finite_box"]["n_samples"][:5].tolist() == [0] * 5 and seen["non_finite_box"]["n_samples"][5] > 0
    assert seen["one_sample"]["n_samples"][0] == 1
    assert [seen[k]["n_samples"][0] for k in ("samples63", "samples64", "samples65")] == [63, 64, 65]
    assert seen["stride2_one_axis"]["n_samples"][:2].tolist() == [7 * 5, 5 * 7]
    assert seen["max_side1"]["n_samples"][:2].tolist() == [1, 1]
    assert seen["map600_256x256"]["n_samples"][0] == 65536 and seen["map600_256x256"]["valid"][0] == 1
    assert seen["map600_128x64_129x64"]["n_samples"][:3].tolist() == [8192, 8256, 91 * 91]
    assert (seen["all_holes"]["n_valid"] == 0).all() and (seen["all_holes"]["valid"] == 0).all() and seen["all_holes"]["n_samples"].max() > 50
    mv = seen["min_valid_one_above"]
    assert mv["n_valid"][0] == 3 and mv["valid"][0] == 0 and mv["z"][0] == 0 and mv["u"][0] == 42
    assert seen["min_valid_met"]["valid"][0] == 1 and seen["min_valid_met"]["z"][0] == 5
    assert seen["even_n_valid"]["n_valid"][0] == 4 and seen["even_n_valid"]["z"][0] == 5     # 3 5 | 7 9: the lower middle
    assert (seen["all_equal"]["z"][:3] == (F(12.5) if fmt == 0 else F(12500) * F(0.001))).all()
    for k in ("lowest_byte_only", "highest_byte_only", "heavy_ties"):
        assert (seen[k]["valid"][:4] == 1).all(), k


# ---------------------------------------------------------------- csrc/locate_window.h on the host
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("locate_window_host")
    return hostprog.build_pair(d, "locate_window_host.cpp"), d


def run_host(drivers, payload, n_words):
    got = hostprog.run_pair(*drivers, payload)
    assert got.size == n_words
    return got


def test_host_window_and_grid_equal_the_twin_over_a_sweep(pkg, drivers):
    """Box sizes 0 .. 300 (with fractional parts), offsets straddling every edge of the map, max_side in {1, 7, 64, 256},
    and a few hostile boxes; the program also checks every grid it forms against the map."""
    from unina_yolo_dla_amd import localize
    maps = [(97, 61), (640, 360), (1, 1)]
    sizes = list(range(0, 301, 7)) + [1, 2, 3, 63, 64, 65, 255, 256, 257, 299, 300]
    cases = []
    rng = np.random.RandomState(3)
    for mw, mh in maps:
        offsets = [-310, -300.5, -65, -1.25, -1, -0.5, 0, 0.375, 1, mw / 2, mw - 65, mw - 1.5, mw - 1, mw - 0.125, mw, mw + 0.5, mw + 7]
        for ms in (1, 7, 64, 256):
            for size in sizes:
                for off in offsets:
                    frac = rng.randint(0, 8) / 8
                    shrink = (1.0, 0.5, 0.3)[rng.randint(3)]
                    sx = (1.0, 0.5, 1.7)[rng.randint(3)]
                    # the same sweep on x and, transposed, on y (offsets scaled to the map's height)
                    cases.append((off, 5.0, off + size + frac, 5.0 + size / 3, sx, 1.0, shrink, mw, mh, ms))
                    oy = off * mh / mw
                    cases.append((3.0, oy, 3.0 + size / 2, oy + size + frac, 1.0, sx, shrink, mw, mh, ms))
    nan, inf = float("nan"), float("inf")
    for box in [(nan, 0, 1, 1), (0, 0, inf, 1), (-inf, 0, inf, 1), (0, -inf, 1, 5), (3e38, 0, 3.3e38, 1), (-3e38, 0, 3e38, 1),
                (5, 5, 4, 6), (5, 5, 6, 4), (1e9, 1e9, 2e9, 2e9), (-2e9, -2e9, -1e9, -1e9), (-1e30, -1e30, 1e30, 1e30)]:
        for sx in (1.0, 8.0):
            cases.append((*box, sx, sx, 1.0, 97, 61, 64))
    payload = struct.pack("<3i", 0x4c4f4331, 0, len(cases)) + b"".join(struct.pack("<7f3i", *c) for c in cases)
    got = run_host(drivers, payload, 12 * len(cases)).reshape(-1, 12)
    n_empty = n_strided = 0
    for c, g in zip(cases, got):
        w = localize.window_numpy(c[:4], c[4], c[5], c[6], c[7], c[8], c[9])
        if w is None:
            assert g.tolist() == [1] + [0] * 11, c
            n_empty += 1
            continue
        want = [0, w["u0"], w["u1"], w["v0"], w["v1"], w["stride_x"], w["stride_y"], w["cols"], w["rows"], w["n_samples"],
                int(np.array(w["uc"]).view(np.int32)), int(np.array(w["vc"]).view(np.int32))]
        assert g.tolist() == want, c
        n_strided += w["stride_x"] > 1 or w["stride_y"] > 1
    assert n_empty > 500 and n_strided > 500 and len(cases) - n_empty > 5000


@pytest.mark.parametrize("fmt", lc.FORMATS)
def test_host_sample_keys_equal_the_twins_validity(pkg, drivers, fmt):
    """locate_key_*: 0 for every hole, the raw bits otherwise -- against locate_numpy's own validity mask on one-pixel maps'
    worth of raw words (every u16 value; for f32 the special values, the range's edges and their neighbours, random bits)."""
    from unina_yolo_dla_amd.engine import DEPTH_F32
    unit, lo, hi = (1.0, 0.3, 40.0) if fmt == DEPTH_F32 else (0.001, 0.3, 40.0)
    if fmt == DEPTH_F32:
        special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1e-45, 1e-40, 0.3, 40.0, 3.4e38], dtype=np.float32).view(np.uint32)
        edges = np.array([0.3, 40.0], dtype=np.float32).view(np.uint32)
        raw = np.concatenate([special, edges - 1, edges + 1, np.random.RandomState(1).randint(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)])
        vals = raw.view(np.float32)
    else:
        raw = np.arange(65536, dtype=np.uint32)
        vals = raw.astype(np.uint16)
    payload = struct.pack("<3i", 0x4c4f4331, 1, len(raw)) + struct.pack("<i3f", fmt, unit, lo, hi) + raw.tobytes()
    got = run_host(drivers, payload, len(raw)).view(np.uint32)
    with np.errstate(all="ignore"):
        z = vals.astype(np.float32) * F(unit)
        ok = (z >= F(lo)) & (z <= F(hi)) & (np.isfinite(vals) if fmt == DEPTH_F32 else vals != 0)
    assert got.tobytes() == np.where(ok, raw, 0).astype(np.uint32).tobytes()
    assert 0 < ok.sum() < len(raw)


def test_host_point_equals_the_twin_over_a_sweep(pkg, drivers):
    """locate_point, the back-projection csrc/locate.hip and csrc/stereo_match.h both call, bit for bit against
    localize.point_numpy: centres on cx / cy, one ulp and a fraction of a pixel beside them and at the map's corners; Z at
    min_depth and max_depth, their neighbours, and values whose product with the centre's offset overflows to +-inf."""
    from unina_yolo_dla_amd import localize
    cam = np.array([70.0, 71.5, 48.25, 30.5], dtype=np.float32)                              # fx, fy, cx, cy
    cx, cy = cam[2], cam[3]
    us = np.array([cx, np.nextafter(cx, F(0)), np.nextafter(cx, F(1e9)), cx - F(0.5), cx + F(0.125), 0.0, 96.5, -3.75, 1e6, -1e6], dtype=np.float32)
    vs = np.array([cy, np.nextafter(cy, F(0)), np.nextafter(cy, F(1e9)), cy + F(0.5), 0.0, 60.5, 1e6], dtype=np.float32)
    lo, hi = F(0.3), F(40.0)
    zs = np.array([lo, np.nextafter(lo, F(1)), hi, np.nextafter(hi, F(0)), 1.0, 12.5, 1e-45, 1e-38, 3e32, 3.4e38], dtype=np.float32)
    uc, vc, Z = (a.reshape(-1) for a in np.meshgrid(us, vs, zs, indexing="ij"))
    payload = struct.pack("<3i", 0x4c4f4331, 2, len(Z)) + cam.tobytes() + np.stack([uc, vc, Z], axis=1).tobytes()
    got = run_host(drivers, payload, 3 * len(Z)).view(np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        want = np.stack(localize.point_numpy(uc, vc, Z, *cam), axis=1)
    assert want.dtype == np.float32 and len(Z) == 700 and not np.isnan(want).any()
    assert got.tobytes() == want.tobytes()
    assert np.isinf(want[:, 0]).sum() > 10 and np.isinf(want[:, 1]).sum() > 10                # overflowed products
    assert (want[uc == cx, 0] == 0).all() and (want[vc == cy, 1] == 0).all() and (want[:, 2] == Z).all()
    assert (want[:, 0] != 0).sum() > 500


# ---------------------------------------------------------------- the entry point's argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the
    checks would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    DETS, COUNT, PLANE, OUT = 0x10000, 0x20000, 0x30000, 0x40000

    def call(dets=DETS, count=COUNT, out=OUT, depth=True, cam=True, par=True, **kw):
        d = dict(format=0, width=97, height=61, pitch=400, plane=PLANE, unit=1.0)
        c = dict(fx=70.0, fy=70.0, cx=48.0, cy=30.0)
        p = dict(sx=1.0, sy=1.0, shrink=0.5, min_depth=0.3, max_depth=40.0, max_side=64, min_valid=1)
        for k, v in kw.items():
            next(t for t in (d, c, p) if k in t)[k] = v
        dd, cc, pp = engine.Depth(**d), engine.Pinhole(**c), engine.LocateParams(**p)
        return L.unina_locate_async(dets, count, C.byref(dd) if depth else None, C.byref(cc) if cam else None,
                                    C.byref(pp) if par else None, out, None)

    bad = [dict(dets=None), dict(count=None), dict(out=None), dict(depth=False), dict(cam=False), dict(par=False), dict(plane=None),
           dict(format=2), dict(format=-1), dict(width=0), dict(height=0), dict(width=-5), dict(height=-1),
           dict(pitch=387), dict(pitch=402), dict(format=1, pitch=193), dict(format=1, pitch=195),
           dict(plane=PLANE + 2), dict(format=1, plane=PLANE + 1), dict(out=OUT + 8),
           *[{k: v} for k in ("fx", "fy", "unit", "sx", "sy") for v in (0.0, -1.0, nan, inf)],
           *[{k: v} for k in ("cx", "cy") for v in (nan, inf, -inf)],
           dict(shrink=0.0), dict(shrink=-0.5), dict(shrink=1.0001), dict(shrink=nan),
           dict(max_side=0), dict(max_side=257), dict(max_side=-1), dict(min_valid=-1),
           dict(min_depth=0.0), dict(min_depth=-1.0), dict(min_depth=nan), dict(min_depth=40.0), dict(min_depth=50.0),
           dict(max_depth=inf), dict(max_depth=nan)]
    for kw in bad:
        assert call(**kw) == 4, kw
    import torch
    if not torch.cuda.is_available():
        assert call() == 3          # the good call reaches HIP, which has no device here: the checks above sit in front of it


def test_cone_record_is_32_bytes_and_the_header_stays_plain_c(pkg, tmp_path):
    from unina_yolo_dla_amd import engine
    assert engine.CONE3D_DTYPE.itemsize == 32
    assert [engine.CONE3D_DTYPE.fields[n][1] for n in ("x", "y", "z", "u", "v", "n_valid", "n_samples", "valid")] == list(range(0, 32, 4))
    assert C.sizeof(engine.LocateParams) == 28 and C.sizeof(engine.Pinhole) == 16
    hostprog.assert_header_is_c99()
    hostprog.compile_c99(tmp_path, 'typedef char cone32[(sizeof(unina_cone3d) == 32) ? 1 : -1];\n'
                                   'typedef char u12[(offsetof(unina_cone3d, u) == 12) ? 1 : -1];\n'
                                   'typedef char valid28[(offsetof(unina_cone3d, valid) == 28) ? 1 : -1];\n'
                                   'typedef char par28[(sizeof(unina_locate_params) == 28) ? 1 : -1];\n'
                                   'typedef char plane16[(offsetof(unina_depth, plane) == 16) ? 1 : -1];\n'
                                   'int use(const GpuDetection *d, const int *n, unina_cone3d *o) {\n'
                                   '  unina_depth z = {UNINA_DEPTH_U16, 4, 4, 8, 0, 0.001f};\n'
                                   '  unina_pinhole c = {1.0f, 1.0f, 2.0f, 2.0f};\n'
                                   '  unina_locate_params p = {1.0f, 1.0f, 0.5f, 0.3f, 40.0f, 64, 1};\n'
                                   '  return unina_locate_async(d, n, &z, &c, &p, o, 0);\n}\n')
