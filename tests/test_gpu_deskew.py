"""csrc/deskew.hip on the GPU through unina_deskew_async: every comparison is BYTE equality with deskew.deskew_numpy on
deskew.table_numpy's rows -- of the n_points entries of d_out and of the header (integer decisions, and fp32 values with a fixed
operation order: no tolerance). d_out and the header are filled with 0xFF before each call. Clouds are uploaded as points of 12,
16, 32 or 48 bytes with NaN bit patterns in every word that is not x, y, z, the time or the carried word, at bases that are 16-byte
aligned or only 4-byte aligned, so both forms of the kernel run. What each constructed case contains is asserted on the twin in
tests/test_deskew_cpu.py.

The sizes at which the kernel changes path (tests/deskew_cases.py names them beside the kernel's constants):
  points 63, 64 | 65: kWave; 255, 256 | 257: kDeskewBlock, one workgroup | two; 70 001: 274 workgroups     -- cloud_size_cases
  keys 2, 3, 64: the bisection's probes behind the table, its first probe on key 63                        -- key_time_case
  tau on a key, one ulp either side, before t_0, behind t_{K-1}: every `<=` of the segment and both clamps  -- key_time_case"""
import ctypes as C

import numpy as np
import pytest

import deskew_cases as dc
from clouds import STRIDES
from records import assert_records_equal

pytestmark = pytest.mark.gpu

MAX_POINTS = 1 << 17


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import deskew, engine
    return torch, deskew, engine


@pytest.fixture(scope="module")
def dev(env):
    return env[1].DeviceDeskewer(MAX_POINTS)


def upload(torch, c, stride=16, offset=0, time_at=None, plane_stride=1):
    """The case's cloud as a [n, stride] uint8 CUDA view `offset` bytes into its allocation, every word that is not a coordinate a
    NaN bit pattern or, from byte 12 on, a word of its own (what a carry_offset may name). time_at: the byte of each point that holds
    its time, or None for a plane of its own (every plane_stride-th word of a tensor). Returns (cloud, times, rows): `times` is what
    DeviceDeskewer.deskew_async takes, rows the uploaded words [n, stride / 4]."""
    n = len(c["points"])
    host = np.full((offset + n * stride) // 4 + 4, 0x7fc00000, dtype=np.uint32)
    rows = host[offset // 4:offset // 4 + n * stride // 4].reshape(n, stride // 4)
    rows[:, 3:] = (0xA0000000 + np.arange(n * (stride // 4 - 3), dtype=np.uint32)).reshape(n, stride // 4 - 3)
    rows[:, :3] = c["points"].view(np.uint32)
    words = c["times"].view(np.uint32)
    if time_at is not None:
        rows[:, time_at // 4] = words
    cloud = torch.from_numpy(host.view(np.uint8)).cuda()[offset:offset + n * stride].view(n, stride)
    if time_at is not None:
        return cloud, time_at, rows.copy()
    plane = np.full(max(n * plane_stride, 1), 0x7fc00000, dtype=np.uint32)
    plane[:n * plane_stride:plane_stride] = words
    t = torch.from_numpy(plane.view(np.float32 if c["fmt"] == dc.F32_S else np.int32)).cuda()
    return cloud, t[:n * plane_stride:plane_stride], rows.copy()


def run_device(dev, c, cloud, times, carry_offset=-1, stream=None):
    dev.out.fill_(0xFF)
    dev.header.fill_(0xFF)
    dev.deskew_async(cloud, times, c["poses"], c["t_sweep"], c["t_ref"], carry_offset, stream=stream, fmt=c["fmt"])
    header, out = dev.read(stream)
    return {"out": out, "header": header}


def twin(env, c, carry=None):
    table = env[1].table_numpy(c["poses"], c["t_sweep"], c["t_ref"])
    return env[1].deskew_numpy(c["points"], c["times"], c["fmt"], carry, table)


def assert_equal(got, want, name):
    for what in ("header", "out"):
        assert_records_equal(got[what], want[what], f"{name}: header {got['header']}", what)


def check(env, dev, c, stride=16, offset=0, time_at=None, carry_offset=-1, want=None):
    cloud, times, rows = upload(env[0], c, stride, offset, time_at)
    carry = None if carry_offset < 0 else rows[:, carry_offset // 4]
    got = run_device(dev, c, cloud, times, carry_offset)
    if want is None:
        want = twin(env, c, carry)
    elif carry is not None:                                   # the shared twin with this layout's carried words
        words = want["out"].view(np.uint32).copy()
        words[:, 3] = np.where(want["invalid"], dc.NAN_WORD, carry)
        want = dict(want, out=words.view(np.float32))
    assert_equal(got, want, f"{c['name']} stride {stride} base +{offset} time {time_at} carry {carry_offset}")
    return got


def test_cloud_sizes_on_the_edges_of_wave_and_workgroup(env, dev):
    """0, 1, 63, 64, 65, 255, 256, 257 and 70 001 points; strides 12, 16, 32, 48 in rotation, bases 16-byte and only 4-byte aligned,
    both formats and K = 2, 3, 64 in turn. The empty cloud leaves d_out alone and the header all-zero."""
    for k, c in enumerate(dc.cloud_size_cases()):
        stride = STRIDES[k % 4]
        got = check(env, dev, c, stride, (0, 4)[(k // 4) % 2], None if stride == 12 else (12, stride - 4)[k % 2],
                    -1 if stride == 12 else (-1, 12, stride - 4)[k % 3])
        assert got["header"]["n_points"][0] == len(c["points"]) == len(got["out"])
        assert got["header"]["n_moved"][0] == len(c["points"]) and got["header"]["n_invalid"][0] == 0
        if k == 0:
            assert (dev.out[:1].cpu().numpy() == 0xFF).all() and not got["header"].view(np.uint8).any()


def test_time_sources_formats_and_the_carried_word(env, dev):
    """The time inside the point at byte 12 and at stride - 4, and as a plane of its own; float32 seconds and uint32 nanoseconds;
    carry_offset -1, 12 and stride - 4 (the carried word may be the time itself); every stride, bases 0 and 4 bytes past a 16-byte
    boundary: only stride 16, 32 or 48 at offset 0 takes the 16-byte loads. With 12-byte points only a plane and -1 are legal."""
    for fmt in (dc.F32_S, dc.U32_NS):
        c = dc.random_case(60 + fmt, 1000, 11, fmt, t_ref=0.05)
        want = twin(env, c)
        for stride in STRIDES:
            inside = () if stride == 12 else sorted({12, stride - 4})
            for time_at in (None, *inside):
                for carry_offset in (-1, *inside):
                    for offset in (0, 4):
                        check(env, dev, c, stride, offset, time_at, carry_offset, want)


def test_a_strided_time_plane_and_a_float_tensor_cloud(env, dev):
    """The times as every third word of a wider tensor, and the cloud as a [n, 5] float32 tensor (x, y, z, intensity, time) whose
    row stride is the point stride: the time at byte 16, the intensity carried."""
    torch = env[0]
    c = dc.random_case(62, 777)
    cloud, times, _ = upload(torch, c, 32, 0, None, plane_stride=3)
    assert_equal(run_device(dev, c, cloud, times), twin(env, c), "strided plane")
    intensity = np.random.RandomState(1).uniform(0, 255, 777).astype(np.float32)
    xyzit = torch.from_numpy(np.concatenate([c["points"], intensity[:, None], c["times"][:, None]], axis=1)).cuda()
    got = run_device(dev, c, xyzit, 16, carry_offset=12)
    assert_equal(got, twin(env, c, intensity.view(np.uint32)), "float tensor")
    assert (got["out"][:, 3] == intensity).all()


def test_tau_on_every_key_and_one_ulp_either_side(env, dev):
    """K = 2, 3, 64: tau exactly on every key, one ulp below and above, before t_0 and behind t_{K-1}; n_before and n_after by value.
    Then every point of 773 in segment 37 of 63: every lane reads the same two rows."""
    for k, K in enumerate(dc.KEY_COUNTS):
        c, (n_before, n_after) = dc.key_time_case(K)
        got = check(env, dev, c, STRIDES[k], 4 * k, None if k == 1 else 12)
        h = got["header"][0]
        assert (h["n_before"], h["n_after"], h["n_invalid"], h["n_moved"]) == (n_before, n_after, 0, len(c["points"]))
    got = check(env, dev, dc.one_segment_case())
    assert got["header"]["n_before"][0] == 0 and got["header"]["n_after"][0] == 0


def test_special_values(env, dev):
    """NaN, +inf and -inf in each coordinate and in a float time: four words 0x7fc00000 each, n_invalid by value, the carried word
    dropped with them; -0.0 coordinates; uint32 times 0 and 0xffffffff."""
    c, bad = dc.special_value_case()
    for stride, offset in ((16, 0), (32, 4)):
        got = check(env, dev, c, stride, offset, None, 12)
        words = got["out"].view(np.uint32)
        assert got["header"]["n_invalid"][0] == len(bad) == 12 and (words[bad] == dc.NAN_WORD).all()
        assert got["header"]["n_moved"][0] == len(words) - 12 and not (words[np.setdiff1d(np.arange(len(words)), bad), 3] == dc.NAN_WORD).any()
    got = check(env, dev, dc.nanosecond_edge_case(), 32, 0, 28, 12)
    assert got["header"]["n_after"][0] >= 2 and got["header"]["n_invalid"][0] == 0


def test_identity_keys_move_nothing(env, dev):
    """Every finite output coordinate equals its input as a number (-0.0 may come back as +0.0) and max_shift2_bits is 0."""
    c = dc.identity_case()
    for stride, offset in ((16, 0), (12, 4)):
        got = check(env, dev, c, stride, offset)
        assert (got["out"][:, :3] == c["points"]).all() and got["header"]["max_shift2_bits"][0] == 0
        assert got["header"]["n_moved"][0] == len(c["points"])


def test_two_runs_and_a_permuted_cloud(env, dev):
    """Two runs give identical bytes; a permuted cloud gives the same header and the permuted points."""
    c = dc.random_case(63, 20000)
    want = twin(env, c)
    cloud, times, _ = upload(env[0], c, 32, 0, 28)
    a, b = run_device(dev, c, cloud, times), run_device(dev, c, cloud, times)
    assert_equal(a, want, "first run")
    assert_equal(b, want, "second run")
    order = np.random.RandomState(2).permutation(len(c["points"]))
    shuffled = dict(c, points=c["points"][order], times=c["times"][order], name="permuted")
    p = check(env, dev, shuffled, 16, 4)
    assert p["header"].tobytes() == want["header"].tobytes() and p["out"].tobytes() == want["out"][order].tobytes()
    assert want["header"]["max_shift2_bits"][0] > np.float32(1.0).view(np.uint32)          # metres of shift: the maximum is not idle


def test_a_side_stream(env, dev):
    torch = env[0]
    c = dc.random_case(64, 5000, 64)
    cloud, times, _ = upload(torch, c, 16, 0, 12)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = run_device(dev, c, cloud, times, stream=s)
    assert_equal(got, twin(env, c), "side stream")


def test_in_front_of_ground_filter_and_clusterer_with_nothing_between_the_calls(env, dev):
    """DeviceDeskewer -> DeviceGroundFilter -> DeviceClusterer on the cornering-cone scene, one stream, no synchronisation between the
    calls: the records, the count and the headers equal deskew_numpy -> ground_numpy -> cluster_numpy. The cone, smeared over metres
    in the raw sweep (no candidate at all, as tests/test_deskew_cpu.py established on the twins), is exactly one candidate."""
    torch, deskew, _ = env
    from unina_yolo_dla_amd import cluster, ground
    c = dc.cornering_cone_scene()
    n = len(c["points"])
    filt, clus = ground.DeviceGroundFilter(MAX_POINTS), cluster.DeviceClusterer(MAX_POINTS)
    try:
        cloud, times, _ = upload(torch, c, 32, 0, 16)
        for t in (dev.out, dev.header, filt.out, clus.det_buf, clus.cones):
            t.fill_(0xFF)
        moved = dev.deskew_async(cloud, times, c["poses"], c["t_sweep"], c["t_ref"], fmt=c["fmt"])
        kept = filt.filter_async(moved, c["m"], c["ground"])
        clus.cluster_async(kept, c["m"], c["cluster"])
        header, dets, cones, count = clus.read()
        d_header, d_out = dev.read()
        g_header, g_out = filt.read()
        d = twin(env, c)
        g = ground.ground_numpy(d["out"], c["m"], c["ground"])
        k = cluster.cluster_numpy(g["out"], c["m"], c["cluster"])
        assert d_out.tobytes() == d["out"].tobytes() and d_header.tobytes() == d["header"].tobytes()
        assert g_out.tobytes() == g["out"].tobytes() and g_header.tobytes() == g["header"].tobytes()
        for got, want in ((header, k["header"]), (dets, k["dets"]), (cones, k["cones"]), (count, k["count"])):
            assert got.tobytes() == want.tobytes()
        assert count[0] == 1 and abs(cones["x"][0] - dc.CONE_AT[0]) < 0.1 and abs(cones["y"][0] - dc.CONE_AT[1]) < 0.1 and cones["n_samples"][0] == 24
        raw = cluster.cluster_numpy(ground.ground_numpy(c["points"], c["m"], c["ground"])["out"], c["m"], c["cluster"])
        assert raw["count"][0] == 0 and d_header["n_moved"][0] == n
    finally:
        filt.close()
        clus.close()


def test_refusals_touch_nothing(env, dev):
    """A refused call leaves the 0xFF fill of d_out and of the header intact: the checks, the table's included, stand in front of
    the memset."""
    torch, deskew, engine = env
    c = dc.random_case(65, 500)
    cloud, times, _ = upload(torch, c, 16, 0, None)
    base, t, out, header = cloud.data_ptr(), times.data_ptr(), dev.out.data_ptr(), dev.header.data_ptr()
    good = deskew.as_poses(c["poses"])
    late = deskew.as_poses(c["poses"][::-1].copy())                                       # key times fall
    dev.out.fill_(0xFF)
    dev.header.fill_(0xFF)

    def call(points=base, stride=16, t=t, t_stride=4, fmt=dc.F32_S, carry=-1, poses=good, t_ref=0.05, out=out, header=header):
        cl, tt = engine.Cloud(500, stride, points), engine.PointTimes(t, t_stride, fmt)
        return dev.L.unina_deskew_async(C.byref(cl), C.byref(tt), carry, poses.ctypes.data, len(poses), 0.0, t_ref, out, header, None)

    for kw in (dict(t_ref=0.2), dict(poses=late), dict(poses=good[:1]), dict(out=out + 8), dict(header=header + 2), dict(carry=8), dict(carry=16),
               dict(fmt=2), dict(t_stride=6), dict(stride=10), dict(out=base), dict(out=t), dict(header=out + 16), dict(points=base + 2)):
        assert call(**kw) == 4, kw
    torch.cuda.synchronize()
    assert (dev.out[:501].cpu().numpy() == 0xFF).all() and (dev.header.cpu().numpy() == 0xFF).all()
    assert call() == 0
    header_now, _ = dev.read()
    assert header_now["n_points"][0] == 500
