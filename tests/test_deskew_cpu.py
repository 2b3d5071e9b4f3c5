"""unina_deskew_async without a GPU: csrc/deskew_math.h compiled for the host (tests/deskew_math_host.cpp, also under
-fsanitize=address,undefined as the stand-alone program it is) against the numpy twins, unina_deskew_table through ctypes against
deskew.table_numpy byte for byte, the argument checks of both entry points, the layouts in C, what each constructed case of
tests/deskew_cases.py contains, and the physical checks on the twins alone: a cornering vehicle's sweep comes back to within a
millimetre of what a LiDAR standing still would have seen, and a cone smeared over metres becomes one candidate again.

Measured on the twins (seed 7, 20 000 points within +-30 m, v = 15 m/s, w = 1.5 rad/s, 0.1 s, t_ref = 0.1): the largest residual is
28.1 mm with K = 2, 0.284 mm with K = 11 and 0.0115 mm with K = 64; without de-skew the same points are off by up to 7.2 m (3.6 m for
t_ref = 0.05)."""
import ctypes as C
import struct

import numpy as np
import pytest

import clouds
import deskew_cases as dc
import hostprog

MAGIC = 0x44534b31
ERR_ARG = 4


@pytest.fixture(scope="module")
def dk(pkg):
    from unina_yolo_dla_amd import build, deskew, engine
    build.build_native()
    return deskew, engine, engine.load_library()


def twin(dk, c, carry=None, poses=None):
    table = dk[0].table_numpy(c["poses"] if poses is None else poses, c["t_sweep"], c["t_ref"])
    return dk[0].deskew_numpy(c["points"], c["times"], c["fmt"], carry, table), table


def all_cases():
    return [*dc.cloud_size_cases()[:-1], dc.random_case(9, 5000, 11, dc.U32_NS, t_ref=0.05), *[dc.key_time_case(k)[0] for k in dc.KEY_COUNTS],
            dc.one_segment_case(), dc.special_value_case()[0], dc.nanosecond_edge_case(), dc.identity_case(), dc.cornering_cone_scene()]


# ---------------------------------------------------------------- csrc/deskew_math.h on the host, plain and sanitised
def test_host_program_gives_the_twins_bytes(dk, tmp_path):
    """Per point the words of x', y', z' and of the shift and the three flags, and per table the rows, of csrc/deskew_math.h built
    by g++ equal the numpy twins'; the sanitised build agrees and reports nothing."""
    exes = hostprog.build_pair(tmp_path, "deskew_math_host.cpp")
    for c in all_cases():
        want, table = twin(dk, c)
        n = len(c["points"])
        words = np.zeros((n, 4), dtype=np.uint32)
        words[:, :3] = c["points"].view(np.uint32)
        words[:, 3] = c["times"].view(np.uint32)
        payload = struct.pack("<8i", MAGIC, 0, n, len(table), c["fmt"], 0, 0, 0) + table.tobytes() + words.tobytes()
        got = hostprog.run_pair(exes, tmp_path, payload, dtype=np.uint32).reshape(n, 8)
        ref = np.zeros((n, 8), dtype=np.uint32)
        ref[:, :3] = want["out"].view(np.uint32)[:, :3]
        ref[:, 3], ref[:, 4], ref[:, 5], ref[:, 6] = want["shift2"], want["invalid"], want["before"], want["after"]
        assert got.tobytes() == ref.tobytes(), (c["name"], np.nonzero((got != ref).any(axis=1))[0][:5])
        assert want["header"]["max_shift2_bits"][0] == (got[:, 3].max() if n else 0)
        poses = dk[0].as_poses(c["poses"])
        payload = struct.pack("<4i2d", MAGIC, 1, 0, len(poses), c["t_sweep"], c["t_ref"]) + poses.tobytes()
        got = hostprog.run_pair(exes, tmp_path, payload, dtype=np.uint32)
        assert got[0] == 0 and got[8:].tobytes() == table.tobytes(), c["name"]
    for name, poses, t_sweep, t_ref in bad_tables():                       # the refusals on the sanitised build as well
        payload = struct.pack("<4i2d", MAGIC, 1, 0, len(poses), t_sweep, t_ref) + np.ascontiguousarray(poses, dtype=np.float64).tobytes()
        got = hostprog.run_pair(exes, tmp_path, payload, dtype=np.uint32)
        assert got[0] == ERR_ARG and not got[1:].any(), name


# ---------------------------------------------------------------- the table
def table_inputs():
    """(name, poses, t_sweep, t_ref): identity keys; K = 2, 3, 64; non-unit quaternions; t_ref on a key, between keys and at both
    ends; absolute stamps near 1.7e9 s with odometry coordinates of kilometres; a vehicle that also pitches and rolls."""
    rng = np.random.RandomState(3)
    out = [("identity", dc.identity_poses(5), 0.0, 0.04)]
    for K in dc.KEY_COUNTS:
        for where, t_ref in (("first", 0.0), ("last", dc.SWEEP), ("between", 0.0371), ("on_a_key", dc.SWEEP * ((K - 1) // 2) / (K - 1))):
            out.append((f"arc{K}_{where}", dc.arc_poses(K), 0.0, t_ref))
    scaled = dc.arc_poses(7)
    scaled[:, 1:5] *= rng.uniform(0.1, 9.0, (7, 1))
    out.append(("non_unit", scaled, 0.0, 0.05))
    stamp = 1.7e9 + 0.123456789
    absolute = dc.arc_poses(11, t_sweep=stamp, origin=(41234.5, -9876.25, 12.0), heading=2.5)
    out.append(("absolute", absolute, stamp, stamp + 0.0625))
    out.append(("absolute_before_sweep", absolute, stamp + 0.02, stamp + 0.1))   # the first keys lie before the sweep's stamp
    tumble = dc.arc_poses(9)
    axis = rng.normal(size=(9, 3)) * 0.05
    tumble[:, 2:5] += axis                                                    # not unit any more: step 1 normalises
    tumble[:, 7] = np.linspace(0.0, 0.3, 9)
    out.append(("tumble", tumble, 0.0, 0.07))
    back = dc.arc_poses(5, heading=3.0)                                       # q.w changes sign along the way
    out.append(("half_turn", back, 0.0, 0.1))
    return out


def test_table_bytes_through_the_c_abi(dk):
    """unina_deskew_table, which needs no device, returns table_numpy's bytes; the rows hold what the steps promise."""
    deskew = dk[0]
    for name, poses, t_sweep, t_ref in table_inputs():
        want = deskew.table_numpy(poses, t_sweep, t_ref)
        got = deskew.table_native(poses, t_sweep, t_ref)
        assert got.tobytes() == want.tobytes(), name
        q = np.stack([want[k] for k in ("qw", "qx", "qy", "qz")], axis=1).astype(np.float64)
        assert np.allclose((q * q).sum(axis=1), 1.0, atol=1e-6) and q[0, 0] >= 0 and ((q[1:] * q[:-1]).sum(axis=1) > 0.5).all(), name
        assert (np.diff(want["t"]) > 0).all() and np.abs(np.stack([want[k] for k in ("px", "py", "pz")])).max() < 10.0, name
    ident = deskew.table_numpy(dc.identity_poses(5), 0.0, 0.04)
    assert (ident["qw"] == 1).all() and not any(ident[k].any() for k in ("qx", "qy", "qz", "px", "py", "pz"))
    # a key at t_ref is the identity, translation zero: the large coordinates cancelled in float64
    on_key = deskew.table_numpy(dc.arc_poses(11, t_sweep=1.7e9, origin=(41234.5, -9876.25, 12.0)), 1.7e9, 1.7e9 + dc.arc_poses(11)[4, 0])
    assert on_key["qw"][4] == 1 and abs(on_key["px"][4]) < 1e-9 and abs(on_key["py"][4]) < 1e-9 and on_key["pz"][4] == 0


def test_keys_given_as_q_and_as_minus_q_make_the_same_table(dk):
    for K in (2, 3, 11, dc.MAX_KEYS):
        poses = dc.arc_poses(K, heading=2.9)
        for first in (0, 1):
            flipped = poses.copy()
            flipped[first::2, 1:5] *= -1.0
            for t_ref in (0.0, 0.033, dc.SWEEP):
                want = dk[0].table_numpy(poses, 0.0, t_ref)
                assert dk[0].table_numpy(flipped, 0.0, t_ref).tobytes() == want.tobytes(), (K, first, t_ref)
                assert dk[0].table_native(flipped, 0.0, t_ref).tobytes() == want.tobytes(), (K, first, t_ref)


def bad_tables():
    """(name, poses, t_sweep, t_ref), each refused: one argument spoiled at a time from a good 5-key arc."""
    good = dc.arc_poses(5)
    nan, inf = float("nan"), float("inf")
    out = [("one_key", good[:1], 0.0, 0.0), ("sixty_five_keys", dc.arc_poses(65), 0.0, 0.05)]
    out += [(f"t_sweep_{v}", good, v, 0.05) for v in (nan, inf, -inf)] + [(f"t_ref_{v}", good, 0.0, v) for v in (nan, inf, -inf)]
    for col in range(8):
        for v in (nan, inf, -inf):
            spoiled = good.copy()
            spoiled[2, col] = v
            out.append((f"field{col}_{v}", spoiled, 0.0, 0.05))
    zero = good.copy()
    zero[3, 1:5] = 0.0
    out.append(("zero_norm", zero, 0.0, 0.05))
    same = good.copy()
    same[2, 0] = same[1, 0]
    out.append(("equal_times", same, 0.0, 0.05))
    back = good.copy()
    back[2, 0] = 0.01
    out.append(("times_fall", back, 0.0, 0.05))
    close = good.copy()
    close[:, 0] = 1.7e9 + np.arange(5) * 1e-6
    out.append(("times_equal_as_float32", close, 0.0, 1.7e9))                 # distinct doubles, one float32
    out += [("t_ref_before", good, 0.0, -1e-9), ("t_ref_after", good, 0.0, dc.SWEEP + 1e-9)]
    wide = dc.arc_poses(3, w=2.2 / 0.05)                                      # 2.2 rad (126 degrees) between two keys
    out.append(("more_than_120_degrees", wide, 0.0, 0.05))
    far = good.copy()
    far[4, 5] = 1e39
    out.append(("translation_beyond_fp32", far, 0.0, 0.05))
    return out


def test_every_bad_table_is_refused_by_the_twin_and_by_the_c_abi(dk):
    deskew, _, L = dk
    for name, poses, t_sweep, t_ref in bad_tables():
        with pytest.raises(ValueError):
            deskew.table_numpy(poses, t_sweep, t_ref)
        with pytest.raises(ValueError):
            deskew.table_native(poses, t_sweep, t_ref)
    rows = np.zeros(5, dtype=deskew.DESKEW_KEY_DTYPE)
    good = deskew.as_poses(dc.arc_poses(5))
    assert L.unina_deskew_table(None, 5, 0.0, 0.05, rows.ctypes.data) == ERR_ARG
    assert L.unina_deskew_table(good.ctypes.data, 5, 0.0, 0.05, None) == ERR_ARG
    assert L.unina_deskew_table(good.ctypes.data, 5, 0.0, 0.05, rows.ctypes.data) == 0
    # 119 degrees between two keys is still a table
    assert len(deskew.table_native(dc.arc_poses(3, w=2.07 / 0.05), 0.0, 0.05)) == 3


# ---------------------------------------------------------------- the entry point's argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(dk):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the checks
    would answer 3 (UNINA_ERR_HIP) instead. The device pointers are never dereferenced by a refused call."""
    deskew, engine, L = dk
    OUT, TIMES, HEADER = 0x50000, 0x60000, 0x70000
    good = deskew.as_poses(dc.arc_poses(5))

    def invoke(f, _m, out=OUT, header=HEADER, carry=-1, poses=good, n_keys=None, t_sweep=0.0, t_ref=0.05, cloud=True, times=True):
        ss = engine.Cloud(**f["cloud"])
        tt = engine.PointTimes(f["times"]["t"], f["times"]["t_stride"], f["times"]["format"])
        keys = None if poses is None else deskew.as_poses(poses)
        return L.unina_deskew_async(C.byref(ss) if cloud else None, C.byref(tt) if times else None, carry, None if keys is None else keys.ctypes.data,
                                    (0 if keys is None else len(keys)) if n_keys is None else n_keys, t_sweep, t_ref, out, header, None)

    from ground_cases import IDENTITY
    call = clouds.caller(invoke, IDENTITY, times=dict(t=TIMES, t_stride=4, format=dc.F32_S))
    cloud_part = [kw for kw in clouds.bad_cloud_args(IDENTITY) if "m" not in kw and kw != dict(n_points=clouds.MAX_POINTS + 1)]
    assert len(cloud_part) == 8
    bad = [dict(out=None), dict(header=None), dict(cloud=False), dict(times=False), dict(poses=None, n_keys=5), dict(points=None), dict(t=None),
           dict(n_points=(1 << 22) + 1), *cloud_part,
           dict(out=OUT + 8), dict(out=OUT + 4), dict(header=HEADER + 2), dict(header=HEADER + 1),
           dict(t=TIMES + 2), dict(t=TIMES + 1), dict(t_stride=0), dict(t_stride=-4), dict(t_stride=2), dict(t_stride=6), dict(format=2), dict(format=-1),
           # carry: below the coordinates' end, not a word, past the point; stride 12 has no room for one
           dict(carry=0), dict(carry=8), dict(carry=-2), dict(carry=-4), dict(carry=14), dict(carry=16), dict(stride=32, carry=32),
           dict(stride=32, carry=30), dict(stride=12, carry=12),
           dict(n_keys=1), dict(n_keys=0), dict(n_keys=-1), dict(poses=dc.arc_poses(65)),
           # d_out inside, over the start of, and over the end of the 500 * 16 bytes of the cloud, of the time plane, of an in-point time
           dict(out=0x30010), dict(out=0x30000 - 7984), dict(out=0x30000 + 8000), dict(points=0x4ff00, stride=48), dict(points=OUT),
           dict(out=TIMES + 1984), dict(out=TIMES - 7984), dict(t=OUT + 7996), dict(t=OUT - 1996), dict(t=OUT - 499 * 64, t_stride=64),
           dict(header=OUT + 16), dict(header=OUT + 7996), dict(header=OUT - 28)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    for name, poses, t_sweep, t_ref in bad_tables():
        assert call(poses=poses, t_sweep=t_sweep, t_ref=t_ref) == ERR_ARG, name
    import torch
    if not torch.cuda.is_available():
        # good calls reach HIP, which has no device here: the checks above sit in front of it
        assert call() == 3 and call(n_points=0, points=None, t=None) == 3
        assert call(n_points=1 << 22, points=0x10000000, t=0x20000000, header=0x30000000) == 3       # 64 MB at d_out: nothing else inside
        assert call(carry=12) == 3 and call(stride=48, carry=44) == 3 and call(stride=12) == 3
        assert call(t=clouds.POINTS + 12, t_stride=16) == 3 and call(t=clouds.POINTS + 28, t_stride=32, stride=32, format=dc.U32_NS) == 3
        assert call(out=0x30000 + 8016) == 3 and call(out=0x30000 - 8000) == 3 and call(out=TIMES + 2000) == 3 and call(out=TIMES - 8000) == 3
        assert call(header=OUT + 8000) == 3 and call(header=OUT - 32) == 3 and call(header=HEADER + 4) == 3
        assert call(poses=dc.arc_poses(2), t_ref=0.0) == 3 and call(poses=dc.arc_poses(64), t_ref=0.1) == 3


def test_layouts_in_c(tmp_path):
    """The header stays plain C99 with the new section, and its records have the sizes the kernel and the dtypes assume."""
    hostprog.assert_header_is_c99()
    hostprog.compile_c99(tmp_path, """
typedef char pose_is_64[sizeof(unina_deskew_pose) == 64 ? 1 : -1];
typedef char key_is_32[sizeof(unina_deskew_key) == 32 && offsetof(unina_deskew_key, t) == 28 ? 1 : -1];
typedef char header_is_32[sizeof(unina_deskew_header) == 32 && offsetof(unina_deskew_header, max_shift2_bits) == 20 ? 1 : -1];
typedef char times_is_16[sizeof(unina_point_times) == 16 && offsetof(unina_point_times, format) == 12 ? 1 : -1];
typedef char limits[UNINA_DESKEW_MAX_KEYS == 64 && UNINA_TIME_F32_S == 0 && UNINA_TIME_U32_NS == 1 ? 1 : -1];
int use(const unina_cloud *c, const unina_point_times *t, const unina_deskew_pose *p, void *o, unina_deskew_header *h) {
  unina_deskew_key rows[UNINA_DESKEW_MAX_KEYS];
  return unina_deskew_table(p, 2, 0.0, 0.0, rows) + unina_deskew_async(c, t, -1, p, 2, 0.0, 0.0, o, h, (hipStream_t)0);
}
""")


# ---------------------------------------------------------------- what the constructed cases contain, on the twin
def test_constructed_cases_contain_what_they_claim(dk):
    deskew = dk[0]
    for K in dc.KEY_COUNTS:
        c, (n_before, n_after) = dc.key_time_case(K)
        got, table = twin(dk, c)
        h = got["header"][0]
        assert (h["n_before"], h["n_after"], h["n_invalid"], h["n_moved"]) == (n_before, n_after, 0, len(c["points"])), K
        seg, s = got["segment"][:K], got["s"][:K]                             # tau exactly on key j
        assert seg.tolist() == [min(j, K - 2) for j in range(K)] and (s[:K - 1] == 0).all() and s[K - 1] == 1
        below = got["segment"][K:2 * K]                                       # one ulp below key j: the segment before it
        assert below.tolist() == [max(j - 1, 0) for j in range(K)] and (got["s"][K + 1:2 * K] < 1).all() and got["s"][K] == 0
        assert (got["s"][-4:] == [0, 0, 1, 1]).all()
    c = dc.one_segment_case()
    assert set(twin(dk, c)[0]["segment"].tolist()) == {37}
    c, bad = dc.special_value_case()
    got, _ = twin(dk, c, carry=np.arange(len(c["points"]), dtype=np.uint32))
    words = got["out"].view(np.uint32)
    assert np.nonzero(got["invalid"])[0].tolist() == bad and got["header"]["n_invalid"][0] == len(bad) == 12
    assert (words[bad] == dc.NAN_WORD).all() and (words[~got["invalid"], 3] == np.arange(len(words))[~got["invalid"]]).all()
    assert np.isfinite(got["out"][~got["invalid"], :3]).all() and got["header"]["n_moved"][0] == len(words) - 12
    c = dc.nanosecond_edge_case()
    got, _ = twin(dk, c)
    # 0xffffffff and 0x80000000 ns lie behind the last key; which side of a key its neighbouring nanoseconds fall is the roundings'
    assert got["header"]["n_after"][0] >= 2 and got["header"]["n_before"][0] == 0 and got["header"]["n_invalid"][0] == 0
    assert got["segment"][[0, 1, 2, 9]].tolist() == [0, 1, 0, 1] and got["after"][[1, 9]].all() and got["s"][0] == 0
    c = dc.identity_case()
    got, _ = twin(dk, c)
    assert (got["out"][:, :3] == c["points"]).all() and got["header"]["max_shift2_bits"][0] == 0 and (got["out"].view(np.uint32)[:, 3] == dc.NAN_WORD).all()
    empty, _ = twin(dk, dc.cloud_size_cases()[0])
    assert not empty["header"].view(np.uint8).any() and empty["out"].shape == (0, 4)
    for bad_call in (lambda: deskew.deskew_numpy(c["points"].astype(np.float64), c["times"], 0, None, deskew.table_numpy(c["poses"], 0.0, 0.04)),
                     lambda: deskew.deskew_numpy(c["points"], c["times"], dc.U32_NS, None, deskew.table_numpy(c["poses"], 0.0, 0.04)),
                     lambda: deskew.deskew_numpy(c["points"], c["times"][:-1], 0, None, deskew.table_numpy(c["poses"], 0.0, 0.04)),
                     lambda: deskew.deskew_numpy(c["points"], c["times"], 0, np.zeros(3, dtype=np.uint32), deskew.table_numpy(c["poses"], 0.0, 0.04))):
        with pytest.raises(ValueError):
            bad_call()


def test_any_order_of_the_cloud_gives_the_same_header_and_the_permuted_points(dk):
    c = dc.random_case(12, 3000)
    want, table = twin(dk, c)
    order = np.random.RandomState(5).permutation(3000)
    got = dk[0].deskew_numpy(c["points"][order], c["times"][order], c["fmt"], None, table)
    assert got["header"].tobytes() == want["header"].tobytes() and got["out"].tobytes() == want["out"][order].tobytes()


# ---------------------------------------------------------------- the physical checks, on the twins alone
def residuals(dk, n_keys, t_ref, seed=7, n=20000, **kw):
    """(largest |deskewed - truth|, largest |measured - truth|) in metres for n static points within +-30 m seen at uniformly random
    times of the sweep from the cornering vehicle; truth comes from the analytic float64 pose (deskew_cases.measure), not from the
    code under test."""
    rng = np.random.RandomState(seed)
    truth = rng.uniform(-30.0, 30.0, (n, 3)) * np.array([1.0, 1.0, 0.1])
    times = rng.uniform(0.0, dc.SWEEP, n).astype(np.float32)
    stamp = kw.pop("t_sweep", 0.0)
    measured = dc.measure(truth, times.astype(np.float64), t_ref, **kw).astype(np.float32)
    table = dk[0].table_numpy(dc.arc_poses(n_keys, t_sweep=stamp, **kw), stamp, stamp + t_ref)
    got = dk[0].deskew_numpy(measured, times, dc.F32_S, None, table)
    assert got["header"]["n_moved"][0] == n
    return (float(np.linalg.norm(got["out"][:, :3].astype(np.float64) - truth, axis=1).max()),
            float(np.linalg.norm(measured.astype(np.float64) - truth, axis=1).max()))


def test_a_cornering_sweep_comes_back_to_within_a_millimetre(dk):
    """v = 15 m/s, w = 1.5 rad/s, 0.1 s, 20 000 static points within +-30 m, 11 equally spaced keys of the exact motion: the residual
    stays below 1 mm for t_ref = 0.1 and 0.05, where the raw points are off by more than 1 m. Between keys the model is nlerp plus
    a linear translation, so the error falls with the square of the key spacing: from K = 2 to K = 11 the spacing falls 10 times
    and the error 100 times (asserted within a factor of two); from K = 11 to K = 64 another 6.3 times, 40 times in the error,
    of which fp32 coordinates of 30 m (ulp 1.9e-6 m, a dozen roundings) leave at least 10 times visible."""
    for t_ref in (dc.SWEEP, 0.05):
        e11, raw = residuals(dk, 11, t_ref)
        print(f"t_ref {t_ref}: K = 11 residual {e11 * 1e3:.4f} mm, raw {raw:.3f} m")
        assert e11 < 1e-3 and raw > 1.0
    e2, _ = residuals(dk, 2, dc.SWEEP)
    e64, _ = residuals(dk, 64, dc.SWEEP)
    e11, _ = residuals(dk, 11, dc.SWEEP)
    print(f"K = 2: {e2 * 1e3:.4f} mm, K = 11: {e11 * 1e3:.4f} mm, K = 64: {e64 * 1e3:.4f} mm")
    assert 50.0 < e2 / e11 < 200.0 and e64 < e11 / 10.0
    # the same vehicle far from the odometry origin, late in the day: the float64 table cancels both
    far, _ = residuals(dk, 11, dc.SWEEP, seed=8, t_sweep=1.7e9 + 0.25, origin=(41234.5, -9876.25, 0.0), heading=2.5)
    assert far < 1e-3


def test_a_smeared_cone_is_one_candidate_again(dk):
    """One cone whose 24 returns are spread over the sweep: as measured, its points lie metres apart and cluster_numpy finds no
    candidate at all (every component has too few points or is too wide for the gate); de-skewed, exactly one, where the cone
    stands."""
    from unina_yolo_dla_amd import cluster
    c = dc.cornering_cone_scene(with_road=False)
    raw = cluster.cluster_numpy(c["points"], c["m"], c["cluster"])
    assert raw["count"][0] == 0 and raw["header"]["n_components"][0] >= 1 and not raw["components"]["cone"].any()
    small = raw["components"]["n_points"] < c["cluster"]["min_points"]
    wide = np.maximum(raw["components"]["x_hi"] - raw["components"]["x_lo"], raw["components"]["y_hi"] - raw["components"]["y_lo"]) > c["cluster"]["max_width"]
    assert (small | wide).all()
    assert np.ptp(c["points"][:, 0]) > 0.5 and np.ptp(c["points"][:, 1]) > 0.5
    got, _ = twin(dk, c)
    fixed = cluster.cluster_numpy(got["out"], c["m"], c["cluster"])
    assert fixed["count"][0] == 1 and fixed["header"]["n_components"][0] == 1
    cone = fixed["cones"][0]
    assert abs(cone["x"] - dc.CONE_AT[0]) < 0.1 and abs(cone["y"] - dc.CONE_AT[1]) < 0.1 and cone["n_samples"] == 24
