"""What the tests of the stages that take a LiDAR sweep (lidar, ground) share: the cloud they upload, with NaN bit patterns where
a correct kernel never reads, the strides they sweep, one ulp beside a threshold, and the refusals of csrc/cloud_io.h -- the list
of bad clouds and extrinsics and the call that a refusal test makes with one argument spoiled at a time."""
import ctypes as C

import numpy as np

F = np.float32
STRIDES = (16, 12, 32, 48)
POINTS = 0x30004                  # the base of a refusal test's cloud: never dereferenced; 4-byte aligned, not 16
CLOUD = dict(n_points=500, stride=16, points=POINTS)
MAX_POINTS = 1000                 # of the handle a refusal test creates


def ulp(v, towards):
    return np.nextafter(F(v), F(towards))


def upload_cloud(torch, pts, stride=16, offset=0):
    """[n, 3] float32 -> a [n, stride] uint8 CUDA view that starts `offset` bytes into its allocation; every word that is not a
    coordinate is a NaN bit pattern."""
    n = len(pts)
    host = np.full((offset + n * stride) // 4 + 4, 0x7fc00000, dtype=np.uint32)
    rows = host[offset // 4:offset // 4 + n * stride // 4].reshape(n, stride // 4)
    rows[:, :3] = np.ascontiguousarray(pts, dtype=np.float32).view(np.uint32)
    dev = torch.from_numpy(host.view(np.uint8)).cuda()
    return dev[offset:offset + n * stride].view(n, stride)


def bad_cloud_args(extrinsic):
    """Keywords of caller()'s call, each of which cloud_ok or extrinsic_ok refuses: n_points -1 and max + 1, strides 8, 0, -16, 14
    and 18, a base 2 and 1 bytes off, and each of the 12 extrinsic values as NaN, inf and -inf."""
    nan, inf = float("nan"), float("inf")
    return [dict(n_points=-1), dict(n_points=MAX_POINTS + 1), dict(stride=8), dict(stride=0), dict(stride=-16), dict(stride=14), dict(stride=18),
            dict(points=POINTS + 2), dict(points=POINTS + 1),
            *[dict(m=[v if j == i else e for j, e in enumerate(extrinsic)]) for i in range(12) for v in (nan, inf, -inf)]]


def caller(invoke, extrinsic, **tables):
    """call(**kw) of a refusal test. `tables`: the default fields of the entry point's structs by name; "cloud" is CLOUD. A keyword
    that is a field of one of them replaces it there, m replaces the extrinsic, every other keyword goes on to
    invoke(fields, float[12], **others), which builds the structs from fields[name] and returns the entry point's code."""
    def call(m=extrinsic, **kw):
        fields = {name: dict(t) for name, t in dict(tables, cloud=CLOUD).items()}
        others = {}
        for k, v in kw.items():
            next((t for t in fields.values() if k in t), others)[k] = v
        return invoke(fields, (C.c_float * 12)(*m), **others)
    return call
