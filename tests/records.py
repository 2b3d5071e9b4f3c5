"""What the GPU tests of the record stages (evalmatch, locate, stereo, track) and of the sweep stages (lidar, ground) share: the
device buffers they upload, with garbage where a correct kernel never reads, and the report of a byte comparison of two arrays."""
import numpy as np

MAXD = 1024                       # MAX_DETECTIONS


def padded_words(records, n_words: int) -> np.ndarray:
    """int32 [n_words]: the records' words first, NaN bit patterns behind them."""
    host = np.full(n_words, 0x7fc00000, dtype=np.int32)
    words = np.ascontiguousarray(records).view(np.int32).reshape(-1)
    host[:len(words)] = words
    return host


def det_buffer(torch, dets, count):
    """Engine.infer_async's int32 buffer on the device (word 0 = count, records from word 8); NaN bit patterns behind the
    records."""
    from unina_yolo_dla_amd.engine import DET_DTYPE
    host = padded_words(np.ascontiguousarray(dets, dtype=DET_DTYPE), 8 * MAXD)
    return torch.from_numpy(np.concatenate([np.array([count] + [0] * 7, dtype=np.int32), host])).cuda()


def assert_records_equal(got, want, name, what=""):
    """Byte equality of two record arrays, or of two plain arrays row by row; the report names the first record that differs."""
    if got.tobytes() != want.tobytes():
        assert got.shape == want.shape, (name, what, got.shape, want.shape)
        bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError(f"{name}: {len(bad)} {what + ' ' if what else ''}records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")
