"""camera.nv12_to_tensor, the numpy float32 twin of the NV12 pre-process the stem kernel computes (include/unina_mi355.h at
unina_infer_nv12), pinned to the scalar oracle bit for bit: the no-resize form to oracle.preprocess_nv12, the resize
definition (ours; the reference has none) to oracle.preprocess_bgra on grey frames, the tile origin to a scalar evaluation
written out here. No GPU."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def camera(pkg):
    from unina_yolo_dla_amd import camera
    return camera


def nv12_frame(seed, h, w, grey=False):
    """Random NV12 planes without padding: y [h, w], uv [(h + 1) // 2, 2 * ((w + 1) // 2)]."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    uv = rng.integers(0, 256, ((h + 1) // 2, 2 * ((w + 1) // 2)), dtype=np.uint8)
    if grey:
        uv[:] = 128
    return y, uv


@pytest.mark.parametrize("h,w", [(50, 70), (7, 9), (64, 64)])   # row tails | odd both ways | whole quads
def test_twin_equals_oracle_without_resize(camera, oracle_mod, h, w):
    y, uv = nv12_frame(31, h, w)
    got = camera.nv12_to_tensor(y, uv)
    want = oracle_mod.preprocess_nv12(y, uv)
    assert got.dtype == np.float32 and got.shape == (3, h, w)
    assert got.tobytes() == want.tobytes()
    assert len(np.unique(got)) > 100 or h * w < 100          # (not a constant picture)


@pytest.mark.parametrize("src,dst", [((50, 70), (64, 64)), ((360, 640), (64, 96)), ((7, 9), (16, 16))])   # up | down | odd, up
def test_resize_definition_equals_bgra_resize_on_grey_frames(camera, oracle_mod, src, dst):
    """All chroma bytes 128: U = V = 0, so r = g = b = Y exactly and the clamps are idle -- the taps are the u8 luma values as
    floats, which is what the BGRA resize blends for a frame with B = G = R = Y."""
    h, w = src
    y, uv = nv12_frame(32, h, w, grey=True)
    img = np.empty((h, w, 4), dtype=np.uint8)
    img[..., :3] = y[..., None]
    img[..., 3] = np.random.default_rng(33).integers(0, 256, (h, w), dtype=np.uint8)
    got = camera.nv12_to_tensor(y, uv, dst_hw=dst)
    want = oracle_mod.preprocess_bgra(img, dst_hw=dst)
    assert got.shape == (3,) + dst and got.tobytes() == want.tobytes()


def scalar_pixel(y, uv, x0, y0, w, h, dst_h, dst_w, dy, dx, norm):
    """One output pixel of a tile, the definition written out operation by operation on np.float32 scalars."""
    f = np.float32

    def tap(xs, ys):
        X, Y = x0 + xs, y0 + ys
        Yv = f(y[Y, X])
        U = f(uv[Y // 2, (X // 2) * 2]) - f(128.0)
        V = f(uv[Y // 2, (X // 2) * 2 + 1]) - f(128.0)
        r = Yv + f(1.402) * V
        g = Yv - f(0.344136) * U - f(0.714136) * V
        b = Yv + f(1.772) * U
        return [max(f(0.0), min(f(255.0), v)) for v in (r, g, b)]

    if (dst_h, dst_w) == (h, w):
        rgb = tap(dx, dy)
    else:
        scale_x, scale_y = f(w) / f(dst_w), f(h) / f(dst_h)
        sx = (f(dx) + f(0.5)) * scale_x - f(0.5)
        sy = (f(dy) + f(0.5)) * scale_y - f(0.5)
        sx = max(f(0.0), min(sx, f(w) - f(1.0)))
        sy = max(f(0.0), min(sy, f(h) - f(1.0)))
        xa, ya = int(sx), int(sy)
        xb, yb = min(xa + 1, w - 1), min(ya + 1, h - 1)
        fx, fy = sx - f(xa), sy - f(ya)
        w00, w01, w10, w11 = (f(1.0) - fx) * (f(1.0) - fy), fx * (f(1.0) - fy), (f(1.0) - fx) * fy, fx * fy
        t00, t01, t10, t11 = tap(xa, ya), tap(xb, ya), tap(xa, yb), tap(xb, yb)
        rgb = [w00 * t00[c] + w01 * t01[c] + w10 * t10[c] + w11 * t11[c] for c in range(3)]
    out = [((rgb[c] / f(255.0)) - f(norm[c])) / f(norm[3 + c]) for c in range(3)]
    assert all(type(v) is np.float32 for v in out)
    return out


def test_tile_origin_enters_the_chroma_index(camera):
    y, uv = nv12_frame(34, 120, 160)
    # even origin: the tile is the crop (the chroma rows and pairs line up)
    x0, y0, w, h = 32, 18, 64, 48
    for dst in (None, (40, 56)):
        tile = camera.nv12_to_tensor(y, uv, dst_hw=dst, origin=(x0, y0), region=(w, h))
        crop = camera.nv12_to_tensor(y[y0:y0 + h, x0:x0 + w], uv[y0 // 2:(y0 + h + 1) // 2, x0:x0 + w], dst_hw=dst)
        assert tile.tobytes() == crop.tobytes()
    # odd origin: no crop of the planes gives it; every pixel against the scalar evaluation
    x0, y0, w, h = 33, 17, 21, 13
    for dst in ((h, w), (16, 20)):
        tile = camera.nv12_to_tensor(y, uv, dst_hw=dst, origin=(x0, y0), region=(w, h))
        assert tile.shape == (3,) + dst
        for dy in range(dst[0]):
            for dx in range(dst[1]):
                want = scalar_pixel(y, uv, x0, y0, w, h, dst[0], dst[1], dy, dx, camera.IMAGENET)
                assert [tile[c, dy, dx] for c in range(3)] == want, (dst, dy, dx)
    # and the odd origin does differ from the neighbouring even one shifted (the chroma pairing is not translation-invariant)
    a = camera.nv12_to_tensor(y, uv, origin=(33, 17), region=(20, 12))
    b = camera.nv12_to_tensor(y[17:, 33:], uv[8:, 32:], region=(20, 12))    # pairs start one pixel early: not the same picture
    assert a.tobytes() != b.tobytes()


def test_bad_regions_are_refused(camera):
    y, uv = nv12_frame(35, 10, 12)
    for kw in (dict(origin=(1, 0), region=(12, 10)), dict(region=(0, 4)), dict(origin=(-1, 0)), dict(dst_hw=(0, 4))):
        with pytest.raises(ValueError):
            camera.nv12_to_tensor(y, uv, **kw)
    with pytest.raises(ValueError):
        camera.nv12_to_tensor(y, uv[:4])                       # a chroma row short
