"""CPU tests of the rendering feature (esmstereo_amd/render.py, csrc/render.hip): the numpy restatement
(tests/render_ref.py) on hand-computed values, the shipped colour tables, the 8-bit PNG writer, and the C ABI's
argument errors, which are raised before any device work."""
import io

import numpy as np
import pytest
import torch

import render_ref as RR
from esmstereo_amd import _lib
from esmstereo_amd import render as R

F32 = np.float32


def test_scale_ties_round_half_to_even():
    u = np.array([50, 150, 250, 350])
    d = (u / 256).astype(F32)
    assert RR.to_u16(d).tolist() == u.tolist()
    assert RR.index_scale(d, 0.01).tolist() == [0, 2, 2, 4]


def test_scale_saturates_at_25550():
    u = np.array([25549, 25550, 25551, 40000, 65535])
    d = (u / 256).astype(F32)
    assert RR.to_u16(d).tolist() == u.tolist()
    assert RR.index_scale(d, 0.01).tolist() == [255] * 5
    assert RR.index_scale(np.array([0.0, 100 / 256], F32), 0.01).tolist() == [0, 1]


def test_scale_u16_wraps_and_specials():
    # the low 16 bits of the integer: -1/256 -> 0xFFFF, 256 -> 0; NaN -> 0; +inf saturates int32 -> 0xFFFF
    d = np.array([-1 / 256, 256.0, np.nan, np.inf, -np.inf], F32)
    assert RR.to_u16(d).tolist() == [0xFFFF, 0, 0, 0xFFFF, 0]


def test_range_min_maps_to_255_and_max_to_0():
    m = np.array([[0.0, 1.0, 2.0, 3.0]], F32)  # u = 0 (invalid), 256, 512, 768
    a, b = RR.range_coefficients(256, 768)
    assert a == F32(-255.0 / 512) and b == F32(382.5)
    # the invalid pixel goes through the same formula: rint(382.5) = 382 -> 255; the middle: rint(127.5) = 128
    assert RR.index_range_image(m).tolist() == [[255, 255, 128, 0]]


def test_range_negative_nan_inf_are_handled():
    m = np.array([[-3.0, np.nan, np.inf, 1.0, 2.0]], F32)  # u = 0, 0, 65535, 256, 512: mn = 256, mx = 65535
    u, valid = RR.range_u(m)
    assert u.tolist() == [[0, 0, 65535, 256, 512]] and valid.tolist() == [[False, False, True, True, True]]
    idx = RR.index_range_image(m)
    assert idx[0, 2] == 0 and idx[0, 3] == 255 and idx[0, 0] == 255


def test_range_degenerate_images_are_index_zero():
    assert not RR.index_range_image(np.zeros((3, 4), F32)).any()                      # no valid pixel
    assert not RR.index_range_image(np.array([[0, -1, np.nan]], F32)).any()
    m = np.full((3, 4), 7.25, F32)
    m[1, 2] = 0
    assert not RR.index_range_image(m).any()                                          # max == min
    both = RR.index_range(np.stack([np.zeros((3, 4), F32), np.arange(12, dtype=F32).reshape(3, 4)]))
    assert not both[0].any() and both[1, 2, 3] == 0 and both[1, 0, 1] == 255


def test_depth_hand_values():
    num, max_depth = F32(0.05 * 640), 5.0
    d = np.array([0.0, 1e-3, 3.3, -2.0, np.nan, np.inf], F32)
    assert RR.index_depth(d, num, max_depth).tolist() == [0, 0, 0, 255, 255, 255]
    z = RR.depth_map(d, num, max_depth)
    assert z[:4].tolist() == [5.0, 5.0, 5.0, 0.0] and np.isnan(z[4]) and z[5] == 0.0
    # inside the range: 32 / 10 = 3.2 -> n = 0.64 -> uint8(163.2) = 163 -> 92
    assert RR.index_depth(np.array([10.0], F32), num, max_depth).tolist() == [255 - 163]


def test_stack_and_lut():
    lut = np.arange(768, dtype=np.uint16).reshape(256, 3).astype(np.uint8)
    idx = np.array([[[0, 255], [7, 8]]], np.uint8)
    img = RR.apply_lut(idx, lut)
    assert img.shape == (1, 2, 2, 3) and img[0, 1, 0].tolist() == lut[7].tolist()
    top = np.full((1, 2, 2, 3), 9, np.uint8)
    s = RR.stack(top, img)
    assert s.shape == (1, 4, 2, 3) and (s[:, :2] == 9).all() and np.array_equal(s[:, 2:], img)


def test_shipped_tables():
    for name in ("jet", "magma"):
        t = R.colormap_lut(name, "cpu", order="rgb")
        assert t.dtype == torch.uint8 and tuple(t.shape) == (256, 3) and t.is_contiguous()
        assert torch.equal(R.colormap_lut(name, "cpu"), t.flip(1))  # the default order is BGR
    magma = R.colormap_lut("magma", "cpu", order="rgb").numpy()
    jet = R.colormap_lut("jet", "cpu", order="rgb").numpy()
    assert tuple(magma[0]) == (0, 0, 4) and tuple(magma[128]) == (183, 55, 121) and tuple(magma[255]) == (252, 253, 191)
    assert tuple(jet[0]) == (0, 0, 128) and tuple(jet[255]) == (128, 0, 0)
    with pytest.raises(KeyError):
        R.colormap_lut("viridis", "cpu")
    with pytest.raises(ValueError):
        R.colormap_lut("jet", "cpu", order="gbr")


def test_png_rgb8_round_trip():
    from PIL import Image
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    im = Image.open(io.BytesIO(R.png_rgb8_bytes(a, order="rgb")))
    assert im.mode == "RGB" and im.size == (7, 5) and np.array_equal(np.asarray(im), a)
    im = Image.open(io.BytesIO(R.png_rgb8_bytes(a)))  # BGR in, as cv2.imwrite takes it
    assert np.array_equal(np.asarray(im), a[:, :, ::-1])
    with pytest.raises(ValueError):
        R.png_rgb8_bytes(a[:, :, 0])


def test_write_png_bgr8(tmp_path):
    from PIL import Image
    a = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    R.write_png_bgr8(str(tmp_path / "f.png"), torch.from_numpy(a))
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "f.png"))), a[:, :, ::-1])


def test_cpu_tensors_are_refused():
    lut = R.colormap_lut("jet", "cpu")
    d = torch.zeros(1, 4, 5)
    for call in (lambda: R.colorize_disparity(d, lut), lambda: R.colorize_range(d, lut),
                 lambda: R.disparity_to_depth(d, 0.05, 640, 5.0), lambda: R.colorize_depth(d, 0.05, 640, 5.0, lut)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_package_exports():
    import esmstereo_amd as E
    for name in R.__all__:
        assert getattr(E, name) is getattr(R, name)


P = 0x1000  # a non-null address that is never dereferenced: every call below is refused before any device work


def _colorize(disp=P, sb=20, sh=5, B=1, H=4, W=5, mode=_lib.COLORIZE_SCALE, lut=P, top=None, out=P, work=None):
    return _lib.lib.esm_disp_colorize_u8(disp, sb, sh, B, H, W, mode, 0.01, 32.0, 5.0, lut, top, out, work, None)


def test_colorize_argument_errors_without_gpu():
    E = -1  # ESM_ERR_ARG
    assert _colorize(disp=None) == E and b"null" in _lib.lib.esm_last_error()
    assert _colorize(lut=None) == E and _colorize(out=None) == E
    assert _colorize(mode=3) == E and b"mode" in _lib.lib.esm_last_error()
    assert _colorize(mode=-1) == E
    assert _colorize(mode=_lib.COLORIZE_RANGE) == E and b"workspace" in _lib.lib.esm_last_error()
    assert _colorize(B=0) == E and _colorize(H=0) == E and _colorize(W=-1) == E
    assert _colorize(sb=-1) == E and _colorize(sh=-1) == E and b"stride" in _lib.lib.esm_last_error()
    assert _colorize(H=1 << 16, W=1 << 15) == E and b"2^31" in _lib.lib.esm_last_error()


def test_depth_argument_errors_without_gpu():
    f = _lib.lib.esm_disp_to_depth_f32
    assert f(None, 20, 5, P, 1, 4, 5, 32.0, 5.0, None) == -1 and f(P, 20, 5, None, 1, 4, 5, 32.0, 5.0, None) == -1
    assert f(P, 20, 5, P, 1, 0, 5, 32.0, 5.0, None) == -1 and f(P, -1, 5, P, 1, 4, 5, 32.0, 5.0, None) == -1
    assert f(P, 20, 5, P, 1, 1 << 16, 1 << 15, 32.0, 5.0, None) == -1


def test_workspace_query():
    q = _lib.lib.esm_disp_colorize_workspace
    assert q(1, 1, 1) > 0 and q(2, 375, 1242) == 2 * q(1, 375, 1242)
    assert q(1, 1100, 1000) > q(1, 1000, 1000)  # grows with the number of workgroups
    assert q(0, 4, 4) == -1 and q(1, 1 << 16, 1 << 15) == -1
