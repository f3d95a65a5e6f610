"""CPU tests of the resizing nodes' front end (csrc/resize.hip, esmstereo_amd/io.py, esmstereo_amd/node.py): the numpy
restatement of the 8-bit resize rule (tests/resize_ref.py) against its own properties and an fp64 bilinear
interpolation, and the C ABI's argument errors, which are raised before any device work."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import node_ref as NR
import resize_ref as RZ
from esmstereo_amd import _lib

F32 = np.float32
#         source      destination
SHAPES = [((23, 37), (23, 37)), ((23, 37), (32, 64)), ((75, 131), (32, 64)), ((20, 150), (32, 64)),
          ((46, 74), (23, 37)), ((1, 5), (7, 9)), ((5, 1), (9, 7)), ((64, 37), (32, 37))]


def images(h, w, c=3, seed=0):
    """Random bytes, an all-255 image and a 0 / 255 checkerboard, [3, h, w, c]."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[:h, :w]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], c, axis=-1)
    return np.stack([rng.integers(0, 256, (h, w, c), dtype=np.uint8), np.full((h, w, c), 255, np.uint8), board])


@pytest.mark.parametrize("size", [(23, 37), (1, 5), (5, 1), (64, 37)])
def test_identity_sizes_return_the_source(size):
    img = images(*size)
    assert np.array_equal(RZ.resize_u8(img, *size), img)
    assert np.array_equal(RZ.resize_grey(img[..., 0], *size), img[..., 0])
    i0, i1, a0, a1 = RZ.taps(size[1], size[1])
    assert np.array_equal(i0, np.arange(size[1])) and (a0 == 2048).all() and (a1 == 0).all()


@pytest.mark.parametrize("src,dst", SHAPES)
def test_all_255_stays_255(src, dst):
    out = RZ.resize_u8(np.full(src + (3,), 255, np.uint8), *dst)
    assert out.shape == dst + (3,) and (out == 255).all()
    assert not RZ.resize_u8(np.zeros(src + (1,), np.uint8), *dst).any()


def test_coefficient_pairs_sum_to_2048():
    pairs = [(d, s) for (sh, sw), (dh, dw) in SHAPES for d, s in ((dh, sh), (dw, sw))]
    pairs += [(576, 375), (960, 1242), (576, 1152), (128, 100), (224, 220), (7, 1000), (1000, 7), (333, 1001)]
    for n_dst, n_src in pairs:
        i0, i1, a0, a1 = RZ.taps(n_dst, n_src)
        assert a0.dtype == np.int32 and ((a0 + a1) == RZ.COEF_ONE).all(), (n_dst, n_src)
        assert (a0 >= 0).all() and (a1 >= 0).all()
        assert (i0 >= 0).all() and (i1 <= n_src - 1).all() and ((i1 - i0) >= 0).all() and ((i1 - i0) <= 1).all()


@pytest.mark.parametrize("src,dst", SHAPES)
def test_within_the_derived_bound_of_an_fp64_bilinear_interpolation(src, dst):
    """Every byte within 1.3 grey levels of F.interpolate(bilinear, align_corners=False) in fp64 on the same image
    (the same sample positions: (i + 0.5) * n_src / n_dst - 0.5, clamped at both ends).  From the definition, with
    the exact result E = sum of S * wx * wy over the four taps:
      coefficients  |a / 2048 - w| <= 2^-12 for each of the two of a pass, on samples <= 255: 255 * 2 * 2^-12 <
                    0.125 per pass, 0.25 for both;
      D >> 4        drops under 16 / 2048 = 0.008 of a grey level;
      the two >> 16 drop under 1 each in units of a quarter grey level: under 0.25 each;
      + 2 >> 2      rounds to the nearest byte: at most 0.5;
    in all under 0.25 + 0.008 + 0.5 + 0.5 = 1.26.  The sample position is an fp32 (half an ulp of a coordinate below
    2048 is 2^-14, times a slope of at most 255 per pixel: under 0.016 per axis), which 1.3 still holds."""
    img = images(*src)
    got = RZ.resize_u8(img, *dst).astype(np.float64)
    t = torch.from_numpy(img.astype(np.float64)).permute(0, 3, 1, 2)
    ref = F.interpolate(t, size=dst, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    assert ref.dtype == np.float64 and ref.shape == got.shape
    worst = np.abs(got - ref).max()
    print("worst distance to fp64 bilinear", src, dst, worst)
    assert worst <= 1.3


def test_squeeze_averages_row_pairs():
    """The node's squeeze of a [2H, W, 3] stack with even H: rows 2y and 2y + 1 with coefficients 1024 and 1024, the
    columns untouched, so the top half of the frame depends on the top panel only."""
    H, W = 32, 37
    y0, y1, b0, b1 = RZ.taps(H, 2 * H)
    assert np.array_equal(y0, 2 * np.arange(H)) and np.array_equal(y1, 2 * np.arange(H) + 1)
    assert (b0 == 1024).all() and (b1 == 1024).all()
    rng = np.random.default_rng(5)
    top, bottom, other = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(3))
    a = RZ.resize_u8(np.concatenate((top, bottom)), H, W)
    b = RZ.resize_u8(np.concatenate((top, other)), H, W)
    assert np.array_equal(a[:H // 2], b[:H // 2]) and not np.array_equal(a[H // 2:], b[H // 2:])
    # 1024 * (S * 128) >> 16 = 2 S exactly, so v = (2 S0 + 2 S1 + 2) >> 2: the mean of the pair, halves rounded up
    s = np.concatenate((top, bottom)).astype(np.int32)
    assert np.array_equal(a, ((s[0::2] + s[1::2] + 1) >> 1).astype(np.uint8))
    # the picture itself: left over colour, squeezed
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    filtered = rng.uniform(0, 100, (H, W)).astype(F32)
    frame = RZ.stack_and_squeeze(top, filtered, lut)
    assert frame.shape == (H, W, 3) and np.array_equal(frame[:H // 2], a[:H // 2])


def test_normalize_is_the_preprocess_arithmetic():
    u = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    v = RZ.normalize(u, mean, std)
    assert v.shape == (3, 1, 256) and v.dtype == F32
    for c in range(3):
        want = (torch.arange(256, dtype=torch.float32).div(255) - torch.tensor(mean[c])) / torch.tensor(std[c])
        assert np.array_equal(v[c, 0], want.numpy())
    assert np.array_equal(RZ.normalize(u, (0, 0, 0), (1, 1, 1))[0, 0], np.arange(256, dtype=F32) / F32(255))
    out, r = RZ.preprocess_resize(u, 1, 256, mean, std)
    assert np.array_equal(r, u) and np.array_equal(out, v)


def test_score_restates_epe_and_d1():
    #              bad     E <= 3   rel <= 5 %   gt = 0   gt >= 192   est = 0 counts
    gt = np.array([[10.0,  10.0,    100.0,       0.0,     192.0,      4.0]], F32)
    est = np.array([[14.0, 12.0,    104.0,       50.0,    0.0,        0.0]], F32)
    epe, d1, valid, bad = RZ.score(gt, est)
    assert (valid, bad) == (4, 2) and epe == (4 + 2 + 4 + 4) / 4 and d1 == 50.0
    assert RZ.score(np.zeros((2, 2), F32), np.ones((2, 2), F32)) == (0.0, 0.0, 0, 0)
    assert epe == NR.epe(gt, est)


def test_package_exports_and_front_end_errors():
    import esmstereo_amd as E
    from esmstereo_amd import io as EIO, node as N
    assert E.resize_u8 is EIO.resize_u8 and E.resize_preprocess is EIO.resize_preprocess
    assert E.ResizeNode is N.ResizeNode and issubclass(N.ResizeNode, N.StereoNode)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.resize_u8(torch.zeros(4, 5, 3, dtype=torch.uint8), (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.resize_preprocess(torch.zeros(4, 5, 3, dtype=torch.uint8), (8, 8))
    for bad in (torch.zeros(4, 5, 3), torch.zeros(5, dtype=torch.uint8), torch.zeros(1, 4, 5, 2, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            E.resize_u8(bad, (8, 8))
    for bad in (torch.zeros(4, 5, 3), torch.zeros(4, 5, dtype=torch.uint8), torch.zeros(1, 4, 5, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            E.resize_preprocess(bad, (8, 8))


P = 0x1000  # a non-null address that is never dereferenced: every call below is refused before any device work
E_ARG = -1  # ESM_ERR_ARG
CONST = (_lib.c_float * 3)(0.5, 0.5, 0.5)


def _resize(src=P, dst=P, B=1, Hs=4, Ws=5, H=8, W=10, C=3):
    return _lib.lib.esm_resize_u8(src, dst, B, Hs, Ws, H, W, C, None)


def _pre(img=P, out=P, resized=None, B=1, Hs=4, Ws=5, H=8, W=10, mean=CONST, stdv=CONST):
    return _lib.lib.esm_preprocess_resize_u8(img, out, resized, B, Hs, Ws, H, W, mean, stdv, None)


def test_resize_argument_errors_without_gpu():
    err = _lib.lib.esm_last_error
    assert _resize(src=None) == E_ARG and b"null" in err()
    assert _resize(dst=None) == E_ARG and b"null" in err()
    for bad in (dict(B=0), dict(Hs=0), dict(Ws=-1), dict(H=0), dict(W=-2)):
        assert _resize(**bad) == E_ARG and b"non-positive" in err(), bad
    for c in (0, 2, 4, -1):
        assert _resize(C=c) == E_ARG and b"1 or 3" in err(), c
    assert _resize(B=65536) == E_ARG and b"65535" in err()
    assert _resize(Hs=1 << 16, Ws=1 << 15, C=1) == E_ARG and b"2^31" in err()  # Hs * Ws * C = 2^31
    assert _resize(H=1 << 16, W=1 << 15, C=1) == E_ARG and b"2^31" in err()
    assert _resize(Hs=1 << 15, Ws=1 << 15, C=3) == E_ARG and b"2^31" in err()   # 3 * 2^30
    assert _resize(H=1 << 15, W=1 << 15, C=3) == E_ARG and b"2^31" in err()


def test_preprocess_resize_argument_errors_without_gpu():
    err = _lib.lib.esm_last_error
    for name in ("img", "out", "mean", "stdv"):
        assert _pre(**{name: None}) == E_ARG and b"null" in err(), name
    for bad in (dict(B=0), dict(Hs=0), dict(Ws=-1), dict(H=0), dict(W=-2)):
        assert _pre(**bad) == E_ARG and b"non-positive" in err(), bad
        assert _pre(resized=P, **bad) == E_ARG
    assert _pre(B=65536) == E_ARG and b"65535" in err()
    assert _pre(Hs=1 << 15, Ws=1 << 15) == E_ARG and b"2^31" in err()
    assert _pre(H=1 << 15, W=1 << 15) == E_ARG and b"2^31" in err()
