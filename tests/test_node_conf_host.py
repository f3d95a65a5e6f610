"""CPU tests of the confidence-gated node's device work (esmstereo_amd/node.py, csrc/node_conf.hip): the numpy
restatement (tests/node_ref.py) on hand-set values, and the C ABI's argument errors, which are raised before any
device work."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import node_ref as NR
from esmstereo_amd import _lib

F32 = np.float32


def test_colour_table_identity():
    """convertTo(CV_8UC3, 255) of c / 255.f gives c back: the kernel may hold the integer table."""
    assert NR.ERR_COLOURS.size == 30
    assert np.array_equal(NR.colour_byte(NR.ERR_COLOURS), NR.ERR_COLOURS)
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(NR.colour_byte(every), every)


def test_error_bounds_are_powers_of_two():
    assert NR.ERR_BOUNDS.tolist() == [0, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 1, 2, 4, 8, 16, np.inf]


def test_error_map_rows():
    #                err = 1/16   err = 16   gt = 0   E/gt < E   E/gt > E   exact    below 1/16
    gt = np.array([[1.0,         1.0,       0.0,     4.0,       0.5,       3.0,     1.0]], F32)
    est = np.array([[0.9375,     17.0,      5.0,     6.0,       0.75,      3.0,     1.03125]], F32)
    assert NR.error_rows(est, gt).tolist() == [[1, 9, -1, 4, 3, 0, 0]]
    img = NR.error_panel(est, gt)
    assert img.shape == (1, 7, 3) and img.dtype == np.uint8
    assert img[0, 0].tolist() == [180, 117, 69]  # row 1 as (col4, col3, col2)
    assert img[0, 1].tolist() == [38, 0, 165]
    assert img[0, 2].tolist() == [0, 0, 0]       # outside the mask
    assert img[0, 5].tolist() == [149, 54, 49]
    # there is no division by 3 or 0.05 here: utils/visualization.py's vis would put E = 2, gt = 4 in another row
    assert NR.error_rows(np.array([[6.0]], F32), np.array([[4.0]], F32))[0, 0] == 4


def test_masked_gt_follows_the_filtered_map():
    filtered = np.array([[5.0, 0.0, 7.0, 3.0]], F32)
    gt16 = np.array([[256, 512, 0, 65535]], np.uint16)
    assert NR.masked_gt(filtered, gt16).tolist() == [[1.0, 0.0, 0.0, 65535 / 256]]
    assert NR.masked_gt(filtered, None).tolist() == [[0.0] * 4]
    frame, gt = NR.panels(filtered, None, gt16, np.zeros((1, 4, 3), np.uint8), np.zeros((256, 3), np.uint8))
    assert frame.shape == (2, 8, 3) and not frame[1, 4:].any()  # no confidence: black
    assert frame[0, 4].tolist() == [67, 109, 244]               # E = 4, rel = 4: row 7
    assert NR.epe(gt, filtered) == 4.0                          # 65535 / 256 is outside (0, 192)


@pytest.mark.parametrize("value,threshold,valid", [(0.29, 0.29, False), (0.57, 0.57, False), (0.3, 0.3, True),
                                                    (0.5, 0.5, True), (np.nan, 0.0, False), (0.0, 0.0, True)])
def test_gate_compares_in_fp64(value, threshold, valid):
    d = np.full((8, 8), 10.0, F32)
    c = np.full((8, 8), F32(value), F32)
    u, m, v = NR.node_filter_conf(d, c, 1, 2, 5, 4, 192.0, threshold)
    assert u.shape == (5, 4) and bool(v.all()) == valid and bool(v.any()) == valid
    assert (u == (2560 if valid else 0)).all() and (m == (10.0 if valid else 0.0)).all()


def test_gate_off_without_a_confidence():
    d = np.full((8, 8), 3.5 / 256, F32)  # 3.5 rounds to even
    d[0, 0] = -1
    u, m, v = NR.node_filter_conf(d, None, 0, 0, 8, 8, 192.0, 2.0)
    assert (u == 4).all() and v.all()
    u, m, v = NR.node_filter_conf(np.full((8, 8), 300.0, F32), None, 0, 0, 8, 8, 192.0, 0.0)
    assert not u.any() and not m.any() and not v.any()  # outside (0, max_disp)


def test_median_matches_scipy():
    import scipy.ndimage
    d = np.random.default_rng(0).standard_normal((23, 41)).astype(F32)
    assert np.array_equal(NR.median5_replicate(d), scipy.ndimage.median_filter(d, size=5, mode="nearest"))
    small = np.random.default_rng(1).standard_normal((3, 4)).astype(F32)  # both extents below 5
    assert np.array_equal(NR.median5_replicate(small), scipy.ndimage.median_filter(small, size=5, mode="nearest"))


def _source(h, w, seed):
    return np.random.default_rng(seed).uniform(0.5, 200.0, (2, h, w)).astype(F32)


def test_resize_identity_returns_the_source_bits():
    s = _source(23, 37, 0)
    assert np.array_equal(NR.resize_linear(s, 23, 37).view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("src,dst", [((23, 37), (46, 74)), ((46, 74), (23, 37))])
def test_resize_agrees_with_torch_at_exact_scales(src, dst):
    s = _source(*src, 1)
    ref = F.interpolate(torch.from_numpy(s)[:, None], size=dst, mode="bilinear", align_corners=False)[:, 0].numpy()
    got = NR.resize_linear(s, *dst)
    assert got.shape == (2,) + dst and got.dtype == F32
    # two lerps of three fp32 roundings each, with slack for the coefficient's 1 - fx
    assert np.abs(got.astype(np.float64) - ref).max() <= 8 * 2.0 ** -24 * np.abs(s).max()


def test_resize_agrees_with_fp64_at_an_odd_ratio():
    s = _source(23, 37, 2)
    got = NR.resize_linear(s, 32, 64)
    ref = NR.resize_linear(s, 32, 64, dtype=np.float64)  # the same fp32 coefficients, no rounding in between
    assert ref.dtype == np.float64 and not np.array_equal(got, ref)
    assert np.abs(got - ref).max() <= 8 * 2.0 ** -24 * np.abs(s).max()
    # the coordinates themselves: output 0 sits at (0.5 * 37 / 64 - 0.5) < 0 -> column 0 alone; the last at column 36
    x0, x1, w0, w1 = NR.linear_coords(64, 37)
    assert (x0[0], w0[0], w1[0]) == (0, 1.0, 0.0) and (x0[-1], x1[-1], w1[-1]) == (36, 36, 0.0)
    assert x0[1] == 0 and w1[1] == F32(1.5 * (37 / 64) - 0.5)


def test_depth_conversion():
    num = float(F32(725.0087) * F32(0.532725))
    d16 = np.array([[0, 1, 100, 65535]], np.uint16)
    s = NR.depth_to_disp(d16, num)
    assert s.dtype == F32 and s[0, 0] == 0.0
    assert s[0, 2] == F32(num) / (F32(100) * F32(0.01)) and s[0, 3] == F32(num) / (F32(65535) * F32(0.01))
    assert np.array_equal(NR.depth16_to_disp(d16, 1, 4, num), s)


def test_package_exports():
    import esmstereo_amd as E
    from esmstereo_amd import node as N
    assert E.ConfidenceNode is N.ConfidenceNode and E.depth16_to_disparity is N.depth16_to_disparity
    assert issubclass(N.ConfidenceNode, N.StereoNode)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.depth16_to_disparity(torch.zeros(4, 5, dtype=torch.int16), 700.0, 0.5)
    with pytest.raises(ValueError):
        N.depth16_to_disparity(torch.zeros(4, 5), 700.0, 0.5)


P = 0x1000  # a non-null address that is never dereferenced: every call below is refused before any device work
E_ARG = -1  # ESM_ERR_ARG


def _filter(disp=P, conf=P, out=P, B=1, Hp=8, Wp=8, top=2, left=1, h=3, w=4):
    return _lib.lib.esm_node_filter_conf_u16(disp, conf, out, None, None, B, Hp, Wp, top, left, h, w, 192.0, 0.5, None)


def test_filter_argument_errors_without_gpu():
    err = _lib.lib.esm_last_error
    assert _filter(disp=None) == E_ARG and b"null" in err()
    assert _filter(out=None) == E_ARG
    for bad in (dict(B=0), dict(Hp=0), dict(Wp=-1), dict(h=0), dict(w=0)):
        assert _filter(**bad) == E_ARG and b"non-positive" in err(), bad
    for bad in (dict(top=-1), dict(left=-1), dict(top=6), dict(left=5), dict(h=9), dict(w=9)):
        assert _filter(**bad) == E_ARG and b"window" in err(), bad
        assert _filter(conf=None, **bad) == E_ARG


def _panels(filtered=P, conf=P, Hp=8, Wp=8, top=2, left=1, gt16=P, left_img=P, lut=P, out=P, work=P, B=1, h=3, w=4):
    return _lib.lib.esm_node_panels_u8(filtered, conf, Hp, Wp, top, left, gt16, left_img, lut, out, None, work, B, h, w,
                                       None)


def test_panels_argument_errors_without_gpu():
    err = _lib.lib.esm_last_error
    for name in ("filtered", "left_img", "lut", "out", "work"):
        assert _panels(**{name: None}) == E_ARG and b"null" in err(), name
    for bad in (dict(B=0), dict(h=0), dict(w=-3)):
        assert _panels(**bad) == E_ARG and b"positive" in err(), bad
        assert _panels(conf=None, **bad) == E_ARG
    assert _panels(B=65536) == E_ARG and b"65535" in err()
    assert _panels(h=1 << 16, w=1 << 15, Hp=1 << 16, Wp=1 << 15, top=0, left=0) == E_ARG and b"2^31" in err()
    for bad in (dict(top=6), dict(left=5), dict(top=-1), dict(Hp=0)):
        assert _panels(**bad) == E_ARG, bad


def _depth(depth=P, out=P, B=1, Hs=4, Ws=5, H=8, W=10):
    return _lib.lib.esm_depth16_to_disp_f32(depth, out, B, Hs, Ws, H, W, 386.0, 0.01, None)


def test_depth_argument_errors_without_gpu():
    err = _lib.lib.esm_last_error
    assert _depth(depth=None) == E_ARG and b"null" in err()
    assert _depth(out=None) == E_ARG
    for bad in (dict(B=0), dict(Hs=0), dict(Ws=-1), dict(H=0), dict(W=0)):
        assert _depth(**bad) == E_ARG and b"non-positive" in err(), bad
    assert _depth(H=1 << 16, W=1 << 15) == E_ARG and b"2^31" in err()
