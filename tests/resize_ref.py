"""A numpy restatement of the resizing nodes' definitions of include/esmstereo_amd.h (esm_resize_u8,
esm_preprocess_resize_u8) and of ResizeNode's picture and score, written from the definitions and importing nothing
from the package.  The taps are node_ref.linear_coords', the ones esm_depth16_to_disp_f32 is defined by.

Reference lines: virtual_kitti_publisher/src/virtual_kitti_publisher_cuda_node.cpp:232-266 (preprocess_image),
:131-213 (the picture: the left image at the network size, vconcat, the squeeze), :80-126 (computeEPE, computeD1);
kitti_publisher_ess/src/kitti_publisher_ess_cuda_node.cpp:241-275 (the same with mean 0, std 1).  The resize rule
restates OpenCV's 8-bit INTER_LINEAR; parity with OpenCV's own bytes is UNPINNED."""
import numpy as np

import node_ref as NR
import render_ref as RR

F32 = np.float32
COEF_ONE = 2048  # 1 << INTER_RESIZE_COEF_BITS


def taps(n_dst, n_src):
    """(i0, i1, a0, a1) along one axis: linear_coords' indices, a0 = rint((1.f - f) * 2048.f), a1 = rint(f * 2048.f)
    (the fp32 product, rounded half to even into an int)."""
    i0, i1, w0, w1 = NR.linear_coords(n_dst, n_src)
    a0 = np.rint(w0 * F32(COEF_ONE)).astype(np.int32)
    a1 = np.rint(w1 * F32(COEF_ONE)).astype(np.int32)
    return i0, i1, a0, a1


def resize_u8(src, H, W):
    """uint8 [..., Hs, Ws, C] -> uint8 [..., H, W, C], int32 arithmetic: the horizontal pass on every source row,
    D = S[x0] * a0 + S[x1] * a1, then v = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim >= 3
    s = src.astype(np.int32)
    y0, y1, b0, b1 = taps(H, src.shape[-3])
    x0, x1, a0, a1 = taps(W, src.shape[-2])
    D = s[..., :, x0, :] * a0[:, None] + s[..., :, x1, :] * a1[:, None]
    assert D.dtype == np.int32
    D0, D1 = D[..., y0, :, :] >> 4, D[..., y1, :, :] >> 4
    v = (((b0[:, None, None] * D0) >> 16) + ((b1[:, None, None] * D1) >> 16) + 2) >> 2
    assert v.dtype == np.int32 and v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def resize_grey(src, H, W):
    """uint8 [..., Hs, Ws] -> [..., H, W] (C = 1)."""
    return resize_u8(np.asarray(src)[..., None], H, W)[..., 0]


def normalize(u8, mean, std):
    """uint8 [..., H, W, 3] -> fp32 [..., 3, H, W]: ((float)u / 255 - mean[c]) / std[c], each operation rounded in
    fp32, channel c as stored."""
    u = np.asarray(u8)
    assert u.dtype == np.uint8 and u.shape[-1] == 3
    m, s = np.asarray(mean, F32), np.asarray(std, F32)
    v = (u.astype(F32) / F32(255) - m) / s
    assert v.dtype == F32
    return np.ascontiguousarray(np.moveaxis(v, -1, -3))


def preprocess_resize(img, H, W, mean, std):
    """esm_preprocess_resize_u8: (out fp32 [..., 3, H, W], resized uint8 [..., H, W, 3])."""
    r = resize_u8(img, H, W)
    return normalize(r, mean, std), r


def stack_and_squeeze(left_resized, filtered, lut):
    """The node's picture (:131-213 without the overlays) for ONE image: the left image at the network size over
    the auto-range colour-mapped disparity (vconcat), then the [2H, W, 3] stack resized to [H, W, 3] (:211-213)."""
    left_resized = np.asarray(left_resized, np.uint8)
    H, W, _ = left_resized.shape
    stack = RR.stack(left_resized, RR.apply_lut(RR.index_range_image(np.asarray(filtered, F32)), lut))
    assert stack.shape == (2 * H, W, 3)
    return resize_u8(stack, H, W)


def score(gt, est, hi=192.0):
    """computeEPE (:80-92) and computeD1 (:95-126): over (gt > 0) & (gt < 192), E = |est - gt| in fp32;
    -> (epe = the fp64 mean of E, d1 = 100 * bad / valid with bad = #(E > 3 && E / gt > 0.05), valid, bad); both
    rates are 0 over no pixel.  est enters as it is, zeros included."""
    gt, est = np.asarray(gt, F32), np.asarray(est, F32)
    mask = (gt > 0) & (gt < F32(hi))
    valid = int(mask.sum())
    E = np.abs(est - gt)[mask]
    bad = int(((E > F32(3)) & (E / gt[mask] > F32(0.05))).sum())
    if not valid:
        return 0.0, 0.0, 0, 0
    return float(E.astype(np.float64).sum() / valid), 100.0 * bad / valid, valid, bad
