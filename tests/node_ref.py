"""A numpy restatement of the confidence-gated node's and the depth-image node's per-frame definitions of
include/esmstereo_amd.h (esm_node_filter_conf_u16, esm_node_panels_u8, esm_depth16_to_disp_f32), written from the
definitions and importing nothing from the package.

Reference lines: kitti_publisher_conf/src/kitti_publisher_conf_cuda_node.cpp:555-576 (the gate), :55-67 (computeEPE),
:69-151 (the node's own error map), :183-257 (the frame); virtual_kitti_publisher/src/
virtual_kitti_publisher_cuda_node.cpp:55-77,146-147 (depth to disparity, resized).  fp32 arithmetic throughout, one
rounding per operation, except where a definition says fp64."""
import numpy as np

import render_ref as RR

F32 = np.float32

# gen_error_colormap (:69-92): lower bound, upper bound, then the colour as the node writes it (R, G, B before its
# COLOR_RGB2BGR)
ERR_BOUNDS = np.array([F32(0.0) / F32(3.0), F32(0.1875) / F32(3.0), F32(0.375) / F32(3.0), F32(0.75) / F32(3.0),
                       F32(1.5) / F32(3.0), F32(3.0) / F32(3.0), F32(6.0) / F32(3.0), F32(12.0) / F32(3.0),
                       F32(24.0) / F32(3.0), F32(48.0) / F32(3.0), F32(np.inf)], dtype=F32)
ERR_COLOURS = np.array([[49, 54, 149], [69, 117, 180], [116, 173, 209], [171, 217, 233], [224, 243, 248],
                        [254, 224, 144], [253, 174, 97], [244, 109, 67], [215, 48, 39], [165, 0, 38]], dtype=np.uint8)


def median5_replicate(d):
    """cv::medianBlur(d, 5) of one [h, w] map with the border replicated inside the map: the 13th of the 25."""
    d = np.asarray(d, F32)
    h, w = d.shape
    p = np.pad(d, 2, mode="edge")
    stack = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)])
    return np.sort(stack, axis=0)[12]


def saturate_u16(r):
    return np.minimum(np.maximum(np.asarray(r, F32), F32(0)), F32(65535)).astype(np.uint16)


def node_filter_conf(disp, conf, top, left, h, w, max_disp, threshold):
    """One image: disp, conf [Hp, Wp] (conf may be None) -> (u16, filtered, valid) of the window (:555-576)."""
    m = median5_replicate(np.asarray(disp, F32)[top:top + h, left:left + w])
    valid = (m > 0) & (m < F32(max_disp))
    if conf is not None:
        c = np.asarray(conf, F32)[top:top + h, left:left + w]
        with np.errstate(invalid="ignore"):
            valid &= c.astype(np.float64) >= float(threshold)  # a float matrix against a double: fp64; NaN is invalid
    m = np.where(valid, m, F32(0))
    return saturate_u16(np.rint(m * F32(256))), m, valid


def masked_gt(filtered, gt16):
    """gt_mat.convertTo(CV_32FC1, 1 / 256), setTo(0, ~valid_mask) (:211-213); valid is filtered > 0."""
    filtered = np.asarray(filtered, F32)
    if gt16 is None:
        return np.zeros(filtered.shape, F32)
    gt = np.asarray(gt16, np.uint16).astype(F32) * (F32(1) / F32(256))
    return np.where(filtered > 0, gt, F32(0))


def error_rows(est, gt):
    """The row of gen_error_colormap each pixel falls in, -1 for none (:94-138): err = min(E, E / gt) over gt > 0."""
    est, gt = np.asarray(est, F32), np.asarray(gt, F32)
    mask = gt > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        E = np.abs(gt - est)
        rel = E / gt
        err = np.where(rel < E, rel, E)  # std::min(abs, rel)
        row = np.full(gt.shape, -1, np.int32)
        for i in range(10):
            row[mask & (err >= ERR_BOUNDS[i]) & (err < ERR_BOUNDS[i + 1])] = i
    return row


def colour_byte(c):
    """convertTo(CV_8UC3, 255.0) of the table's c / 255.f (:87,219)."""
    return RR.saturate_u8(np.rint((np.asarray(c, F32) / F32(255)) * F32(255)))


def error_panel(est, gt):
    """vis (:94-151) -> convertTo(CV_8UC3, 255) -> COLOR_RGB2BGR (:219-220): uint8 [..., 3], black outside."""
    row = error_rows(est, gt)
    table = np.concatenate([colour_byte(ERR_COLOURS)[:, ::-1], np.zeros((1, 3), np.uint8)])  # row -1: black
    return table[row]


def conf_panel(conf, shape):
    """conf_map.convertTo(CV_8UC1, 256.0), COLOR_GRAY2BGR (:204-205); NaN gives 0; black without a confidence."""
    if conf is None:
        return np.zeros(tuple(shape) + (3,), np.uint8)
    with np.errstate(invalid="ignore"):
        g = RR.saturate_u8(np.rint(np.asarray(conf, F32) * F32(256)))
    return np.repeat(g[..., None], 3, axis=-1)


def panels(filtered, conf, gt16, left_img, lut):
    """One image: (frame [2h, 2w, 3] uint8, gt_f32 [h, w]).  conf is already the window [h, w] or None."""
    filtered = np.asarray(filtered, F32)
    gt = masked_gt(filtered, gt16)
    disp_colour = RR.apply_lut(RR.index_range_image(filtered), lut)
    left_col = np.concatenate((np.asarray(left_img, np.uint8), disp_colour), axis=0)    # vconcat (:251)
    right_col = np.concatenate((error_panel(filtered, gt), conf_panel(conf, filtered.shape)), axis=0)  # (:254)
    return np.concatenate((left_col, right_col), axis=1), gt                              # hconcat (:257)


def epe(gt, est, hi=192.0):
    """computeEPE (:55-67): the fp64 mean of |est - gt| (fp32) over (gt > 0) & (gt < 192); 0 over no pixel, as
    cv::mean.  The sum runs in fp64 in whatever order; compare with a tolerance or against the device's records."""
    gt, est = np.asarray(gt, F32), np.asarray(est, F32)
    mask = (gt > 0) & (gt < F32(hi))
    n = int(mask.sum())
    return float(np.abs(gt - est)[mask].astype(np.float64).sum() / n) if n else 0.0


def depth_to_disp(depth16, num, depth_scale=0.01):
    """depthToDisparity (virtual_kitti...:55-77): z = d16 * scale; z <= 0 gives 0, else num / z."""
    z = np.asarray(depth16, np.uint16).astype(F32) * F32(depth_scale)
    with np.errstate(divide="ignore"):
        return np.where(z <= 0, F32(0), F32(num) / z).astype(F32)


def linear_coords(n_dst, n_src):
    """OpenCV's float INTER_LINEAR taps along one axis: (i0, i1, w0, w1) with w0 = 1 - f, w1 = f in fp32."""
    scale = float(n_src) / float(n_dst)
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f)
    f = f - s
    s = s.astype(np.int64)
    lo, hi = s < 0, s >= n_src - 1
    f = np.where(lo | hi, F32(0), f).astype(F32)
    s = np.where(lo, 0, np.where(hi, n_src - 1, s))
    return s, np.minimum(s + 1, n_src - 1), (F32(1) - f).astype(F32), f


def resize_linear(src, H, W, dtype=F32):
    """[..., Hs, Ws] -> [..., H, W]: horizontally first on the two rows, then vertically, every operation rounded in
    `dtype` (fp32 is the definition; fp64 evaluates the same fp32 coefficients without the roundings)."""
    src = np.asarray(src, F32).astype(dtype)
    y0, y1, wy0, wy1 = linear_coords(H, src.shape[-2])
    x0, x1, wx0, wx1 = linear_coords(W, src.shape[-1])
    wx0, wx1, wy0, wy1 = (a.astype(dtype) for a in (wx0, wx1, wy0, wy1))
    r = src[..., :, x0] * wx0 + src[..., :, x1] * wx1
    return r[..., y0, :] * wy0[:, None] + r[..., y1, :] * wy1[:, None]


def depth16_to_disp(depth16, H, W, num, depth_scale=0.01):
    return resize_linear(depth_to_disp(depth16, num, depth_scale), H, W)
