"""Every stream-taking entry point outside the hot path, captured on a side stream and replayed on other data
(tests/graph_replay.py says what that proves).

The conv forms, the pairs, the shuffle heads and the plan are replayed inside graphs already (ELSEWHERE names the
tests); the entry points below, the frame side of the nodes among them, were only ever launched on the default stream.
Shapes are the small ragged ones of the LDS-poison tests.  Calls of several launches are here on purpose: the three of
each codec (four chunks / several intervals per image, and two sets of pictures whose streams differ in length), the two
of esm_disp_metrics_f32, the range, fold and render launches of ESM_COLORIZE_RANGE at 513 partial ranges, normcorr.

The positive control runs once per module: a closure that launches esm_disp_to_u16 on a third stream while the side
stream captures must be rejected by the harness (its own assertion, or the runtime's error).  Where it is not, the
cases skip with that reason: the harness would prove nothing on such a machine.

tests/test_graph_replay_table_host.py holds REPLAYED and ELSEWHERE against include/esmstereo_amd.h.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

import esmstereo_amd as E  # noqa: E402
from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd._lib import CONF_ATTEND, CONF_COMBINE, CONF_COST_FEATURES, CONF_ENLARGE, CONF_SIGMOID  # noqa: E402
from esmstereo_amd.engine import ACT_SILU, Ctx  # noqa: E402
from graph_replay import assert_replays, stream  # noqa: E402

lib, check = _lib.lib, _lib.check
DEV = torch.device("cuda")
B = 2

# Exports with a `void* stream` that are not in REPLAYED below, and why.
_GRAPH = "replayed inside a graph already by tests/test_gpu_parity.py::"
ELSEWHERE = {
    "esm_conv_f32": _GRAPH + "test_forward_graph_matches_eager",
    "esm_gwc_stem_f32": _GRAPH + "test_forward_graph_matches_eager",
    "esm_shuffle_tail_f32": _GRAPH + "test_forward_graph_matches_eager",
    "esm_shuffle_conv_f32": _GRAPH + "test_forward_graph_matches_eager",
    "esm_conv_pair2_f32": _GRAPH + "test_forward_graph_matches_eager",
    "esm_convt_1x1_f32": _GRAPH + "test_forward_graph_matches_eager",
    "esm_plan_run": _GRAPH + "test_plan_modes_agree_and_probe",
    "esm_plan_run_op": _GRAPH + "test_plan_modes_agree_and_probe",
    "esm_plan_graph_build": _GRAPH + "test_plan_modes_agree_and_probe",
    "esm_plan_graph_launch": _GRAPH + "test_plan_modes_agree_and_probe",
    "esm_lds_fill_u32": "debug only",
    "esm_lds_probe_u32": "debug only",
}


def rnd(seed, *shape, lo=0.0, hi=1.0):
    return torch.from_numpy(np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32))


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def u8(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def u16(seed, *shape, hi=65536):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, hi, shape, dtype=np.uint16).view(np.int16))


def like(values):
    """Device tensors at fixed addresses for one set of values."""
    return [torch.empty_like(v, device=DEV) for v in values]


def buf(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=DEV)


# Each builder returns (launch, inputs, a, b, outputs); `where` gives the stream handle at call time.

# ---- io.hip, resize.hip

def io_disp_to_u16(where=stream):
    Hp, Wp, top, left, h, w = 40, 70, 3, 5, 31, 59
    a, b = [rnd(1, B, Hp, Wp, hi=200)], [rnd(2, B, Hp, Wp, hi=200)]
    (d,), out = like(a), buf(B, h, w, dtype=torch.int16)
    return (lambda: check(lib.esm_disp_to_u16(d.data_ptr(), out.data_ptr(), B, Hp, Wp, top, left, h, w, where()),
                          "disp_to_u16")), [d], a, b, [out]


def io_preprocess_u8(pad_normalized):
    H, W, Hp, Wp = 37, 61, 64, 64
    a, b = [u8(3, B, H, W, 3)], [u8(4, B, H, W, 3)]
    (img,), out = like(a), buf(B, 3, Hp, Wp)
    top, left = Hp - H, (Wp - W if pad_normalized else 0)
    return (lambda: check(lib.esm_preprocess_u8(img.data_ptr(), out.data_ptr(), B, H, W, Hp, Wp, top, left,
                                                pad_normalized, stream()), "preprocess")), [img], a, b, [out]


def io_node_filter_u16():
    Hp, Wp, top, left, h, w = 40, 70, 3, 5, 31, 59
    a, b = [rnd(5, B, Hp, Wp, lo=-20, hi=220)], [rnd(6, B, Hp, Wp, lo=-20, hi=220)]
    (d,), out, filt = like(a), buf(B, h, w, dtype=torch.int16), buf(B, h, w)
    return (lambda: check(lib.esm_node_filter_u16(d.data_ptr(), out.data_ptr(), filt.data_ptr(), B, Hp, Wp, top, left,
                                                  h, w, 192.0, stream()), "node_filter")), [d], a, b, [out, filt]


def resize_u8(C):
    Hs, Ws, H, W = 23, 37, 31, 59
    shape = (B, Hs, Ws, 3) if C == 3 else (B, Hs, Ws)
    a, b = [u8(7, *shape)], [u8(8, *shape)]
    (src,), dst = like(a), buf(*((B, H, W, 3) if C == 3 else (B, H, W)), dtype=torch.uint8)
    return (lambda: check(lib.esm_resize_u8(src.data_ptr(), dst.data_ptr(), B, Hs, Ws, H, W, C, stream()),
                          "resize_u8")), [src], a, b, [dst]


def preprocess_resize_u8():
    Hs, Ws, H, W = 46, 74, 23, 37
    a, b = [u8(9, B, Hs, Ws, 3)], [u8(10, B, Hs, Ws, 3)]
    (img,), out, resized = like(a), buf(B, 3, H, W), buf(B, H, W, 3, dtype=torch.uint8)
    mean, std = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    return (lambda: check(lib.esm_preprocess_resize_u8(img.data_ptr(), out.data_ptr(), resized.data_ptr(), B, Hs, Ws, H,
                                                       W, mean, std, stream()), "preprocess_resize")), [img], a, b, \
        [out, resized]


# ---- node_conf.hip

def node_filter_conf():
    Hp, Wp, top, left, h, w = 70, 150, 2, 7, 67, 141
    a = [rnd(11, 1, Hp, Wp, lo=-20, hi=220), rnd(12, 1, Hp, Wp)]
    b = [rnd(13, 1, Hp, Wp, lo=-20, hi=220), rnd(14, 1, Hp, Wp)]
    (d, c) = like(a)
    out, filt, valid = buf(1, h, w, dtype=torch.int16), buf(1, h, w), buf(1, h, w, dtype=torch.uint8)
    return (lambda: check(lib.esm_node_filter_conf_u16(d.data_ptr(), c.data_ptr(), out.data_ptr(), filt.data_ptr(),
                                                       valid.data_ptr(), 1, Hp, Wp, top, left, h, w, 192.0, 0.5,
                                                       stream()), "node_filter_conf")), [d, c], a, b, [out, filt, valid]


def _filtered(seed, *shape):
    """A masked median map as esm_node_filter_u16 leaves it: values in (0, 190), a fifth of the pixels 0."""
    m = rnd(seed, *shape, lo=0.01, hi=190.0)
    m[rnd(seed + 100, *shape) < 0.2] = 0.0
    return m


def node_panels():
    Hp, Wp, top, left, h, w = 70, 150, 2, 7, 67, 141  # five partial ranges: range pass + panels
    def values(s):
        return [_filtered(s, 1, h, w), rnd(s + 1, 1, Hp, Wp, lo=-0.1, hi=1.1), u16(s + 2, 1, h, w),
                u8(s + 3, 1, h, w, 3), u8(s + 4, 256, 3)]
    a, b = values(20), values(30)
    f, c, gt, img, lut = like(a)
    frame, gt_f32 = buf(1, 2 * h, 2 * w, 3, dtype=torch.uint8), buf(1, h, w)
    work = buf(E.range_workspace_bytes(1, h, w), dtype=torch.uint8)
    return (lambda: check(lib.esm_node_panels_u8(f.data_ptr(), c.data_ptr(), Hp, Wp, top, left, gt.data_ptr(),
                                                 img.data_ptr(), lut.data_ptr(), frame.data_ptr(), gt_f32.data_ptr(),
                                                 work.data_ptr(), 1, h, w, stream()), "node_panels")), \
        [f, c, gt, img, lut], a, b, [frame, gt_f32]


def depth16_to_disp():
    Hs, Ws, H, W = 23, 37, 46, 74
    a, b = [u16(40, B, Hs, Ws, hi=30000)], [u16(41, B, Hs, Ws, hi=30000)]
    (d16,), out = like(a), buf(B, H, W)
    return (lambda: check(lib.esm_depth16_to_disp_f32(d16.data_ptr(), out.data_ptr(), B, Hs, Ws, H, W, 386.1, 0.01,
                                                      stream()), "depth16_to_disp")), [d16], a, b, [out]


# ---- metrics.hip

def _metric_values(seed, H, W):
    gt = rnd(seed, B, H, W, lo=0.5, hi=230.0)
    gt[rnd(seed + 1, B, H, W) < 0.3] = 0.0
    est = gt + randn(seed + 2, B, H, W) * 2.0
    return [est, gt, rnd(seed + 3, B, H, W) < 0.8]


def disp_metrics():
    H, W = 7, 37
    a, b = _metric_values(50, H, W), _metric_values(60, H, W)
    est, gt, mask = like(a)
    records, values, batch = buf(B, 12, dtype=torch.float64), buf(B, 10), buf(10)
    work = buf(check(lib.esm_disp_metrics_workspace(B, H, W)), dtype=torch.uint8)
    thres = (ctypes.c_float * 3)(1.0, 2.0, 3.0)
    return (lambda: check(lib.esm_disp_metrics_f32(est.data_ptr(), H * W, W, gt.data_ptr(), H * W, W, mask.data_ptr(),
                                                   H * W, W, B, H, W, 0.0, 192.0, 1, thres, 3, 0.05, work.data_ptr(),
                                                   records.data_ptr(), values.data_ptr(), batch.data_ptr(), stream()),
                          "disp_metrics")), [est, gt, mask], a, b, [records, values, batch]


def disp_error_map():
    H, W = 23, 37  # (rows below 10 are the legend, whatever the input)
    a, b = _metric_values(70, H, W)[:2], _metric_values(80, H, W)[:2]
    (est, gt), out = like(a), buf(B, 3, H, W)
    return (lambda: check(lib.esm_disp_error_map_f32(est.data_ptr(), H * W, W, gt.data_ptr(), H * W, W, out.data_ptr(),
                                                     B, H, W, 3.0, 0.05, stream()), "disp_error_map")), \
        [est, gt], a, b, [out]


# ---- render.hip

def colorize(mode, nb, H, W, stacked, partials=None):
    from esmstereo_amd.render import COLORIZE_DEPTH, COLORIZE_RANGE, COLORIZE_SCALE
    code = {"scale": COLORIZE_SCALE, "range": COLORIZE_RANGE, "depth": COLORIZE_DEPTH}[mode]

    def values(s):
        d = _filtered(s, nb, H, W) if mode == "range" else rnd(s, nb, H, W, lo=0.5, hi=120.0)
        return [d, u8(s + 1, 256, 3)] + ([u8(s + 2, nb, H, W, 3)] if stacked else [])
    a, b = values(90), values(95)
    ins = like(a)
    d, lut, top = ins[0], ins[1], (ins[2] if stacked else None)
    out = buf(nb, 2 * H if stacked else H, W, 3, dtype=torch.uint8)
    work = None
    if mode == "range":
        nbytes = check(lib.esm_disp_colorize_workspace(nb, H, W))
        if partials is not None:  # (one partial and one folded record for a single pixel)
            assert check(lib.esm_disp_colorize_workspace(1, H, W)) // (lib.esm_disp_colorize_workspace(1, 1, 1) // 2) \
                == partials + 1
        work = buf(nbytes, dtype=torch.uint8)
    return (lambda: check(lib.esm_disp_colorize_u8(d.data_ptr(), H * W, W, nb, H, W, code, 0.01, 386.1 * 0.54, 80.0,
                                                   lut.data_ptr(), top.data_ptr() if stacked else None, out.data_ptr(),
                                                   work.data_ptr() if work is not None else None, stream()),
                          "disp_colorize")), ins, a, b, [out]


def disp_to_depth():
    H, W = 67, 131
    a, b = [rnd(100, B, H, W, lo=-1.0, hi=120.0)], [rnd(101, B, H, W, lo=-1.0, hi=120.0)]
    (d,), out = like(a), buf(B, H, W)
    return (lambda: check(lib.esm_disp_to_depth_f32(d.data_ptr(), H * W, W, out.data_ptr(), B, H, W, 386.1 * 0.54, 80.0,
                                                    stream()), "disp_to_depth")), [d], a, b, [out]


# ---- png.hip, jpeg.hip: three launches each; the two sets of pictures give streams of different lengths

def _png_buffers(rows, row_bytes):
    slot = check(lib.esm_png_stream_bound(rows * (1 + row_bytes)))
    work = buf(check(lib.esm_png_workspace_bytes(B, rows, row_bytes)), dtype=torch.uint8)
    return work, buf(B, slot, dtype=torch.uint8), slot, buf(B, dtype=torch.int32)


def png_u16(filt):
    import test_gpu_png as TP
    h, w = TP.shape_for(3 * TP.C + 5, 2)  # four chunks
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int16))  # noqa: E731
    a = [t(np.stack([TP.ramp_u16(h, w), TP.noise_u16(h, w, 5)]))]
    b = [t(np.stack([TP.noise_u16(h, w, 6), TP.ramp_u16(h, w)[::-1, ::-1]]))]
    (src,), (work, out, slot, lengths) = like(a), _png_buffers(h, 2 * w)
    return (lambda: check(lib.esm_png_encode_u16(src.data_ptr(), B, h, w, work.data_ptr(), out.data_ptr(), slot,
                                                 lengths.data_ptr(), filt, stream()), "png_encode_u16")), \
        [src], a, b, [out, lengths]


def png_rgb8(bgr):
    import test_gpu_png as TP
    h, w = TP.shape_for(3 * TP.C + 5, 3)
    y, x = np.mgrid[0:h, 0:w]
    smooth = torch.from_numpy(np.stack([(3 * x + y) % 256, (x + 2 * y) % 256, (x * y) % 256], axis=-1).astype(np.uint8))
    a, b = [torch.stack([smooth, u8(110, h, w, 3)])], [torch.stack([u8(111, h, w, 3), smooth.flip(0)])]
    (src,), (work, out, slot, lengths) = like(a), _png_buffers(h, 3 * w)
    return (lambda: check(lib.esm_png_encode_rgb8(src.data_ptr(), B, h, w, bgr, work.data_ptr(), out.data_ptr(), slot,
                                                  lengths.data_ptr(), 1, stream()), "png_encode_rgb8")), \
        [src], a, b, [out, lengths]


def png_disp_f32():
    Hp, Wp, top, left, h, w = 80, 70, 9, 6, 67, 59  # raw 67 * 119 = 7973 bytes: three chunks
    y, x = torch.meshgrid(torch.arange(Hp), torch.arange(Wp), indexing="ij")
    smooth = (20 + 0.11 * x + 0.07 * y).float()
    a, b = [torch.stack([smooth, rnd(120, Hp, Wp, hi=200)])], [torch.stack([rnd(121, Hp, Wp, hi=200), smooth * 2])]
    (d,), (work, out, slot, lengths) = like(a), _png_buffers(h, 2 * w)
    return (lambda: check(lib.esm_png_encode_disp_f32(d.data_ptr(), B, Hp, Wp, top, left, h, w, work.data_ptr(),
                                                      out.data_ptr(), slot, lengths.data_ptr(), 1, stream()),
                          "png_encode_disp")), [d], a, b, [out, lengths]


def jpeg_rgb8(sub):
    import test_gpu_jpeg as TJ
    h, w, ri = 37, 50, 3  # 12 MCUs of 420 (4 intervals), 35 of 444 (12 intervals)
    pic = lambda k: torch.from_numpy(TJ.picture(k, h, w).copy())  # noqa: E731
    a, b = [torch.stack([pic("ramp"), pic("noise")])], [torch.stack([pic("noise"), pic("checker")])]
    (src,) = like(a)
    work = buf(check(lib.esm_jpeg_workspace_bytes(B, h, w, sub, ri)), dtype=torch.uint8)
    slot = 3 * h * w
    out, lengths = buf(B, slot, dtype=torch.uint8), buf(B, dtype=torch.int32)
    return (lambda: check(lib.esm_jpeg_encode_rgb8(src.data_ptr(), B, h, w, 1, 75, sub, ri, work.data_ptr(),
                                                   out.data_ptr(), slot, lengths.data_ptr(), stream()),
                          "jpeg_encode_rgb8")), [src], a, b, [out, lengths]


# ---- volumes.hip, regression.hip

def _features(seed, C, H, W):
    return [randn(seed, B, C, H, W), randn(seed + 1, B, C, H, W)]


def volume(kind):
    C, G, D, H, W = 16, 8, 9, 5, 19
    a, b = _features(130, C, H, W), _features(140, C, H, W)
    if kind == "gwc*att":
        a, b = a + [rnd(132, B, G, H, W) + 0.5], b + [rnd(142, B, G, H, W) + 0.5]
    ins = like(a)
    L, R = (t.data_ptr() for t in ins[:2])
    if kind in ("gwc", "gwc*att"):
        V = buf(B, G, D, H, W)
        att = ins[2].data_ptr() if kind == "gwc*att" else None

        def launch():
            check(lib.esm_gwc_volume_f32(L, R, att, V.data_ptr(), B, C, H, W, D, G, stream()), kind)
    elif kind == "concat":
        V = buf(B, 2 * C, D, H, W)

        def launch():
            check(lib.esm_concat_volume_f32(L, R, V.data_ptr(), B, C, H, W, D, stream()), kind)
    else:
        V, work = buf(B, 1, D, H, W), buf(2, B, C, H, W)

        def launch():
            check(lib.esm_normcorr_volume_f32(L, R, V.data_ptr(), work.data_ptr(), B, C, H, W, D, stream()), kind)
    return launch, ins, a, b, [V]


def regression(kind):
    D, H, W = 9, 5, 19
    soft = lambda s: torch.softmax(randn(s, B, D, H, W), dim=1)  # noqa: E731
    a, b = [soft(150)], [soft(151)]
    if kind.endswith("samples"):
        a, b = a + [rnd(152, B, D, H, W, hi=48.0)], b + [rnd(153, B, D, H, W, hi=48.0)]
    ins, out = like(a), buf(B, 1, H, W)
    cost, samples, o = ins[0].data_ptr(), (ins[1].data_ptr() if len(ins) > 1 else None), out.data_ptr()

    def launch():
        if kind == "disp":
            rc = lib.esm_disp_regression_f32(cost, o, B, D, H, W, stream())
        elif kind.startswith("topk2"):
            rc = lib.esm_topk2_regression_f32(cost, samples, o, B, D, H, W, stream())
        else:
            rc = lib.esm_topk_regression_f32(cost, samples, o, B, D, H, W, 3, stream())
        check(rc, kind)
    return launch, ins, a, b, [out]


# ---- confidence.hip, dwconv.hip, smix.hip (through the package's descriptors; a Ctx takes the current stream)

def conf(op):
    C, D, H, W = 5, 9, 5, 19
    shapes, oshape, c, d = {
        CONF_COST_FEATURES: ([(B, D, H, W)], (B, 7, H, W), 0, D),
        CONF_ATTEND: ([(B, C, H, W)] * 3 + [(B, 3, H, W)], (B, 3 * C, H, W), C, 0),
        CONF_ENLARGE: ([(B, C, H, W), (B, 1, H, W)], (B, 9 * C, H, W), C, 0),
        CONF_COMBINE: ([(B, 9, 4 * H, 4 * W), (B, 1, H, W)], (B, 1, 4 * H, 4 * W), 0, 0),
        CONF_SIGMOID: ([(B, 1, H, W)], (B, 1, H, W), 1, 0),
    }[op]

    def values(s):
        xs = [randn(s + i, *shp) for i, shp in enumerate(shapes)]
        if op == CONF_ENLARGE:
            xs[1] = 2 * torch.sigmoid(3 * xs[1])
        return xs
    a, b = values(160), values(170)
    ins, out = like(a), buf(*oshape)
    return (lambda: Ctx(DEV).conf(op, ins, out, B, c, d, H, W)), ins, a, b, [out]


def dwconv(k, s):
    C, H, W = 5, 9, 21
    g = torch.Generator().manual_seed(k * 10 + s)
    w = (torch.randn(C, k * k, generator=g) * 0.3).to(DEV)
    sc, sh = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    p = (k - 1) // 2 if s == 1 else ((s - 1) + (k - 1)) // 2
    a, b = [randn(180, B, C, H, W)], [randn(181, B, C, H, W)]
    (x,) = like(a)
    out = EN.run_dwconv(Ctx(DEV), x, w, sc, sh, k, s, p, ACT_SILU)
    return (lambda: EN.run_dwconv(Ctx(DEV), x, w, sc, sh, k, s, p, ACT_SILU, out=out)), [x], a, b, [out]


def _fmblock(C):
    torch.manual_seed(7)
    blk = E.FMBlock(C, 7, 2).eval()
    with torch.no_grad():
        for n, prm in blk.named_parameters():
            if n.endswith("norm1.body.weight") or n.endswith("norm2.body.weight"):
                prm.uniform_(0.8, 1.2)
    return blk.to(DEV)._packed()


def smix(form, C=16):
    H, W = 7, 13
    p = _fmblock(C)
    a, b = [randn(190, B, C, H, W), randn(191, B, C, H, W)], [randn(192, B, C, H, W), randn(193, B, C, H, W)]
    x, res = like(a)
    out = buf(B, C, H, W)
    if form == "mlp":
        fn = lambda: EN.run_smix(Ctx(DEV), x, [p["a1"]], res=res, out=out)  # noqa: E731
    elif form == "dw+2mlp":
        fn = lambda: EN.run_smix(Ctx(DEV), x, [p["a2"], p["b1"]], dw=p["dw0"], res=res, out=out)  # noqa: E731
    else:
        fn = lambda: EN.run_smix(Ctx(DEV), x, [p["b2"]], dw=p["dw1"], res=res, out=out)  # noqa: E731
    return fn, [x, res], a, b, [out]


def fmnet(form, C):
    H, W = 7, 13
    p = _fmblock(C)
    st = [p["a1"], p["a2"], p["b1"], p["b2"]]
    a, b = [randn(200, B, C, H, W)], [randn(201, B, C, H, W)]
    (x,) = like(a)
    out, work = buf(B, C, H, W), buf(B, C, H, W)
    if form == "net":
        return (lambda: EN.run_fmnet(Ctx(DEV), x, st, p["dw0"], p["dw1"], out=out)), [x], a, b, [out]
    if form == "block":
        return (lambda: EN.run_fmnet(Ctx(DEV), x, st, p["dw0"], p["dw1"], out=out, conv=p["cw"], two_launch=False)), \
            [x], a, b, [out]
    return (lambda: EN.run_fmnet(Ctx(DEV), x, st, p["dw0"], p["dw1"], out=out, conv=p["cw"], two_launch=True,
                                 work=work)), [x], a, b, [out, work]


# id -> (export, builder, arguments): one case per entry point and mode
CASES = {
    "disp_to_u16": ("esm_disp_to_u16", io_disp_to_u16, ()),
    "preprocess_u8-pad-normalized": ("esm_preprocess_u8", io_preprocess_u8, (1,)),
    "preprocess_u8-pad-zero": ("esm_preprocess_u8", io_preprocess_u8, (0,)),
    "node_filter_u16": ("esm_node_filter_u16", io_node_filter_u16, ()),
    "resize_u8-rgb": ("esm_resize_u8", resize_u8, (3,)),
    "resize_u8-gray": ("esm_resize_u8", resize_u8, (1,)),
    "preprocess_resize_u8": ("esm_preprocess_resize_u8", preprocess_resize_u8, ()),
    "node_filter_conf_u16": ("esm_node_filter_conf_u16", node_filter_conf, ()),
    "node_panels_u8": ("esm_node_panels_u8", node_panels, ()),
    "depth16_to_disp": ("esm_depth16_to_disp_f32", depth16_to_disp, ()),
    "disp_metrics": ("esm_disp_metrics_f32", disp_metrics, ()),
    "disp_error_map": ("esm_disp_error_map_f32", disp_error_map, ()),
    "colorize-scale-stacked": ("esm_disp_colorize_u8", colorize, ("scale", 3, 67, 131, True)),
    "colorize-range-5-partials": ("esm_disp_colorize_u8", colorize, ("range", 3, 67, 131, True, 5)),
    "colorize-range-513-partials": ("esm_disp_colorize_u8", colorize, ("range", 1, 3, 350003, False, 513)),
    "colorize-depth": ("esm_disp_colorize_u8", colorize, ("depth", 3, 67, 131, False)),
    "disp_to_depth": ("esm_disp_to_depth_f32", disp_to_depth, ()),
    "png_u16-none": ("esm_png_encode_u16", png_u16, (0,)),
    "png_u16-sub": ("esm_png_encode_u16", png_u16, (1,)),
    "png_u16-up": ("esm_png_encode_u16", png_u16, (2,)),
    "png_rgb8-bgr": ("esm_png_encode_rgb8", png_rgb8, (1,)),
    "png_rgb8-rgb": ("esm_png_encode_rgb8", png_rgb8, (0,)),
    "png_disp_f32": ("esm_png_encode_disp_f32", png_disp_f32, ()),
    "jpeg-420": ("esm_jpeg_encode_rgb8", jpeg_rgb8, (420,)),
    "jpeg-444": ("esm_jpeg_encode_rgb8", jpeg_rgb8, (444,)),
    "gwc": ("esm_gwc_volume_f32", volume, ("gwc",)),
    "gwc*att": ("esm_gwc_volume_f32", volume, ("gwc*att",)),
    "concat": ("esm_concat_volume_f32", volume, ("concat",)),
    "normcorr": ("esm_normcorr_volume_f32", volume, ("normcorr",)),
    "disp_regression": ("esm_disp_regression_f32", regression, ("disp",)),
    "topk2_regression": ("esm_topk2_regression_f32", regression, ("topk2",)),
    "topk2_regression-samples": ("esm_topk2_regression_f32", regression, ("topk2-samples",)),
    "topk_regression-k3": ("esm_topk_regression_f32", regression, ("topk3",)),
    "topk_regression-k3-samples": ("esm_topk_regression_f32", regression, ("topk3-samples",)),
    "conf-cost-features": ("esm_conf_f32", conf, (CONF_COST_FEATURES,)),
    "conf-attend": ("esm_conf_f32", conf, (CONF_ATTEND,)),
    "conf-enlarge": ("esm_conf_f32", conf, (CONF_ENLARGE,)),
    "conf-combine": ("esm_conf_f32", conf, (CONF_COMBINE,)),
    "conf-sigmoid": ("esm_conf_f32", conf, (CONF_SIGMOID,)),
    "dwconv-k3s1": ("esm_dwconv_f32", dwconv, (3, 1)),
    "dwconv-k3s2": ("esm_dwconv_f32", dwconv, (3, 2)),
    "dwconv-k5s1": ("esm_dwconv_f32", dwconv, (5, 1)),
    "dwconv-k5s2": ("esm_dwconv_f32", dwconv, (5, 2)),
    "smix-mlp": ("esm_smix_f32", smix, ("mlp",)),
    "smix-dw+2mlp": ("esm_smix_f32", smix, ("dw+2mlp",)),
    "smix-dw+mlp-C8": ("esm_smix_f32", smix, ("dw+mlp", 8)),
    "fmnet-net-C8": ("esm_fmnet_f32", fmnet, ("net", 8)),
    "fmnet-block-C16": ("esm_fmnet_f32", fmnet, ("block", 16)),
    "fmnet-two-launches-C16": ("esm_fmnet_f32", fmnet, ("two", 16)),
}
REPLAYED = {export for export, _, _ in CASES.values()}


# ---------------------------------------------------------------------------------------------- the positive control

@pytest.fixture(scope="module")
def control():
    """A call that does what the harness exists to catch: its launch goes to a third stream, not the current one."""
    third = torch.cuda.Stream()
    case = io_disp_to_u16(where=lambda: ctypes.c_void_p(third.cuda_stream))
    try:
        assert_replays(*case, "positive control")
    except AssertionError as e:
        return dict(rejected=True, how=f"the harness: {e}")
    except Exception as e:  # noqa: BLE001
        return dict(rejected=True, how=f"the runtime: {type(e).__name__}: {e}")
    finally:
        torch.cuda.synchronize()
    return dict(rejected=False, how="a launch on a third stream during the capture passed every step")


@pytest.fixture
def harness(control):
    if not control["rejected"]:
        pytest.skip("the positive control was not rejected on this machine: " + control["how"])


def test_positive_control_is_rejected(control):
    print("graph replay, positive control:", control["how"])
    assert control["rejected"], control["how"]


@pytest.mark.parametrize("name", list(CASES))
def test_replays(name, harness):
    _, build, args = CASES[name]
    assert_replays(*build(*args), name)
