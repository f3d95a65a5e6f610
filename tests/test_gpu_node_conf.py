"""GPU tests of the confidence-gated node's device work (csrc/node_conf.hip, esmstereo_amd/node.py): every comparison
is bit-exact against the numpy restatement (tests/node_ref.py).

Shapes: the existing node test's (B = 2, a 31 x 59 window at (3, 5) of a 40 x 70 map: one tile across, ragged); a
3 x 4 window at (2, 1) of an 8 x 8 map (both extents below 5: the replicate clamp acts on both sides at once); a
67 x 141 window at (2, 7) of a 70 x 150 map (3 x 9 tiles of 64 x 8 with ragged edges, rows of the frame at every byte
alignment); for the panels also 3 x 175000 and 3 x 350003 windows (257 and 513 partial ranges: a second round of the
panel kernel's fold of the partials, and the range folded by a launch of its own)."""
import json
import os

import numpy as np
import pytest
import torch

import node_ref as NR
from lds_poison import assert_leftover_free
from helpers import GOLDEN_DIR, load_spec, seeded_state

pytestmark = pytest.mark.gpu

import esmstereo_amd as E  # noqa: E402
from esmstereo_amd._lib import check, lib  # noqa: E402
from esmstereo_amd.backbone import StubFeature  # noqa: E402
from esmstereo_amd.node import ConfidenceNode, StereoNode, depth16_to_disparity  # noqa: E402
from oracle import io_oracle as IO  # noqa: E402

DEV = torch.device("cuda")
F32 = np.float32
MAX_DISP = 192.0
#          B, Hp, Wp, top, left, h, w
SHAPES = {"node": (2, 40, 70, 3, 5, 31, 59), "tiny": (1, 8, 8, 2, 1, 3, 4), "tiles": (1, 70, 150, 2, 7, 67, 141)}
# the panels alone (the filter's tests do not take these): the partial ranges of one image past the 256 that one round
# of the panel kernel's own fold takes, and past the 512 above which the range is folded by a launch of its own
ROUND_SHAPES = {"257-partials": (1, 6, 175009, 2, 4, 3, 175000), "513-partials": (1, 6, 350012, 2, 4, 3, 350003)}


def shape(name):
    return SHAPES[name] if name in SHAPES else ROUND_SHAPES[name]


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


def filter_inputs(name, threshold):
    """(disp, conf) [B, Hp, Wp]: disparities uniform in (-20, 220) with a run of 2.5 / 256 half-way cases; confidences
    uniform in [0, 1] with float32(0.29), float32(0.57), the threshold itself and NaN planted inside the window."""
    B, Hp, Wp, top, left, h, w = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    d = rng.uniform(-20, 220, (B, Hp, Wp)).astype(F32)
    c = rng.uniform(0, 1, (B, Hp, Wp)).astype(F32)
    if w >= 16:
        d[0, top + h // 3 - 2:top + h // 3 + 3, left + 4:left + 16] = F32(2.5 / 256)  # medians of 2.5 / 256
        c[0, top + h // 3, left + 4:left + 16] = 1.0
    else:
        d[0] = F32(2.5 / 256)
    win = c[:, top:top + h, left:left + w]
    flat = rng.permutation(win[0].size)
    for k, v in enumerate((F32(0.29), F32(0.57), F32(threshold), F32(np.nan))):
        for j in flat[k::4][:max(1, win[0].size // 8)]:
            win[0, j // w, j % w] = v
    return d, c


def run_filter(d, c, name, threshold, want_valid=True):
    B, Hp, Wp, top, left, h, w = SHAPES[name]
    dd, cc = dev(d), (dev(c) if c is not None else None)
    out = torch.full((B, h, w), -1, dtype=torch.int16, device=DEV)
    filt = torch.full((B, h, w), -7.0, device=DEV)
    valid = torch.full((B, h, w), 9, dtype=torch.uint8, device=DEV)
    check(lib.esm_node_filter_conf_u16(dd.data_ptr(), cc.data_ptr() if cc is not None else None, out.data_ptr(),
                                       filt.data_ptr(), valid.data_ptr() if want_valid else None, B, Hp, Wp, top, left,
                                       h, w, MAX_DISP, float(threshold), None), "node_filter_conf")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16), filt.cpu().numpy(), valid.cpu().numpy()


def ref_filter(d, c, name, threshold):
    B, Hp, Wp, top, left, h, w = SHAPES[name]
    r = [NR.node_filter_conf(d[b], None if c is None else c[b], top, left, h, w, MAX_DISP, threshold) for b in range(B)]
    return tuple(np.stack([x[k] for x in r]) for k in range(3))


@pytest.mark.parametrize("threshold", [0.29, 0.57, 0.5])
@pytest.mark.parametrize("name", list(SHAPES))
def test_filter_conf_bit_exact(name, threshold):
    d, c = filter_inputs(name, threshold)
    u, m, v = run_filter(d, c, name, threshold)
    ru, rm, rv = ref_filter(d, c, name, threshold)
    # the planted values decide pixels: float32(0.29) < 0.29 and float32(0.57) < 0.57 in fp64, 0.5 == 0.5
    _, _, rv_open = ref_filter(d, None, name, threshold)
    B, Hp, Wp, top, left, h, w = SHAPES[name]
    exact = (c[:, top:top + h, left:left + w] == F32(threshold)) & rv_open
    assert exact.any() and bool(rv[exact].all()) == (threshold == 0.5) and bool(rv[exact].any()) == (threshold == 0.5)
    assert np.array_equal(u, ru) and np.array_equal(v, rv.astype(np.uint8))
    assert np.array_equal(m.view(np.uint32), rm.view(np.uint32))
    assert 0 < rv.sum() < rv_open.sum()
    # `valid` is optional
    u2, m2, v2 = run_filter(d, c, name, threshold, want_valid=False)
    assert np.array_equal(u2, ru) and np.array_equal(m2, rm) and (v2 == 9).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_filter_without_conf_equals_node_filter(name):
    B, Hp, Wp, top, left, h, w = SHAPES[name]
    d, _ = filter_inputs(name, 0.5)
    u, m, v = run_filter(d, None, name, 2.0)  # the threshold is not read
    dd = dev(d)
    out = torch.empty(B, h, w, dtype=torch.int16, device=DEV)
    filt = torch.empty(B, h, w, device=DEV)
    check(lib.esm_node_filter_u16(dd.data_ptr(), out.data_ptr(), filt.data_ptr(), B, Hp, Wp, top, left, h, w, MAX_DISP,
                                  None), "node_filter")
    torch.cuda.synchronize()
    assert np.array_equal(u, out.cpu().numpy().view(np.uint16))
    assert np.array_equal(m.view(np.uint32), filt.cpu().numpy().view(np.uint32))
    assert np.array_equal(v, (m > 0).astype(np.uint8))
    for b in range(B):
        ru, rm = IO.node_filter_u16(d[b], top, left, h, w, MAX_DISP)
        assert np.array_equal(u[b], ru) and np.array_equal(m[b], rm)


@pytest.mark.parametrize("poison", [1e30, np.nan])
@pytest.mark.parametrize("name", list(SHAPES))
def test_filter_ignores_the_map_outside_the_window(name, poison):
    B, Hp, Wp, top, left, h, w = SHAPES[name]
    d, c = filter_inputs(name, 0.5)
    want = run_filter(d, c, name, 0.5)
    inside = np.zeros((Hp, Wp), bool)
    inside[top:top + h, left:left + w] = True
    dp, cp = (np.where(inside, a, F32(poison)).astype(F32) for a in (d, c))
    got = run_filter(dp, cp, name, 0.5)
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)


# ---- panels -------------------------------------------------------------------------------------------------------

def panel_inputs(name, special=False):
    B, Hp, Wp, top, left, h, w = shape(name)
    rng = np.random.default_rng(7 + sum(map(ord, name)))
    if special:
        # one image with no valid pixel (the empty-range rule), one whose valid pixels all hold one value (mx == mn)
        filtered = np.zeros((2, h, w), F32)
        filtered[1] = np.where(rng.uniform(0, 1, (h, w)) < 0.7, F32(7.25), F32(0))
        filtered[1, 0, 0] = 7.25
        B = 2
    else:
        d = rng.uniform(-20, 220, (B, Hp, Wp)).astype(F32)
        filtered = np.stack([NR.node_filter_conf(d[b], None, top, left, h, w, MAX_DISP, 0.0)[1] for b in range(B)])
        filtered[:, 0, :2] = 0  # invalid pixels under a ground truth
    conf = rng.uniform(-0.1, 1.1, (B, Hp, Wp)).astype(F32)
    conf[0, top, left] = np.nan
    conf[0, top + h - 1, left + w - 1] = 1.0  # 256 saturates to 255
    conf[:, :top], conf[:, :, :left] = 1e30, -1e30  # outside the window: never read
    # around the estimate, so that every row of the error table is hit; 0 = no ground truth; >= 192 * 256
    est = np.where(filtered > 0, filtered, 50)
    gt = est * rng.choice([1.0, 1.01, 1.05, 1.3, 2.0, 0.5, 0.1, 0.05], size=est.shape)
    gt = gt + rng.choice([0, 0.05, 0.3, 3, 20], size=est.shape)
    gt16 = np.clip(np.rint(gt * 256), 0, 65535).astype(np.uint16)
    gt16[rng.uniform(0, 1, gt16.shape) < 0.2] = 0
    gt16[rng.uniform(0, 1, gt16.shape) < 0.1] = rng.integers(192 * 256, 65536, dtype=np.uint16)
    gt16[:, 0, 0] = 40 * 256  # filtered == 0 here (first case) under a non-zero ground truth
    left_img = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    return filtered, conf, gt16, left_img, lut


def run_panels(name, filtered, conf, gt16, left_img, lut, want_gt=True):
    _, Hp, Wp, top, left, h, w = shape(name)
    B = filtered.shape[0]
    n = B * 2 * h * 2 * w * 3
    out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=DEV)  # the frame is exactly [B, 2h, 2w, 3]: no padding
    gt_f32 = torch.full((B, h, w), -3.0, device=DEV)
    work = torch.empty(E.range_workspace_bytes(B, h, w), dtype=torch.uint8, device=DEV)
    keep = [dev(filtered), dev(conf) if conf is not None else None, dev(gt16) if gt16 is not None else None,
            dev(left_img), dev(lut)]
    p = [t.data_ptr() if t is not None else None for t in keep]
    check(lib.esm_node_panels_u8(p[0], p[1], Hp, Wp, top, left, p[2], p[3], p[4], out.data_ptr(),
                                 gt_f32.data_ptr() if want_gt else None, work.data_ptr(), B, h, w, None), "node_panels")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[n:] == 0xA5).all()
    return o[:n].reshape(B, 2 * h, 2 * w, 3), gt_f32.cpu().numpy()


def ref_panels(name, filtered, conf, gt16, left_img, lut):
    _, Hp, Wp, top, left, h, w = shape(name)
    r = [NR.panels(filtered[b], None if conf is None else conf[b, top:top + h, left:left + w],
                   None if gt16 is None else gt16[b], left_img[b], lut) for b in range(filtered.shape[0])]
    return np.stack([x[0] for x in r]), np.stack([x[1] for x in r])


@pytest.mark.parametrize("with_conf", [True, False])
@pytest.mark.parametrize("with_gt", [True, False])
@pytest.mark.parametrize("name", ["node", "tiny"])
def test_panels_bit_exact(name, with_gt, with_conf):
    filtered, conf, gt16, left_img, lut = panel_inputs(name)
    conf, gt16 = (conf if with_conf else None), (gt16 if with_gt else None)
    frame, gt = run_panels(name, filtered, conf, gt16, left_img, lut)
    rframe, rgt = ref_panels(name, filtered, conf, gt16, left_img, lut)
    B, h, w = filtered.shape
    assert frame.shape == (B, 2 * h, 2 * w, 3)
    top_rows, bottom_rows, left_cols, right_cols = slice(0, h), slice(h, 2 * h), slice(0, w), slice(w, 2 * w)
    for panel, (ys, xs) in {"left": (top_rows, left_cols), "disparity": (bottom_rows, left_cols),
                            "error": (top_rows, right_cols), "confidence": (bottom_rows, right_cols)}.items():
        assert np.array_equal(frame[:, ys, xs], rframe[:, ys, xs]), panel
    assert np.array_equal(gt.view(np.uint32), rgt.view(np.uint32))
    assert np.array_equal(frame[:, :h, :w], left_img)
    if with_gt and name == "node":
        rows = NR.error_rows(filtered, rgt)
        assert set(np.unique(rows)) == set(range(-1, 10))  # every row of the table, and black
        assert (rgt[:, 0, 0] == 0).all() and (gt16[:, 0, 0] != 0).all()
    else:
        assert with_gt or not frame[:, :h, w:].any()
    assert with_conf or not frame[:, h:, w:].any()
    # gt_f32 is optional
    frame2, untouched = run_panels(name, filtered, conf, gt16, left_img, lut, want_gt=False)
    assert np.array_equal(frame2, rframe) and (untouched == -3.0).all()


@pytest.mark.parametrize("with_conf_and_gt", [True, False])
@pytest.mark.parametrize("name,partials", [("257-partials", 257), ("513-partials", 513)])
def test_panels_past_one_round_of_partials(name, partials, with_conf_and_gt):
    """One image of 3 x 175000 / 3 x 350003 pixels: 257 partial ranges (the panel kernel's fold takes a second round of
    256) and 513 (the first count whose range is folded by a separate launch, as test_gpu_render.py has it for
    esm_disp_colorize_u8).  Bit-equal to node_ref, every panel; the count is asserted, so that another tile size cannot
    move the case back into one round."""
    _, _, _, _, _, h, w = shape(name)
    per_partial = lib.esm_disp_colorize_workspace(1, 1, 1) // 2  # one partial and one folded record
    assert lib.esm_disp_colorize_workspace(1, h, w) // per_partial == partials + 1
    filtered, conf, gt16, left_img, lut = panel_inputs(name)
    conf, gt16 = (conf, gt16) if with_conf_and_gt else (None, None)
    # the image's extremes lie in partials that only a later round of a 256-wide fold reaches: the maximum in the last
    # one, the minimum in partial 256 (2048 pixels each, which the count above pins)
    flat = filtered[0].reshape(-1)
    flat[(flat > 190) | (flat < 1)] = 0
    flat[h * w - 5], flat[256 * 2048 + 7] = F32(191.75), F32(1 / 256)
    assert (h * w - 5) // 2048 == partials - 1 and flat.max() == F32(191.75) and flat[flat > 0].min() == F32(1 / 256)
    frame, gt = run_panels(name, filtered, conf, gt16, left_img, lut)
    rframe, rgt = ref_panels(name, filtered, conf, gt16, left_img, lut)
    upper, lower, left_cols, right_cols = slice(0, h), slice(h, 2 * h), slice(0, w), slice(w, 2 * w)
    for panel, (ys, xs) in {"left": (upper, left_cols), "disparity": (lower, left_cols),
                            "error": (upper, right_cols), "confidence": (lower, right_cols)}.items():
        assert np.array_equal(frame[:, ys, xs], rframe[:, ys, xs]), panel
    assert np.array_equal(gt.view(np.uint32), rgt.view(np.uint32))


@pytest.mark.parametrize("name", ["node", "tiny"])
def test_panels_empty_and_flat_range(name):
    filtered, conf, gt16, left_img, lut = panel_inputs(name, special=True)
    frame, gt = run_panels(name, filtered, conf, gt16, left_img, lut)
    rframe, rgt = ref_panels(name, filtered, conf, gt16, left_img, lut)
    assert np.array_equal(frame, rframe) and np.array_equal(gt, rgt)
    h, w = filtered.shape[1:]
    assert (frame[:, h:, :w] == lut[0]).all()  # DEFINED HERE: index 0 everywhere for both
    assert not gt[0].any() and not frame[0, :h, w:].any()


def test_panels_match_the_separate_entry_points():
    """The colour panel is ESM_COLORIZE_RANGE itself: the left column equals colorize_range(stack=left)."""
    filtered, conf, gt16, left_img, lut = panel_inputs("tiles")
    frame, _ = run_panels("tiles", filtered, conf, gt16, left_img, lut)
    rframe, _ = ref_panels("tiles", filtered, conf, gt16, left_img, lut)
    assert np.array_equal(frame, rframe)
    two = E.colorize_range(dev(filtered), dev(lut), stack=dev(left_img)).cpu().numpy()
    assert np.array_equal(frame[:, :, :filtered.shape[2]], two)


def test_results_do_not_depend_on_lds_leftovers():
    """Both kernels stage in LDS (the median's tile and halo; the colour table and the range): on a ragged shape the
    result is the same bits whatever the previous kernel left there (tests/lds_poison.py)."""
    name = "tiles"
    B, Hp, Wp, top, left, h, w = SHAPES[name]
    d, c = filter_inputs(name, 0.5)
    dd, cc = dev(d), dev(c)
    out = torch.empty(B, h, w, dtype=torch.int16, device=DEV)
    filt = torch.empty(B, h, w, device=DEV)
    valid = torch.empty(B, h, w, dtype=torch.uint8, device=DEV)
    assert_leftover_free(
        lambda: check(lib.esm_node_filter_conf_u16(dd.data_ptr(), cc.data_ptr(), out.data_ptr(), filt.data_ptr(),
                                                   valid.data_ptr(), B, Hp, Wp, top, left, h, w, MAX_DISP, 0.5, None),
                      "node_filter_conf"), [out, filt, valid], "node_filter_conf")
    filtered, conf, gt16, left_img, lut = panel_inputs(name)
    t = [dev(a) for a in (filtered, conf, gt16, left_img, lut)]
    frame = torch.empty(B, 2 * h, 2 * w, 3, dtype=torch.uint8, device=DEV)
    gt_f32 = torch.empty(B, h, w, device=DEV)
    work = torch.empty(E.range_workspace_bytes(B, h, w), dtype=torch.uint8, device=DEV)
    assert_leftover_free(
        lambda: check(lib.esm_node_panels_u8(t[0].data_ptr(), t[1].data_ptr(), Hp, Wp, top, left, t[2].data_ptr(),
                                             t[3].data_ptr(), t[4].data_ptr(), frame.data_ptr(), gt_f32.data_ptr(),
                                             work.data_ptr(), B, h, w, None), "node_panels"),
        [frame, gt_f32], "node_panels")


# ---- depth image -> disparity --------------------------------------------------------------------------------------

@pytest.mark.parametrize("src,dst", [((23, 37), (23, 37)), ((23, 37), (46, 74)), ((46, 74), (23, 37)),
                                     ((23, 37), (32, 64))])
def test_depth16_to_disparity_bit_exact(src, dst):
    rng = np.random.default_rng(src[0] + dst[1])
    d16 = rng.integers(1, 65536, (2,) + src, dtype=np.uint16)
    d16[rng.uniform(0, 1, d16.shape) < 0.1] = 0
    d16[0, 0, 0], d16[0, 0, 1], d16[1, -1, -1], d16[1, -1, -2] = 0, 65535, 65535, 0
    focal, baseline = 725.0087, 0.532725
    num = float(F32(focal) * F32(baseline))
    ref = NR.depth16_to_disp(d16, dst[0], dst[1], num)
    got = depth16_to_disparity(dev(d16), focal, baseline, size=dst)
    assert got.shape == (2,) + dst and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    if src == dst:
        assert np.array_equal(got.cpu().numpy(), NR.depth_to_disp(d16, num))
        one = depth16_to_disparity(dev(d16[0]), focal, baseline)  # [H, W], size = None
        assert one.shape == src and np.array_equal(one.cpu().numpy(), ref[0])
        assert got[0, 0, 0] == 0 and got[0, 0, 1] == num / (F32(65535) * F32(0.01))


# ---- the node, end to end ------------------------------------------------------------------------------------------

class DispOnly(torch.nn.Module):
    """The confidence model behind the plain node's signature."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, left, right):
        return self.model(left, right)[0]


def test_confidence_node_end_to_end():
    with open(os.path.join(GOLDEN_DIR, "manifest.json")) as f:
        m = json.load(f)["hot_S_gwc.npz"]
    model = E.ESMStereo_confidence(192, True, False, m["backbone"], m["cv_scale"], feature_cls=StubFeature)
    sd = seeded_state(load_spec(m["spec"]), m["seed"])
    sd.update({"confidence_net." + k: v for k, v in seeded_state(load_spec("spec_conf.json"), 77).items()})
    model.load_state_dict(sd)
    model = model.eval().to(DEV)
    H, W = 100, 220
    rng = np.random.default_rng(3)
    left = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    right = np.roll(left, -6, axis=1)
    node = ConfidenceNode(model, H, W, max_disp=MAX_DISP)
    # the model's own output on the node's input (the preprocessing is StereoNode's, checked in tests/test_node.py)
    x = [torch.from_numpy(np.ascontiguousarray(IO.node_preprocess(a))).unsqueeze(0).to(DEV) for a in (left, right)]
    with torch.no_grad():
        disp, conf = (t[0].cpu().numpy() for t in model(x[0], x[1]))
    assert disp.shape == conf.shape == (node.hp, node.wp)
    thr = float(np.median(conf[:H, :W]))  # a double that is a float32: pixels exactly at the threshold are valid
    open_u, open_m, _ = NR.node_filter_conf(disp, None, 0, 0, H, W, MAX_DISP, 0.0)
    gt = open_m * rng.choice([1.0, 1.02, 1.2, 0.7], size=open_m.shape) + rng.choice([0, 0.1, 2.0], size=open_m.shape)
    gt16 = np.clip(np.rint(gt * 256), 0, 65535).astype(np.uint16)
    gt16[rng.uniform(0, 1, gt16.shape) < 0.2] = 0
    gt16[rng.uniform(0, 1, gt16.shape) < 0.05] = 60000
    lut = E.colormap_lut("magma").cpu().numpy()

    def reference(threshold):
        u, filt, valid = NR.node_filter_conf(disp, conf, 0, 0, H, W, MAX_DISP, threshold)
        frame, gt_f32 = NR.panels(filt, conf[:H, :W], gt16, left, lut)
        return u, frame, NR.epe(gt_f32, filt), filt, valid

    u16, frame, epe, ms = node.process_scored(left, right, gt16, threshold=thr)
    assert torch.equal(node.net_in[0], x[0]) and torch.equal(node.net_in[1], x[1])
    ru, rframe, repe, rfilt, rvalid = reference(thr)
    assert u16.shape == (H, W) and u16.dtype == np.uint16 and ms > 0
    assert frame.shape == (2 * H, 2 * W, 3) and frame.dtype == np.uint8
    assert 0 < rvalid.sum() < (open_m > 0).sum()  # the gate decides pixels
    assert np.array_equal(u16, ru) and np.array_equal(frame, rframe)
    # the fp64 sum is exact in any order, so "to the last bit" holds whatever order the device adds in: gt is a multiple
    # of 2^-8 and every valid est a multiple of q = ulp(smallest valid est), so every |gt - est| is a multiple of q,
    # and the terms are non-negative, so every partial sum stays below the total T < 2^52 q
    q = float(np.spacing(rfilt[rfilt > 0].min()))
    total = float(np.abs(NR.masked_gt(rfilt, gt16) - rfilt).astype(np.float64).sum())
    print("epe", epe, repe, "q", q, "total", total)
    assert q <= 2.0 ** -8 and total < 2.0 ** 52 * q
    assert epe == repe and repe > 0
    assert node.epe_mean == epe
    # a second frame with another threshold: the running mean
    thr2 = float(np.quantile(conf[:H, :W], 0.25))
    u2, frame2, epe2, _ = node.process_scored(left, right, gt16, threshold=thr2)
    ru2, rframe2, repe2, _, _ = reference(thr2)
    assert np.array_equal(u2, ru2) and np.array_equal(frame2, rframe2) and epe2 == repe2
    assert node.frame_count == 2 and node.epe_mean == (epe + epe2) / 2
    # process: the same gate without the frame
    u3, _ = node.process(left, right, threshold=thr)
    assert np.array_equal(u3, ru)
    # threshold 0 lets every confidence through: the plain node's map; above 1 nothing passes
    plain, _ = StereoNode(DispOnly(model), H, W, max_disp=MAX_DISP).process(left, right)
    u0, _ = node.process(left, right, threshold=0.0)
    assert np.array_equal(u0, plain) and np.array_equal(u0, open_u) and u0.any()
    u_none, _ = node.process(left, right, threshold=1.5)
    assert not u_none.any()
    # the inherited two-panel picture is the gated map's
    u4, pic, _ = node.process_rendered(left, right)
    r4, filt4, _ = NR.node_filter_conf(disp, conf, 0, 0, H, W, MAX_DISP, 0.5)
    assert np.array_equal(u4, r4) and pic.shape == (2 * H, W, 3) and np.array_equal(pic[:H], left)
