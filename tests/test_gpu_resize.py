"""GPU tests of the resizing nodes' front end (csrc/resize.hip, esmstereo_amd/io.py, esmstereo_amd.node.ResizeNode):
every comparison is bit for bit against the numpy restatement (tests/resize_ref.py).

Every output is written inside a larger poisoned buffer, at an aligned and at a misaligned offset (the dword and
16-byte stores and their byte / scalar fallbacks), and the surroundings are checked afterwards.  The kernels use no
LDS, so there is no leftover test here (tests/lds_poison.py is for kernels that stage there)."""
import json
import os

import numpy as np
import pytest
import torch

import node_ref as NR
import resize_ref as RZ
from helpers import GOLDEN_DIR, load_spec, seeded_state

pytestmark = pytest.mark.gpu

import esmstereo_amd as E  # noqa: E402
from esmstereo_amd._lib import c_float, check, lib  # noqa: E402
from esmstereo_amd.backbone import StubFeature  # noqa: E402
from esmstereo_amd.io import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from esmstereo_amd.node import ResizeNode  # noqa: E402

DEV = torch.device("cuda")
F32 = np.float32
B = 2
#         source      destination   what it reaches
SHAPES = [((23, 37), (23, 37)),   # identity
          ((23, 37), (32, 64)),   # up both ways
          ((75, 131), (32, 64)),  # down by more than 2: taps skip pixels
          ((20, 150), (32, 64)),  # up in y, down in x: the virtual-KITTI case
          ((46, 74), (23, 37)),   # exact 2x down, odd widths, tails
          ((1, 5), (7, 9)),       # one source row: both clamps
          ((5, 1), (9, 7)),       # one source column: both clamps
          ((64, 37), (32, 37))]   # the node's squeeze
IDS = ["%dx%d-%dx%d" % (s + d) for s, d in SHAPES]
CONSTANTS = {"imagenet": (IMAGENET_MEAN, IMAGENET_STD), "ess": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))}
POISON_U8, POISON_F32 = 0xA5, -7.0
U8_OFFSETS, F32_OFFSETS = (64, 61), (16, 3)  # elements in front of the output: aligned, and not


def inputs(h, w, c):
    """{kind: uint8 [B, h, w, c]}: random bytes, an all-255 image, a 0 / 255 checkerboard and its inverse."""
    rng = np.random.default_rng(1000 * h + 10 * w + c)
    yy, xx = np.mgrid[:h, :w]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], c, axis=-1)
    return {"random": rng.integers(0, 256, (B, h, w, c), dtype=np.uint8),
            "white": np.full((B, h, w, c), 255, np.uint8), "board": np.stack([board, 255 - board])}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n, offset, dtype, poison):
    """A poisoned buffer with n elements of output at `offset`: (buffer, the output's address)."""
    buf = torch.full((offset + n + 64,), poison, dtype=dtype, device=DEV)
    return buf, buf.data_ptr() + offset * buf.element_size()


def take(buf, n, offset, poison):
    """The n output elements; the elements around them still hold the poison."""
    a = buf.cpu().numpy()
    assert (a[:offset] == poison).all() and (a[offset + n:] == poison).all(), "wrote outside the output"
    return a[offset:offset + n]


def run_resize(img, H, W, offset=64):
    b, hs, ws, c = img.shape
    n = b * H * W * c
    src = dev(img)
    buf, ptr = guarded(n, offset, torch.uint8, POISON_U8)
    check(lib.esm_resize_u8(src.data_ptr(), ptr, b, hs, ws, H, W, c, None), "resize_u8")
    torch.cuda.synchronize()
    return take(buf, n, offset, POISON_U8).reshape(b, H, W, c)


def run_preprocess(img, H, W, mean, std, want_resized, off_u8=64, off_f32=16):
    b, hs, ws, _ = img.shape
    n = b * H * W * 3
    src = dev(img)
    out_buf, out_ptr = guarded(n, off_f32, torch.float32, POISON_F32)
    res_buf, res_ptr = guarded(n, off_u8, torch.uint8, POISON_U8)
    m, s = (c_float * 3)(*mean), (c_float * 3)(*std)
    check(lib.esm_preprocess_resize_u8(src.data_ptr(), out_ptr, res_ptr if want_resized else None, b, hs, ws, H, W, m,
                                       s, None), "preprocess_resize_u8")
    torch.cuda.synchronize()
    out = take(out_buf, n, off_f32, F32(POISON_F32)).reshape(b, 3, H, W)
    res = res_buf.cpu().numpy()
    if not want_resized:
        assert (res == POISON_U8).all()
        return out, None
    return out, take(res_buf, n, off_u8, POISON_U8).reshape(b, H, W, 3)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_resize_u8_bit_exact(src, dst, c):
    for kind, img in inputs(*src, c).items():
        ref = RZ.resize_u8(img, *dst)
        for offset in U8_OFFSETS:
            got = run_resize(img, *dst, offset=offset)
            assert got.shape == (B,) + dst + (c,) and np.array_equal(got, ref), (kind, offset)
        if src == dst:
            assert np.array_equal(ref, img)
        if kind == "white":
            assert (ref == 255).all()


@pytest.mark.parametrize("constants", list(CONSTANTS))
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_preprocess_resize_bit_exact(src, dst, constants):
    mean, std = CONSTANTS[constants]
    for kind, img in inputs(*src, 3).items():
        ref_out, ref_res = RZ.preprocess_resize(img, *dst, mean, std)
        bytes_alone = run_resize(img, *dst)
        for off_u8, off_f32 in zip(U8_OFFSETS, F32_OFFSETS):
            for want_resized in (True, False):
                out, res = run_preprocess(img, *dst, mean, std, want_resized, off_u8, off_f32)
                assert out.dtype == F32 and np.array_equal(out.view(np.uint32), ref_out.view(np.uint32)), kind
                if want_resized:
                    assert np.array_equal(res, ref_res) and np.array_equal(res, bytes_alone), kind


@pytest.mark.parametrize("size", [(23, 37), (32, 64), (128, 224)])
def test_identity_size_equals_preprocess_u8(size):
    """Hs == H, Ws == W with the ImageNet constants: esm_preprocess_u8 on the same bytes with no padding."""
    H, W = size
    img = inputs(H, W, 3)["random"]
    out, res = run_preprocess(img, H, W, IMAGENET_MEAN, IMAGENET_STD, True)
    src = dev(img)
    plain = torch.empty(B, 3, H, W, device=DEV)
    check(lib.esm_preprocess_u8(src.data_ptr(), plain.data_ptr(), B, H, W, H, W, 0, 0, 1, None), "preprocess")
    torch.cuda.synchronize()
    assert np.array_equal(out.view(np.uint32), plain.cpu().numpy().view(np.uint32)) and np.array_equal(res, img)
    # the same through the Python front, against plain numpy
    front, front_res = E.resize_preprocess(src, size, return_resized=True)
    want = (img.astype(F32) / F32(255) - np.asarray(IMAGENET_MEAN, F32)) / np.asarray(IMAGENET_STD, F32)
    assert front.shape == (B, 3, H, W) and front.dtype == torch.float32
    assert np.array_equal(front.cpu().numpy().view(np.uint32), want.transpose(0, 3, 1, 2).view(np.uint32).copy())
    assert np.array_equal(front_res.cpu().numpy(), img)


def test_python_fronts_ranks_views_and_devices():
    src, dst = (20, 150), (32, 64)
    img = inputs(*src, 3)["random"]
    ref = RZ.resize_u8(img, *dst)
    grey_ref = RZ.resize_grey(img[..., 0], *dst)
    t = dev(img)
    # [B, H, W, 3], [H, W, 3], [B, H, W], [H, W]
    for got, want in ((E.resize_u8(t, dst), ref), (E.resize_u8(t[0], dst), ref[0]),
                      (E.resize_u8(dev(img[..., 0]), dst), grey_ref),
                      (E.resize_u8(dev(img[0, ..., 0]), dst), grey_ref[0])):
        assert got.dtype == torch.uint8 and got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)
    ref_out, ref_res = RZ.preprocess_resize(img, *dst, IMAGENET_MEAN, IMAGENET_STD)
    out = E.resize_preprocess(t, dst)
    one, one_res = E.resize_preprocess(t[1], dst, return_resized=True)
    assert isinstance(out, torch.Tensor) and out.shape == (B, 3) + dst and one.shape == (1, 3) + dst
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref_out.view(np.uint32))
    assert np.array_equal(one.cpu().numpy(), ref_out[1:2]) and np.array_equal(one_res.cpu().numpy(), ref_res[1:2])
    ess = E.resize_preprocess(t, dst, mean=(0, 0, 0), std=(1, 1, 1))
    assert np.array_equal(ess.cpu().numpy(), RZ.normalize(ref_res, (0, 0, 0), (1, 1, 1)))
    # a non-contiguous view equals its contiguous copy: a channel-reversed view (BGR of RGB), a strided grey view
    bgr = t.flip(-1)
    view = t[:, ::2, 1::3]
    grey = t[..., 1]
    assert not view.is_contiguous() and not grey.is_contiguous()
    assert torch.equal(E.resize_u8(view, dst), E.resize_u8(view.contiguous(), dst))
    assert np.array_equal(E.resize_u8(view, dst).cpu().numpy(), RZ.resize_u8(img[:, ::2, 1::3], *dst))
    assert np.array_equal(E.resize_u8(grey, dst).cpu().numpy(), RZ.resize_grey(img[..., 1], *dst))
    assert np.array_equal(E.resize_u8(bgr, dst).cpu().numpy(), ref[..., ::-1])
    assert torch.equal(E.resize_preprocess(view, dst), E.resize_preprocess(view.contiguous(), dst))
    # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.resize_u8(t.cpu(), dst)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.resize_preprocess(t.cpu(), dst)
    with pytest.raises(ValueError):
        E.resize_u8(t.float(), dst)
    with pytest.raises(ValueError):
        E.resize_preprocess(t[..., 0], dst)


# ---- the node, end to end ------------------------------------------------------------------------------------------

MAX_DISP = 192.0
CAM, NET = (100, 220), (128, 224)
FOCAL, BASELINE = 725.0087, 0.532725


@pytest.fixture(scope="module")
def model():
    with open(os.path.join(GOLDEN_DIR, "manifest.json")) as f:
        m = json.load(f)["hot_S_gwc.npz"]
    net = E.ESMStereo_trt(192, True, False, m["backbone"], m["cv_scale"], feature_cls=StubFeature)
    net.load_state_dict(seeded_state(load_spec(m["spec"]), m["seed"]))
    return net.eval().to(DEV)


def test_resize_node_end_to_end(model):
    (H, W), (Hn, Wn) = CAM, NET
    rng = np.random.default_rng(4)
    left = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    right = np.roll(left, -6, axis=1)
    num = float(F32(FOCAL) * F32(BASELINE))
    lut = E.colormap_lut("magma").cpu().numpy()
    node = ResizeNode(model, H, W, Hn, Wn, max_disp=MAX_DISP)

    # the restatement: the resized input, the model's own output on it, the filter, the picture, the score
    x, resized = zip(*(RZ.preprocess_resize(a, Hn, Wn, IMAGENET_MEAN, IMAGENET_STD) for a in (left, right)))
    xt = [torch.from_numpy(a).unsqueeze(0).to(DEV) for a in x]
    with torch.no_grad():
        disp = model(xt[0], xt[1])[0].cpu().numpy()
    assert disp.shape == (Hn, Wn)
    ru, rfilt, rvalid = NR.node_filter_conf(disp, None, 0, 0, Hn, Wn, MAX_DISP, 0.0)
    rframe = RZ.stack_and_squeeze(resized[0], rfilt, lut)
    # a random 16-bit depth image, 10 % of it zeros: disparities on both sides of 192; on half of the pixels the depth
    # of the estimate itself (sampled at the camera size), so that some pixels score as good
    depth16 = rng.integers(150, 20000, (H, W), dtype=np.uint16)
    est_cam = rfilt[(np.arange(H) * Hn // H)[:, None], (np.arange(W) * Wn // W)[None, :]]
    near = (est_cam > 0) & (rng.uniform(0, 1, (H, W)) < 0.5)
    depth16[near] = np.clip(np.rint(num / (est_cam[near].astype(np.float64) * 0.01)), 1, 65535).astype(np.uint16)
    depth16[rng.uniform(0, 1, (H, W)) < 0.1] = 0
    gt = NR.depth16_to_disp(depth16, Hn, Wn, num)
    repe, rd1, rn, rbad = RZ.score(gt, rfilt)
    assert rvalid.any() and 0 < rbad < rn < Hn * Wn and ((gt >= 192) | (gt == 0)).any()

    u16, frame, epe, d1, ms = node.process_scored(left, right, depth16, FOCAL, BASELINE)
    # input
    assert torch.equal(node.net_in[0].view(torch.int32), xt[0].view(torch.int32))
    assert torch.equal(node.net_in[1].view(torch.int32), xt[1].view(torch.int32))
    # disparity
    assert u16.shape == (Hn, Wn) and u16.dtype == np.uint16 and ms > 0 and np.array_equal(u16, ru)
    # frame
    assert frame.shape == (Hn, Wn, 3) and frame.dtype == np.uint8 and np.array_equal(frame, rframe)
    assert np.array_equal(node.dev_left.cpu().numpy(), resized[0])
    # ground truth and score: the counts exactly, epe to 1e-12 (the fp64 summation order is the device's)
    assert np.array_equal(node.gt_f32.cpu().numpy().view(np.uint32), gt.view(np.uint32))
    rec = node.host_records.numpy()[0]
    print("epe", epe, repe, "d1", d1, rd1, "valid", rec[0], rn, "bad", rec[8], rbad)
    assert rec[0] == rn and rec[8] == rbad
    assert d1 == rd1 and abs(epe - repe) <= 1e-12 * repe and repe > 0
    assert node.frame_count == 1 and node.epe_mean == epe

    # a second frame: the running mean
    left2, right2 = right, left
    x2 = [torch.from_numpy(RZ.preprocess_resize(a, Hn, Wn, IMAGENET_MEAN, IMAGENET_STD)[0]).unsqueeze(0).to(DEV)
          for a in (left2, right2)]
    with torch.no_grad():
        disp2 = model(x2[0], x2[1])[0].cpu().numpy()
    ru2, rfilt2, _ = NR.node_filter_conf(disp2, None, 0, 0, Hn, Wn, MAX_DISP, 0.0)
    repe2, rd12, _, _ = RZ.score(gt, rfilt2)
    u2, frame2, epe2, d12, _ = node.process_scored(left2, right2, depth16, FOCAL, BASELINE)
    assert np.array_equal(u2, ru2) and d12 == rd12 and abs(epe2 - repe2) <= 1e-12 * max(repe2, 1e-300)
    assert np.array_equal(frame2, RZ.stack_and_squeeze(RZ.resize_u8(left2, Hn, Wn), rfilt2, lut))
    assert node.frame_count == 2 and node.epe_mean == (epe + epe2) / 2

    # process and process_rendered: the same map, the same picture; the loop form
    u3, _ = node.process(left, right)
    u4, pic, _ = node.process_rendered(left, right)
    assert np.array_equal(u3, ru) and np.array_equal(u4, ru) and np.array_equal(pic, rframe)
    outs = list(node.run([(left, right), (left2, right2)]))
    assert len(outs) == 2 and np.array_equal(outs[0][0], ru) and np.array_equal(outs[1][0], ru2)
    assert node.frame_count == 2  # only process_scored counts

    # wrong sizes
    with pytest.raises(ValueError):
        node.process(left[:-1], right[:-1])
    with pytest.raises(ValueError):
        node.process_rendered(left, right[:, :-1])
    with pytest.raises(ValueError):
        node.process_scored(left, right, depth16[:-1], FOCAL, BASELINE)
    with pytest.raises(ValueError):
        node.process_scored(left, right, depth16.astype(np.int32), FOCAL, BASELINE)


def test_resize_node_at_the_network_size_and_ess_constants(model):
    """Camera size == network size: net_in is esm_preprocess_u8's unpadded output; mean 0 / std 1 is the ESS node."""
    Hn, Wn = NET
    rng = np.random.default_rng(6)
    left = rng.integers(0, 256, (Hn, Wn, 3), dtype=np.uint8)
    right = np.roll(left, -4, axis=1)
    node = ResizeNode(model, Hn, Wn, Hn, Wn, max_disp=MAX_DISP)
    u16, frame, _ = node.process_rendered(left, right)
    src = dev(np.stack([left, right]))
    plain = torch.empty(2, 3, Hn, Wn, device=DEV)
    check(lib.esm_preprocess_u8(src.data_ptr(), plain.data_ptr(), 2, Hn, Wn, Hn, Wn, 0, 0, 1, None), "preprocess")
    torch.cuda.synchronize()
    assert torch.equal(node.net_in[:, 0].view(torch.int32), plain.view(torch.int32))
    assert u16.shape == (Hn, Wn) and np.array_equal(node.dev_left.cpu().numpy(), left)
    assert np.array_equal(frame[:Hn // 2], RZ.resize_u8(left, Hn // 2, Wn))  # the top panel, squeezed
    ess = ResizeNode(model, 100, 220, Hn, Wn, mean=(0, 0, 0), std=(1, 1, 1))
    ess.process(left[:100, :220], right[:100, :220])
    want = RZ.preprocess_resize(left[:100, :220], Hn, Wn, (0, 0, 0), (1, 1, 1))[0]
    assert np.array_equal(ess.net_in[0, 0].cpu().numpy().view(np.uint32), want.view(np.uint32))
