"""The device JPEG encoder (csrc/jpeg.hip) against tests/jpeg_ref.py: the same bytes, lengths included.

jpeg_ref is the definition of include/esmstereo_amd.h one bit at a time (pinned by test_jpeg_host.py's anchors and
PIL), so equality with it checks the colour conversion, the padding, both DCT passes, the quantisation, every code,
every run, the DC chains, the restart markers' positions and indices, the byte stuffing and the offsets of every
interval at once.  Shapes are the smallest that can go wrong: one pixel, exactly one MCU, sizes that are no multiple
of the MCU in either direction, several MCU rows, intervals that straddle rows, more than 8 intervals (the marker
index wraps), fewer MCUs than Ri.

LDS, in tests/lds_poison.py's terms: like png.hip the kernel keeps OFFSETS in LDS (the blocks' bit counts become
indices into the staging buffer) and ORs its bits into a staging buffer, so a leftover word would be a wild index or
stray bits.  It writes every such word before it reads it and zeroes the staging it uses; ``test_lds_leftovers`` runs a
multi-interval B = 2 encode behind both poison patterns and asserts the same bytes.
"""
import functools
import io as _io

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

import jpeg_ref  # noqa: E402
import lds_poison  # noqa: E402
from esmstereo_amd import _lib, render  # noqa: E402
from esmstereo_amd.video import MjpegWriter  # noqa: E402

lib = _lib.lib
DEV = torch.device("cuda")
SIZES = ((1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (37, 50), (33, 129), (48, 64))


@functools.lru_cache(maxsize=None)
def picture(kind: str, h: int, w: int) -> np.ndarray:
    """uint8 [h, w, 3] in the stored channel order (the tests choose what that order means)."""
    if kind == "ramp":
        a = jpeg_ref.anchor_picture(h, w)
    elif kind == "noise":
        a = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "zero":
        a = np.zeros((h, w, 3), dtype=np.uint8)
    elif kind == "white":
        a = np.full((h, w, 3), 255, dtype=np.uint8)
    elif kind == "checker":  # 0 / 255 per pixel: the largest high-frequency coefficients
        y, x = np.mgrid[0:h, 0:w]
        a = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    elif kind == "basis":  # every DCT basis function's sign pattern and its negative, one per 8 x 8 block
        a = np.zeros((64, 128, 3), dtype=np.uint8)
        for k in range(64):
            v, u = divmod(k, 8)
            a[8 * v:8 * v + 8, 8 * u:8 * u + 8] = jpeg_ref.basis_sign_picture(k)
            a[8 * v:8 * v + 8, 64 + 8 * u:64 + 8 * u + 8] = 255 - jpeg_ref.basis_sign_picture(k)
    else:
        raise KeyError(kind)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(kind: str, h: int, w: int, quality: int, sub: int, ri: int, order: str) -> bytes:
    return jpeg_ref.encode(picture(kind, h, w), quality, sub, ri, order)


def check(kinds, h, w, quality=75, sub=420, ri=8, order="bgr"):
    """One batch of len(kinds) different pictures: files and lengths equal the reference, twice."""
    a = np.stack([picture(k, h, w) for k in kinds])
    t = torch.from_numpy(a.copy()).to(DEV)
    enc = render.JpegEncoder(len(kinds), h, w, quality, str(sub), ri)
    files = enc.encode(t, order)
    assert len(files) == len(kinds)
    for b, kind in enumerate(kinds):
        ref = reference(kind, h, w, quality, sub, ri, order)
        assert int(enc.host_lengths[b]) == len(ref) - 629, (kind, int(enc.host_lengths[b]), len(ref) - 629)
        assert files[b] == ref, f"{kind} {h}x{w} q{quality} {sub} Ri {ri} {order}: the bytes differ from jpeg_ref"
    assert enc.encode(t, order) == files, "the bytes differ between two calls"
    return files


@pytest.mark.parametrize("order", ("bgr", "rgb"))
@pytest.mark.parametrize("sub", (420, 444))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes(size, sub, order):
    check(("ramp", "noise"), *size, sub=sub, order=order)  # B = 2: own offsets, length and slot each


@pytest.mark.parametrize("sub", (420, 444))
@pytest.mark.parametrize("ri", (1, 3, 8, 16))
def test_restart_intervals(ri, sub):
    check(("ramp", "noise"), 33, 129, sub=sub, ri=ri)  # 9 (420) / 17 (444) MCUs per row: intervals straddle rows
    check(("noise", "ramp"), 37, 50, sub=sub, ri=ri)   # Ri = 1 at 420: 12 intervals, RST7 is followed by RST0
    check(("ramp",), 16, 16, sub=sub, ri=ri)           # 1 (420) / 4 (444) MCUs: at Ri = 8, 16 one interval, no marker


def test_marker_sequence():
    """The restart markers of 37 x 50 at 420 / Ri = 1, read back from the device's own bytes: D0 .. D7, D0, D1, D2."""
    data = check(("noise",), 37, 50, ri=1)[0][629:]
    marks = [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and data[i + 1] not in (0x00, 0xFF)]
    assert marks == [0xD0 + (k & 7) for k in range(11)] + [0xD9]


@pytest.mark.parametrize("sub", (420, 444))
@pytest.mark.parametrize("kind", ("ramp", "noise", "zero", "white"))
def test_contents(kind, sub):
    check((kind, "noise"), 37, 50, sub=sub, ri=3)
    check((kind,), 37, 50, quality=100, sub=sub, ri=3)
    check((kind,), 37, 50, quality=1, sub=sub, ri=3)


@pytest.mark.parametrize("sub", (420, 444))
def test_checkerboard_and_basis_patterns_at_quality_100(sub):
    """Q = 1 everywhere: the largest values a coefficient can take (DC -1024, AC up to 1020: sizes 11 and 10), long
    codes and many 0xFF bytes.  The AC guard of +-1023 is not reached by any of them (jpeg_ref records a hit)."""
    check(("checker", "noise"), 37, 50, quality=100, sub=sub)
    check(("basis",), 64, 128, quality=100, sub=sub, ri=5)
    hits = []
    jpeg_ref.encode_scan(picture("basis", 64, 128), 100, sub, 5, hits)
    assert hits == []
    Image = pytest.importorskip("PIL.Image")
    got = np.asarray(Image.open(_io.BytesIO(reference("basis", 64, 128, 100, sub, 5, "bgr"))).convert("RGB"))
    assert np.abs(got.astype(int) - picture("basis", 64, 128)[:, :, ::-1]).max() <= 8


def scan_bytes(kind, h, w, quality, sub, ri, order="bgr") -> bytes:
    return reference(kind, h, w, quality, sub, ri, order)[629:]


@pytest.mark.parametrize("fill", (0x00, 0xFF))
def test_prefilled_buffers_and_neighbouring_slot(fill):
    """Slots, workspace and lengths hold `fill` before the call: the same bytes either way, nothing behind a scan's
    length, nothing in the slot of an image that was not encoded."""
    h, w = 37, 50
    a = torch.from_numpy(np.stack([picture("ramp", h, w), picture("noise", h, w)])).to(DEV)
    enc = render.JpegEncoder(2, h, w, 75, "420", 3)
    for n in (1, 2):
        enc.out.fill_(fill)
        enc.work.fill_(fill)
        enc.lengths.fill_(-7)
        files = enc.encode(a[:n], "bgr")
        out = enc.out.cpu().numpy()
        for b, kind in enumerate(("ramp", "noise")[:n]):
            ref = scan_bytes(kind, h, w, 75, 420, 3)
            assert files[b][629:] == ref and int(enc.lengths[b]) == len(ref)
            assert out[b, :len(ref)].tobytes() == ref
            assert (out[b, len(ref):] == fill).all(), "bytes behind the scan were written"
        for b in range(n, 2):
            assert (out[b] == fill).all(), "the slot of an image that was not encoded was written"
            assert int(enc.lengths[b]) == -7


def test_overflow_reports_the_need_and_the_encoder_retries():
    """48 x 64 noise at quality 100 / 444: a scan longer than the raw frame (the default slot)."""
    h, w, raw = 48, 64, 3 * 48 * 64
    ref = scan_bytes("noise", h, w, 100, 444, 8)
    assert len(ref) > raw
    a = torch.from_numpy(picture("noise", h, w).copy()).to(DEV)
    out = torch.full((2, raw), 0xA5, dtype=torch.uint8, device=DEV)  # slot 1: the poisoned neighbour
    lengths = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    work = torch.empty(lib.esm_jpeg_workspace_bytes(1, h, w, 444, 8), dtype=torch.uint8, device=DEV)
    _lib.check(lib.esm_jpeg_encode_rgb8(a.data_ptr(), 1, h, w, 1, 100, 444, 8, work.data_ptr(), out.data_ptr(), raw,
                                        lengths.data_ptr(), None), "jpeg_encode_rgb8")
    torch.cuda.synchronize()
    assert lengths.tolist() == [-len(ref), -7]
    got = out.cpu().numpy()
    assert (got[1] == 0xA5).all(), "the neighbouring slot was written"
    assert got[0].tobytes() == ref[:raw]  # the truncated scan: what fits, in place
    enc = render.JpegEncoder(1, h, w, 100, "444", 8)
    assert enc.slot == raw
    assert enc.encode(a, "bgr") == [reference("noise", h, w, 100, 444, 8, "bgr")]
    assert enc.slot == lib.esm_jpeg_stream_bound(h, w, 444, 8) >= len(ref)
    assert enc.encode(a, "bgr") == [reference("noise", h, w, 100, 444, 8, "bgr")]  # the kept slot: no retry needed


def check_lds_leftovers(h, w, sub, ri):
    """A B = 2 encode behind poisoned LDS (see the module docstring): same lengths, same bytes."""
    a = torch.from_numpy(np.stack([picture("ramp", h, w), picture("noise", h, w)])).to(DEV)
    enc = render.JpegEncoder(2, h, w, 75, str(sub), ri)
    enc.out.fill_(0xFF)
    enc.lengths.fill_(-1)
    stream = render._stream(enc.work)

    def launch():
        _lib.check(lib.esm_jpeg_encode_rgb8(a.data_ptr(), 2, h, w, 1, 75, sub, ri, enc.work.data_ptr(),
                                            enc.out.data_ptr(), enc.slot, enc.lengths.data_ptr(), stream),
                   "jpeg_encode_rgb8")

    def outputs():  # the lengths and each scan up to its length; then spoil both again, so that a launch that stored
        n = enc.lengths.clone()  # nothing cannot leave "the same bytes"
        keep = torch.arange(enc.slot, device=DEV)[None, :] < n[:, None]
        scans = torch.where(keep, enc.out, torch.zeros_like(enc.out))
        enc.out.fill_(0xFF)
        enc.lengths.fill_(-1)
        return [n, scans]

    lds_poison.assert_leftover_free(launch, outputs, "jpeg_encode_rgb8")
    assert enc.encode(a, "bgr") == [reference(k, h, w, 75, sub, ri, "bgr") for k in ("ramp", "noise")]


@pytest.mark.parametrize("sub", (420, 444))
def test_lds_leftovers(sub):
    check_lds_leftovers(37, 50, sub, 3)  # several intervals


def test_mjpeg_writer_takes_the_nodes_frame(tmp_path):
    """MjpegWriter.write(node.dev_frame) after StereoNode.process_rendered: the AVI's frame is jpeg_encode_bgr8 of
    the same tensor, which is jpeg_ref's file of the frame the node returned."""
    import json
    import os
    import esmstereo_amd as E
    from esmstereo_amd.backbone import StubFeature
    from esmstereo_amd.node import StereoNode
    from helpers import GOLDEN_DIR, load_spec, seeded_state
    with open(os.path.join(GOLDEN_DIR, "manifest.json")) as f:
        m = json.load(f)["hot_S_gwc.npz"]
    model = E.ESMStereo_trt(192, True, False, m["backbone"], 16, feature_cls=StubFeature)
    model.load_state_dict(seeded_state(load_spec(m["spec"]), m["seed"]))
    model = model.eval().to(DEV)
    H, W = 37, 70
    rng = np.random.default_rng(2)
    left = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    right = np.roll(left, -6, axis=1)
    node = StereoNode(model, H, W, max_disp=192.0)
    path = str(tmp_path / "node.avi")
    with MjpegWriter(path, fps=10, quality=90) as wr:
        _, frame, _ = node.process_rendered(left, right)
        wr.write(node.dev_frame)
        expect = render.jpeg_encode_bgr8(node.dev_frame, quality=90)[0]
        _, frame_b, _ = node.process_rendered(right, left)
        wr.write(node.dev_frame)
        with pytest.raises(ValueError, match="frames"):
            wr.write(node.dev_frame[:-1])
    assert expect == jpeg_ref.encode(frame, 90, 420, 8, "bgr")
    data = open(path, "rb").read()
    tree = jpeg_ref.riff_walk(data)
    chunks = jpeg_ref.riff_find(tree, b"LIST:movi")[3]
    assert [c[0] for c in chunks] == [b"00dc", b"00dc"]
    assert data[chunks[0][1]:chunks[0][1] + chunks[0][2]] == expect
    assert data[chunks[1][1]:chunks[1][1] + chunks[1][2]] == jpeg_ref.encode(frame_b, 90, 420, 8, "bgr")
    Image = pytest.importorskip("PIL.Image")
    got = np.asarray(Image.open(_io.BytesIO(expect)).convert("RGB"))
    assert got.shape == (2 * H, W, 3)


def test_cpu_tensor_raises(tmp_path):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.jpeg_encode_bgr8(torch.zeros(4, 5, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.JpegEncoder(1, 4, 5).encode(torch.zeros(1, 4, 5, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.JpegEncoder(1, 4, 5, device="cpu")
    with MjpegWriter(str(tmp_path / "a.avi")) as wr:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            wr.write(torch.zeros(4, 5, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="frames of"):
        render.JpegEncoder(1, 4, 5).encode(torch.zeros(1, 4, 6, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="subsampling"):
        render.JpegEncoder(1, 4, 5, subsampling="422")
