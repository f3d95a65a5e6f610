"""GPU tests of the rendering kernels (csrc/render.hip) and their Python front (esmstereo_amd/render.py, the node's
process_rendered) against the numpy restatement tests/render_ref.py.  Every comparison is bit-equal: uint8 frames
with np.array_equal, the depth map on fp32 bit patterns (every NaN one pattern).

Shapes: one pixel; 1 x 3 x 5 (every group crosses a row's end); 2 x 7 x 13 as a window at odd offsets inside a
2 x 16 x 24 map of NaN; 3 x 67 x 131 (five workgroups and partial ranges per image, a different range per image, image
0 without a valid pixel, image 1 with all valid pixels equal); 1 x 1024 x 1024 and 2 x 3 x 350003 (512 and 513
partial ranges per image: the last size the render pass folds itself and the first that takes the separate fold)."""
import ctypes

import numpy as np
import pytest
import torch

import render_ref as RR

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = torch.device("cuda")
NUM, MAX_DEPTH = F32(0.05 * 640), 5.0
BASELINE, FOCAL = 0.05, 640
MODES = ("scale", "range", "depth")
# ties of the SCALE index (u = 50, 150, 250, 350), its saturation (u = 25550, 300 px), the 16-bit wrap (256 px, a
# negative value), and what the clips and the valid mask have to handle
PLANTS = [50 / 256, 150 / 256, 250 / 256, 350 / 256, 25550 / 256, -2.0, 0.0, np.nan, 1e-3, 3.3, -1 / 256, -0.0]
# in a batch's first image only (they would pin every image's range to the 16-bit maximum)
WILD = [np.inf, 300.0, 256.0, -np.inf, 65535 / 256, 1e9]


def make(B, H, W, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0, 200, (B, H, W)).astype(F32)
    d[rng.uniform(size=d.shape) < 0.2] = 0  # the node's invalid pixels
    for b in range(B):  # a different range per image
        d[b] *= F32(1.0 / (b + 1))
        flat = d[b].reshape(-1)
        plants = np.asarray(PLANTS[:9] + WILD[:3] + PLANTS[9:] + WILD[3:] if b == 0 else PLANTS, F32)
        pos = rng.permutation(flat.size)[:len(plants)]
        flat[pos] = plants[:len(pos)]
    return d


def make_cases():
    cases = {"1x1x1": np.full((1, 1, 1), 150 / 256, F32), "1x3x5": make(1, 3, 5, 1), "2x7x13": make(2, 7, 13, 2),
             "3x67x131": make(3, 67, 131, 3), "1x1024x1024": make(1, 1024, 1024, 4),
             "2x3x350003": make(2, 3, 350003, 5)}
    d = cases["3x67x131"]
    d[0] = np.where(d[0] > 0, -d[0], d[0])          # image 0: no valid pixel (negatives, zeros, NaN, -inf)
    d[1] = np.where(d[1] > 0, F32(7.25), d[1])      # image 1: all valid pixels equal
    assert not (d[0] > 0).any() and (d[1] > 0).sum() > 1000 and len(np.unique(d[2][d[2] > 0])) > 1000
    return cases


CASES = make_cases()
RNG = np.random.default_rng(99)
LUT = RNG.integers(0, 256, (256, 3), dtype=np.uint8)
_REFS = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def frames(name):
    B, H, W = CASES[name].shape
    return np.random.default_rng(B * H * W).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def ref(name, mode, stacked, lut=LUT):
    """The restatement's frame, computed once per (case, mode) and left unchanged."""
    key = (name, mode, lut.tobytes())
    if key not in _REFS:
        _REFS[key] = RR.render(CASES[name], lut, mode, None, 0.01, NUM, MAX_DEPTH)
        _REFS[key].setflags(write=False)
    img = _REFS[key]
    return RR.stack(frames(name), img) if stacked else img


def run(mode, d, lut, top=None):
    from esmstereo_amd import render as R
    if mode == "scale":
        return R.colorize_disparity(d, lut, 0.01, stack=top)
    if mode == "range":
        return R.colorize_range(d, lut, stack=top)
    return R.colorize_depth(d, BASELINE, FOCAL, MAX_DEPTH, lut, stack=top)


def embed(a, H, W, top, left):
    """`a` [B, h, w] as the window (top, left) of a [B, H, W] device tensor of NaN: a view, not a copy."""
    big = torch.full((a.shape[0], H, W), float("nan"), device=DEV)
    big[:, top:top + a.shape[1], left:left + a.shape[2]] = dev(a)
    v = big[:, top:top + a.shape[1], left:left + a.shape[2]]
    assert v.data_ptr() != big.data_ptr() and not v.is_contiguous()
    return v


def bits(a):
    """fp32 bit patterns, with every NaN as one pattern."""
    a = np.ascontiguousarray(np.asarray(a, F32))
    return np.where(np.isnan(a), F32(np.nan), a).view(np.uint32)


def device_input(name):
    return embed(CASES[name], 16, 24, 3, 5) if name == "2x7x13" else dev(CASES[name])


@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_colorize_bit_equal(name, mode, stacked):
    top = dev(frames(name)) if stacked else None
    got = run(mode, device_input(name), dev(LUT), top)
    B, H, W = CASES[name].shape
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 2 * H if stacked else H, W, 3)
    assert got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), ref(name, mode, stacked))


def test_range_cases_are_what_the_docstring_says():
    idx = RR.index_range(CASES["3x67x131"])
    assert not idx[0].any() and not idx[1].any() and len(np.unique(idx[2])) > 100
    two = RR.range_u(CASES["2x7x13"])[0]
    assert two[0].max() == 65535 and 25550 <= two[1].max() < 65535  # a planted inf in image 0 only
    from esmstereo_amd._lib import lib
    per_partial = lib.esm_disp_colorize_workspace(1, 1, 1) // 2  # one partial and one folded record
    assert lib.esm_disp_colorize_workspace(1, 1024, 1024) // per_partial == 512 + 1
    assert lib.esm_disp_colorize_workspace(1, 3, 350003) // per_partial == 513 + 1
    assert lib.esm_disp_colorize_workspace(1, 67, 131) // per_partial == 5 + 1


@pytest.mark.parametrize("mode,table", [("scale", "jet"), ("range", "magma"), ("depth", "jet")])
def test_shipped_tables(mode, table):
    from esmstereo_amd import render as R
    lut = R.colormap_lut(table, DEV)
    assert lut.is_cuda and lut.dtype == torch.uint8
    got = run(mode, dev(CASES["3x67x131"]), lut)
    host = R.colormap_lut(table, "cpu").numpy()
    assert np.array_equal(got.cpu().numpy(), ref("3x67x131", mode, False, host))


@pytest.mark.parametrize("mode", MODES)
def test_input_layouts(mode):
    name = "3x67x131"
    d, lut, want = CASES[name], dev(LUT), ref(name, mode, False)
    assert np.array_equal(run(mode, dev(d[:, None]), lut).cpu().numpy(), want)          # [B, 1, H, W]
    one = run(mode, dev(d[2]), lut)                                                      # [H, W]
    assert tuple(one.shape) == (67, 131, 3) and np.array_equal(one.cpu().numpy(), want[2])
    top = dev(frames(name)[2])
    one = run(mode, dev(d[2]), lut, top)                                                 # [H, W] under [H, W, 3]
    assert tuple(one.shape) == (134, 131, 3)
    assert np.array_equal(one.cpu().numpy(), RR.stack(frames(name)[2], want[2]))
    # a row-strided view (every second row of a taller map; the rows between are NaN): read where it lies
    tall = torch.full((3, 134, 131), float("nan"), device=DEV)
    tall[:, ::2] = dev(d)
    view = tall[:, ::2]
    assert not view.is_contiguous() and view.stride(2) == 1
    assert np.array_equal(run(mode, view, lut).cpu().numpy(), want)
    # a W-strided view is copied, not refused
    wide = torch.full((3, 67, 262), float("nan"), device=DEV)
    wide[:, :, ::2] = dev(d)
    assert np.array_equal(run(mode, wide[:, :, ::2], lut).cpu().numpy(), want)


def raw_colorize(mode, d, lut, top, out_ptr):
    """The C entry point itself, writing at any byte address."""
    from esmstereo_amd._lib import check, lib
    B, H, W = (int(v) for v in d.shape)
    work = torch.empty(check(lib.esm_disp_colorize_workspace(B, H, W)), dtype=torch.uint8, device=DEV)
    check(lib.esm_disp_colorize_u8(d.data_ptr(), d.stride(0), d.stride(1), B, H, W, MODES.index(mode), 0.01,
                                   float(NUM), MAX_DEPTH, lut.data_ptr(), top.data_ptr() if top is not None else None,
                                   out_ptr, work.data_ptr(), None), "colorize")
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["1x3x5", "2x7x13", "3x67x131"])
def test_every_output_alignment_and_nothing_beyond(name, mode):
    """The output (and the frame on top) at each of the four byte alignments inside a poisoned buffer: the frame is
    right and the bytes before and after it are untouched."""
    d, lut = device_input(name), dev(LUT)
    B, H, W = CASES[name].shape
    want = ref(name, mode, True)
    n, pad = want.size, 64
    for off in range(4):
        big = torch.full((pad + off + n + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        src = torch.full((off + n // 2 + 4,), 0x5A, dtype=torch.uint8, device=DEV)
        src[off:off + n // 2] = dev(frames(name)).reshape(-1)
        raw_colorize(mode, d, lut, src[off:], big.data_ptr() + pad + off)
        host = big.cpu().numpy()
        assert np.array_equal(host[pad + off:pad + off + n], want.reshape(-1)), off
        assert (host[:pad + off] == 0xA5).all() and (host[pad + off + n:] == 0xA5).all(), off
        big.fill_(0xA5)  # the same without the frame on top
        raw_colorize(mode, d, lut, None, big.data_ptr() + pad + off)
        host = big.cpu().numpy()
        assert np.array_equal(host[pad + off:pad + off + n // 2], ref(name, mode, False).reshape(-1)), off
        assert (host[:pad + off] == 0xA5).all() and (host[pad + off + n // 2:] == 0xA5).all(), off


@pytest.mark.parametrize("name", list(CASES))
def test_depth_map_bit_exact(name):
    from esmstereo_amd import render as R
    d = device_input(name)
    got = R.disparity_to_depth(d, BASELINE, FOCAL, MAX_DEPTH)
    assert got.dtype == torch.float32 and got.shape == d.shape and got.is_contiguous()
    assert np.array_equal(bits(got.cpu().numpy()), bits(RR.depth_map(CASES[name], NUM, MAX_DEPTH)))


def test_depth_map_layouts_and_bounds():
    from esmstereo_amd import render as R
    d = CASES["3x67x131"]
    want = bits(RR.depth_map(d, NUM, MAX_DEPTH))
    got = R.disparity_to_depth(dev(d[:, None]), BASELINE, FOCAL, MAX_DEPTH)
    assert tuple(got.shape) == (3, 1, 67, 131) and np.array_equal(bits(got.cpu().numpy()).reshape(3, 67, 131), want)
    got = R.disparity_to_depth(dev(d[2]), BASELINE, FOCAL, MAX_DEPTH)
    assert tuple(got.shape) == (67, 131) and np.array_equal(bits(got.cpu().numpy()), want[2])
    # the C entry point into a poisoned buffer, at an element offset that is no multiple of four
    from esmstereo_amd._lib import check, lib
    x = dev(CASES["2x7x13"])
    n = x.numel()
    big = torch.full((7 + n + 9,), -77.0, device=DEV)
    check(lib.esm_disp_to_depth_f32(x.data_ptr(), x.stride(0), x.stride(1), big.data_ptr() + 4 * 7, 2, 7, 13,
                                    float(NUM), MAX_DEPTH, None), "depth")
    torch.cuda.synchronize()
    host = big.cpu().numpy()
    assert np.array_equal(bits(host[7:7 + n]), bits(RR.depth_map(CASES["2x7x13"], NUM, MAX_DEPTH)).reshape(-1))
    assert (host[:7] == -77).all() and (host[7 + n:] == -77).all()


@pytest.mark.parametrize("mode", MODES)
def test_two_runs_give_the_same_bytes(mode):
    d, lut, top = dev(CASES["3x67x131"]), dev(LUT), dev(frames("3x67x131"))
    a = run(mode, d, lut, top).cpu().numpy()
    b = run(mode, d, lut, top).cpu().numpy()
    assert np.array_equal(a, b)


def test_range_into_the_callers_buffers():
    """A per-frame loop's form: the frame into `out`, the partial ranges in `workspace`, nothing allocated."""
    from esmstereo_amd import render as R
    name = "3x67x131"
    d, lut, top = dev(CASES[name]), dev(LUT), dev(frames(name))
    out = torch.full((3 * 134 * 131 * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    work = torch.full((R.range_workspace_bytes(3, 67, 131) + 8,), 0xA5, dtype=torch.uint8, device=DEV)
    got = R.colorize_range(d, lut, stack=top, out=out, workspace=work)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (3, 134, 131, 3)
    assert np.array_equal(got.cpu().numpy(), ref(name, "range", True))
    assert (work[-8:] == 0xA5).all()  # the workspace is as large as the query says, no larger
    with pytest.raises(ValueError):
        R.colorize_range(d, lut, stack=top, out=out[1:])
    with pytest.raises(ValueError):
        R.colorize_range(d, lut, workspace=work[:8])
    with pytest.raises(ValueError):
        R.colorize_range(d, lut, workspace=work[1:])  # not 8-byte aligned


def test_wrong_arguments_are_refused():
    from esmstereo_amd import render as R
    d, lut = dev(CASES["1x3x5"]), dev(LUT)
    with pytest.raises(ValueError):
        R.colorize_disparity(d.double(), lut)
    with pytest.raises(ValueError):
        R.colorize_disparity(d, lut[:, :2])
    with pytest.raises(ValueError):
        R.colorize_disparity(d, lut, stack=torch.zeros(1, 3, 4, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        R.colorize_disparity(d, lut.cpu())


def test_stereo_node_process_rendered():
    import json
    import os
    import esmstereo_amd as E
    from esmstereo_amd.backbone import StubFeature
    from esmstereo_amd.node import StereoNode
    from helpers import GOLDEN_DIR, load_spec, seeded_state
    from oracle import io_oracle as IO
    with open(os.path.join(GOLDEN_DIR, "manifest.json")) as f:
        m = json.load(f)["hot_S_gwc.npz"]
    model = E.ESMStereo_trt(192, True, False, m["backbone"], 16, feature_cls=StubFeature)
    model.load_state_dict(seeded_state(load_spec(m["spec"]), m["seed"]))
    model = model.eval().to(DEV)
    H, W = 101, 219  # 101 rows of 657 bytes: the colour image under the left frame starts at an odd address
    rng = np.random.default_rng(2)
    left = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    right = np.roll(left, -6, axis=1)
    node = StereoNode(model, H, W, max_disp=192.0)
    assert node.lut is None and not hasattr(node, "host_frame")  # nothing allocated for a node that never renders
    u16, frame, ms = node.process_rendered(left, right)
    assert u16.shape == (H, W) and u16.dtype == np.uint16 and ms > 0
    assert frame.shape == (2 * H, W, 3) and frame.dtype == np.uint8
    with torch.no_grad():
        disp = model(node.net_in[0], node.net_in[1])[0].cpu().numpy()
    ref_u, ref_m = IO.node_filter_u16(disp, 0, 0, H, W, 192.0)
    assert np.array_equal(u16, ref_u)
    magma = E.colormap_lut("magma", "cpu").numpy()  # the default table, BGR
    assert np.array_equal(frame, RR.render(ref_m[None], magma, "range", left[None])[0])
    # the 16-bit output is process()'s, and a second run gives the same bytes
    assert np.array_equal(node.process(left, right)[0], u16)
    u16b, frame_b, _ = node.process_rendered(left, right)
    assert np.array_equal(u16b, u16) and np.array_equal(frame_b, frame)
    # a table of the caller's, given to the constructor
    node2 = StereoNode(model, H, W, max_disp=192.0, lut=dev(LUT))
    assert tuple(node2.host_frame.shape) == (2 * H, W, 3) and node2.host_frame.is_pinned()
    _, frame2, _ = node2.process_rendered(left, right)
    assert np.array_equal(frame2, RR.render(ref_m[None], LUT, "range", left[None])[0])
