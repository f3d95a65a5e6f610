"""The one-branch GELU (csrc/common.h gelu_erf) through every kernel family that has its own epilogue code.

A plain BasicConv epilogue with BN folded to scale 1 and shift 0 and no residual, behind an identity conv, stores
exactly GELU(input): the products with the zero weights add exact zeros.  One member of every family runs on the same
pool of input values (drawn from the grids of tests/test_gelu_fit_host.py; finite and normal, so that no family's
handling of denormal operands enters):

* 1x1, 1 -> 1, hints 0 / SMALL / WIDE (the launch of test_gelu_epilogue_branch_free_erf): the reference bits R1, and
  R2 = the same launch over R1;
* 3x3 16 -> 16 on 16 x 8 x 40 and 3x3x3 8 -> 8 on 8 x 4 x 6 x 24 with the centre tap the identity matrix (one or two
  16-column tiles plus a ragged one), forced through the lean, stem, row-streaming, tiled, plane-streaming, LDS-staged
  and direct forms; the 1x1 pointwise form; the 2-D single-input-channel form (1 -> 16: channel 0 carries the value);
* ConvTranspose k4 s2 p1 with tap (1, 1) the identity (out[2i, 2j] = GELU(x[i, j]), the other outputs GELU(0) = 0)
  through the all-classes, tiled, lean and general forms;
* the pair forms (LDS-staged and K-split, 2-D and 3-D) with both convs the identity, and the fused ConvTranspose + 1x1
  (lean and tiled) with one transposed tap and the 1x1 the identity on the transposed conv's channels and zero on the
  concatenated ones: these store GELU(GELU(x)).

Every family must return R1 (R2 for the two-stage ones) bit for bit (the sign of a zero aside: an accumulator starts
at +0), and meet |y - GELU(x)| <= 2.5e-7 |x| + 1e-37 against fp64 F.gelu, the bound of
test_gelu_epilogue_branch_free_erf (for the second stage x is R1, which the bitwise check ties to the kernel's own
intermediate).  The special values go through the 1 -> 1 launch, where no zero weight meets an infinity.

Families that cannot take an identity layer, and why:
* gwc_stem (gwc_stem.hip): its input is the group-wise correlation of two feature maps computed in the same kernel;
  no weight choice makes its pre-activation an arbitrary given value (checked against fp64 in test_gwc_stem_fused);
* the fused refinement heads (shuffle_tail.hip): their GELU'd maps (c1, the second conv) never leave LDS and feed
  further convs with SiLU / softmax stages behind them (checked in the shuffle-tail tests of test_gpu_parity.py).
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd._lib import (FORM_C1IN, FORM_GENERAL, FORM_PW, FORM_SMALL, FORM_STEM, FORM_TILE2,  # noqa: E402
                                FORM_TILE3, FORM_WIDE, FORM_WIDE3, FORM_WIDET, HINT_C1IN, HINT_ROWS, HINT_SMALL,
                                HINT_SMALL_NO_ZSPLIT, HINT_STEM, HINT_TILE, HINT_TILE_PW, HINT_TILE_WLDS, HINT_WIDE,
                                HINT_WIDE3, HINT_WIDET)
from esmstereo_amd.engine import ACT_GELU, Ctx, pack_conv, run_conv, run_convt_1x1, run_pair2  # noqa: E402

DEV = torch.device("cuda")
HINT_PW = HINT_TILE | HINT_TILE_PW
LDS_STAGED, DIRECT, ROWS_FORM = 0x11, 0x211, 0x411  # the general form's variants (test_conv_every_tile_variant)
N2, N3 = 16 * 8 * 40, 8 * 4 * 6 * 24
_REF = {}


def pool() -> torch.Tensor:
    """N2 finite, normal fp32 values: the parity test's grid and windows, fp32 values of +-[2^-4, 16), a log sweep."""
    g = torch.Generator().manual_seed(2024)
    pick = lambda t, n: t[torch.randperm(t.numel(), generator=g)[:n]]  # noqa: E731
    lin = pick(torch.linspace(-12, 12, 200001), 2048)
    win = torch.cat([pick(torch.linspace(1.40, 1.43, 20001), 256), pick(torch.linspace(-1.43, -1.40, 20001), 256)])
    lo, hi = (int(np.array(v, np.float32).view(np.uint32)) for v in (2.0 ** -4, 16.0))
    bits = torch.randint(lo // 16, hi // 16, (1536,), generator=g) * 16
    dense = torch.from_numpy(bits.numpy().astype(np.uint32).view(np.float32).copy())
    dense = dense * (torch.randint(0, 2, (1536,), generator=g) * 2 - 1).float()
    mag = torch.from_numpy(np.logspace(-30, math.log10(3.0e38), 1024).astype(np.float32))
    sweep = mag * (torch.randint(0, 2, (1024,), generator=g) * 2 - 1).float()
    x = torch.cat([lin, win, dense, sweep])
    x = x[torch.randperm(x.numel(), generator=g)]
    assert x.numel() == N2 and bool(torch.isfinite(x).all())
    assert bool(((x == 0) | (x.abs() >= 1e-30)).all())
    return x


def identity(nd: int, cin: int, cout: int, k: int, transposed: bool = False, extra: int = 0):
    """A packed GELU BasicConv whose BN is scale 1 / shift 0 and whose only nonzero weights copy input channel i to
    output channel i: at the centre tap (k 3), the only tap (k 1) or tap (1, 1[, 1]) of a ConvTranspose k4 s2 p1.
    `extra` further input channels have zero weights."""
    if transposed:
        cls = torch.nn.ConvTranspose3d if nd == 3 else torch.nn.ConvTranspose2d
        conv = cls(cin, cout, 4, 2, 1, bias=False)
    else:
        cls = torch.nn.Conv3d if nd == 3 else torch.nn.Conv2d
        conv = cls(cin + extra, cout, k, 1, k // 2, bias=False)
    with torch.no_grad():
        conv.weight.zero_()
        tap = (1,) * nd if transposed else (k // 2,) * nd
        for i in range(min(cin, cout)):
            conv.weight[(i, i) + tap] = 1.0
    p = pack_conv(conv.to(DEV), None, ACT_GELU)
    p.scale = torch.ones(cout, device=DEV)
    p.shift = torch.zeros(cout, device=DEV)
    return p


def conv_form(p, x, hint):
    d, _, _ = EN._conv_desc(Ctx(DEV), p, [x], hint=hint)
    return _lib.lib.esm_conv_form(ctypes.byref(d))


def ref():
    """(pool, R1 = GELU(pool), R2 = GELU(R1)) through the 1x1 1 -> 1 launch with the automatic form, computed once."""
    if not _REF:
        x = pool()
        p = identity(2, 1, 1, 1)
        r1 = run_conv(Ctx(DEV), p, [x.view(1, 1, 1, N2).to(DEV)]).view(-1).clone()
        r2 = run_conv(Ctx(DEV), p, [r1.view(1, 1, 1, N2)]).view(-1).clone()
        torch.cuda.synchronize()
        _REF.update(x=x, r1=r1.cpu(), r2=r2.cpu(), p11=p)
    return _REF["x"], _REF["r1"], _REF["r2"]


def check(y: torch.Tensor, arg: torch.Tensor, want: torch.Tensor, what: str):
    """y: a family's output; arg: the value each element's (last) GELU was applied to; want: the reference bits."""
    y = y.detach().cpu().reshape(-1)
    arg, want = arg.reshape(-1), want.reshape(-1)
    assert y.shape == want.shape, what
    gold = F.gelu(arg.double())
    err = (y.double() - gold).abs()
    lim = 2.5e-7 * arg.double().abs() + 1e-37
    worst = float((err / lim).max())
    print(f"{what}: worst |error| / (2.5e-7 |x| + 1e-37) = {worst:.3f}")
    assert bool((err <= lim).all()), (what, worst)
    same = (y.view(torch.int32) == want.view(torch.int32)) | ((y == 0) & (want == 0))
    assert bool(same.all()), (what, int((~same).sum()))


def strided_fill(shape, vals: torch.Tensor) -> torch.Tensor:
    """zeros(shape) with vals at the even positions of every spatial axis (where tap (1, 1[, 1]) of the ConvTranspose
    writes)."""
    t = torch.zeros(shape)
    t[(slice(None), slice(None)) + (slice(0, None, 2),) * (len(shape) - 2)] = vals
    return t


def test_reference_launch_meets_the_bound():
    """R1 and R2 themselves against fp64, and the other forms of the 1 -> 1 launch bit for bit."""
    x, r1, r2 = ref()
    check(r1, x, r1, "1x1 1->1 automatic")
    check(r2, r1, r2, "1x1 1->1 automatic, second stage")
    for hint in (HINT_SMALL, HINT_WIDE):
        y = run_conv(Ctx(DEV), _REF["p11"], [x.view(1, 1, 1, N2).to(DEV)], hint=hint)
        check(y, x, r1, f"1x1 1->1 hint {hint:#x}")


SINGLE = [  # (id, nd, k, hint, the form esm_conv_form must report)
    ("2d-lean", 2, 3, HINT_SMALL, FORM_SMALL),
    ("2d-stem", 2, 3, HINT_STEM, FORM_STEM),
    ("2d-row-streaming", 2, 3, HINT_WIDE, FORM_WIDE),
    ("2d-tiled", 2, 3, HINT_TILE, FORM_TILE2),
    ("2d-lds-staged", 2, 3, LDS_STAGED, FORM_GENERAL),
    ("2d-direct", 2, 3, DIRECT, FORM_GENERAL),
    ("2d-rows", 2, 3, ROWS_FORM, FORM_GENERAL),
    ("2d-pointwise", 2, 1, HINT_PW, FORM_PW),
    ("3d-lean", 3, 3, HINT_SMALL, FORM_SMALL),
    ("3d-lean-plain-loop", 3, 3, HINT_SMALL | HINT_SMALL_NO_ZSPLIT, FORM_SMALL),
    ("3d-stem", 3, 3, HINT_STEM, FORM_STEM),
    ("3d-plane-streaming", 3, 3, HINT_WIDE3, FORM_WIDE3),
    ("3d-tiled", 3, 3, HINT_TILE, FORM_TILE3),
    ("3d-tiled-wlds", 3, 3, HINT_TILE | HINT_TILE_WLDS, FORM_TILE3),
    ("3d-lds-staged", 3, 3, LDS_STAGED, FORM_GENERAL),
    ("3d-direct", 3, 3, DIRECT, FORM_GENERAL),
    ("3d-rows", 3, 3, ROWS_FORM, FORM_GENERAL),
    ("3d-pointwise", 3, 1, HINT_PW, FORM_PW),
]


@pytest.mark.parametrize("name,nd,k,hint,form", SINGLE, ids=[c[0] for c in SINGLE])
def test_identity_conv(name, nd, k, hint, form):
    x, r1, _ = ref()
    c, shape, n = (16, (1, 16, 8, 40), N2) if nd == 2 else (8, (1, 8, 4, 6, 24), N3)
    p = identity(nd, c, c, k)
    xd = x[:n].view(shape).to(DEV)
    assert conv_form(p, xd, hint) == form
    check(run_conv(Ctx(DEV), p, [xd], hint=hint), x[:n], r1[:n], name)


def test_identity_conv_single_input_channel():
    """conv_stem.hip c1in_kernel, 1 -> 16: channel 0 is GELU(x), the other channels GELU(0) = 0."""
    x, r1, _ = ref()
    p = identity(2, 1, 16, 3)
    xd = x[:320].view(1, 1, 8, 40).to(DEV)
    assert conv_form(p, xd, HINT_C1IN) == FORM_C1IN
    arg, want = torch.zeros(1, 16, 8, 40), torch.zeros(1, 16, 8, 40)
    arg[0, 0], want[0, 0] = x[:320].view(8, 40), r1[:320].view(8, 40)
    check(run_conv(Ctx(DEV), p, [xd], hint=HINT_C1IN), arg, want, "2d-c1in")


TRANSPOSED = [
    ("2dT-all-classes", 2, HINT_WIDET, FORM_WIDET),
    ("2dT-tiled", 2, HINT_TILE, FORM_TILE2),
    ("2dT-lean", 2, HINT_SMALL, FORM_SMALL),
    ("2dT-lds-staged", 2, LDS_STAGED, FORM_GENERAL),
    ("2dT-direct", 2, DIRECT, FORM_GENERAL),
    ("3dT-tiled", 3, HINT_TILE, FORM_TILE3),
    ("3dT-lean", 3, HINT_SMALL, FORM_SMALL),
    ("3dT-lds-staged", 3, LDS_STAGED, FORM_GENERAL),
]


def _transposed_case(nd):
    """(channels, input shape, output shape, number of input values)"""
    return (16, (1, 16, 4, 20), (1, 16, 8, 40), 1280) if nd == 2 else (8, (1, 8, 2, 3, 12), (1, 8, 4, 6, 24), 576)


@pytest.mark.parametrize("name,nd,hint,form", TRANSPOSED, ids=[c[0] for c in TRANSPOSED])
def test_identity_conv_transposed(name, nd, hint, form):
    x, r1, _ = ref()
    c, ishape, oshape, n = _transposed_case(nd)
    p = identity(nd, c, c, 4, transposed=True)
    xd = x[:n].view(ishape).to(DEV)
    assert conv_form(p, xd, hint) == form
    y = run_conv(Ctx(DEV), p, [xd], hint=hint)
    check(y, strided_fill(oshape, x[:n].view(ishape)), strided_fill(oshape, r1[:n].view(ishape)), name)


PAIRS = [("2d-pair-lds", 2, False, "lds"), ("2d-pair-ksplit", 2, True, "ksplit"), ("3d-pair-ksplit", 3, True, "ksplit")]


@pytest.mark.parametrize("name,nd,ksplit,form", PAIRS, ids=[c[0] for c in PAIRS])
def test_identity_pair(name, nd, ksplit, form):
    """Two 3x3 (3x3x3) identity BasicConvs in one launch: GELU(GELU(x))."""
    x, r1, r2 = ref()
    c, shape, n = (16, (1, 16, 8, 40), N2) if nd == 2 else (8, (1, 8, 4, 6, 24), N3)
    pa, pb = identity(nd, c, c, 3), identity(nd, c, c, 3)
    ctx = Ctx(DEV)
    y = run_pair2(ctx, pa, [x[:n].view(shape).to(DEV)], pb, force=True, ksplit=ksplit)
    assert (ctx.meta[-1]["kind"], ctx.meta[-1]["form"]) == ("conv_pair", form)
    check(y, r1[:n], r2[:n], name)


UP1 = [("2d-convt+1x1-lean", 2, HINT_SMALL, "lean"), ("2d-convt+1x1-tiled", 2, HINT_TILE | HINT_ROWS(1), "tiled"),
       ("3d-convt+1x1-lean", 3, HINT_SMALL, "lean"), ("3d-convt+1x1-tiled", 3, HINT_TILE | HINT_ROWS(1), "tiled")]


@pytest.mark.parametrize("name,nd,hint,form", UP1, ids=[c[0] for c in UP1])
def test_identity_convt_1x1(name, nd, hint, form):
    """ConvTranspose (tap (1, 1[, 1]) the identity) + cat + 1x1 (identity on the transposed conv's channels, zero on
    the concatenated ones, which carry ordinary finite values): GELU(GELU(x)) at the even positions, 0 elsewhere."""
    x, r1, r2 = ref()
    c, ishape, oshape, n = _transposed_case(nd)
    pa, pb = identity(nd, c, c, 4, transposed=True), identity(nd, c, c, 1, extra=c)
    torch.manual_seed(5)
    side = torch.randn(oshape).to(DEV)
    assert EN.convt_1x1_supported(pa, pb, [side])
    ctx = Ctx(DEV)
    old = dict(EN.HINT_SET)
    EN.HINT_SET["convT"] = hint
    try:
        y = run_convt_1x1(ctx, pa, [x[:n].view(ishape).to(DEV)], pb, [side])
    finally:
        EN.HINT_SET.clear()
        EN.HINT_SET.update(old)
    assert (ctx.meta[-1]["kind"], ctx.meta[-1]["form"]) == ("conv_up1", form)
    check(y, strided_fill(oshape, r1[:n].view(ishape)), strided_fill(oshape, r2[:n].view(ishape)), name)


def test_special_values():
    """+-0, denormals, large negative values, +-inf and NaN through the 1 -> 1 launch (every pixel its own column: no
    zero weight meets a non-finite value), in each of its three forms."""
    ref()
    fi = np.finfo(np.float32)
    vals = [0.0, -0.0, 1e-40, -1e-40, float(fi.smallest_subnormal), -float(fi.smallest_subnormal), float(fi.tiny),
            -float(fi.tiny), -6.0, -20.0, -1e6, -float(fi.max), float(fi.max), float("inf"), float("nan"), float("-inf")]
    x = torch.tensor(vals + [1.0] * (64 - len(vals)), dtype=torch.float32)
    gold = F.gelu(x.double())
    for hint in (0, HINT_SMALL, HINT_WIDE):
        y = run_conv(Ctx(DEV), _REF["p11"], [x.view(1, 1, 1, 64).to(DEV)], hint=hint).view(-1).cpu()
        fin = torch.isfinite(x)
        err = (y.double() - gold).abs()
        assert bool((err[fin] <= 2.5e-7 * x.double().abs()[fin] + 1e-37).all()), hex(hint)
        assert y[0] == 0 and y[1] == 0, hex(hint)                       # (the accumulator's +0 absorbs the sign of -0)
        assert bool((y[9:12] == 0).all()), (hex(hint), y[9:12])        # -20, -1e6, -FLT_MAX: zero, nothing left behind
        assert -6.0e-9 <= float(y[8]) < 0, (hex(hint), float(y[8]))    # GELU(-6) = -5.92e-9
        assert float(y[12]) == float(fi.max) and float(y[13]) == float("inf"), hex(hint)
        assert bool(torch.isnan(y[14])), hex(hint)
        assert bool(torch.isnan(y[15])), hex(hint)                      # -inf * 0, as the two-branch form gave
        assert bool((y[16:] == y[16]).all()), hex(hint)                 # the non-finite pixels touched no other pixel
