"""GPU layout tests: every kernel form on strided views with poisoned surroundings (tests/layouts.py).

The parity tests run the kernels on fresh, contiguous, aligned tensors whose neighbours hold ordinary numbers.
The hot path runs them on crops, channel slices and buffers carved 256 B apart out of one arena.  Each case
here embeds every source, every epilogue operand and every output in its own allocation full of a NaN
sentinel, in two placements ("gapped16": 16-byte aligned base and strides, vector paths active; "odd": 4-byte
aligned base, odd row stride, the scalar fall-backs), and asserts

  (c) the form under test is the one ``esm_conv_form`` reports for the descriptor (convs);
  (d) the output is finite and within the op's own tolerance of the fp64 torch reference of the logical data
      (1e-5 relative for the convs; 1e-6 / bitwise where the op's parity test says so): a load one element
      outside the extent turns the output into NaN, whatever weight or mask it meets;
  (e) every cell outside the ``out`` / ``out2`` views is bitwise untouched;
  (f) the result is bitwise the same form's result on contiguous copies (fixed-order, address-independent sums).

Where a form's check rejects a placement the documented outcome is asserted instead: the fall-back form the
query reports, or an ``EsmError``.  Entry points that take bare contiguous pointers get "carved" operands.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import feature_pair
from layouts import PLACEMENTS, assert_guards_intact, embed, guard_snapshot
from test_gpu_parity import _mk, _ref_conv, pk, rel

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

import esmstereo_amd as E  # noqa: E402
from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd._lib import HINT_ROWS as ROWS  # noqa: E402
from esmstereo_amd._lib import (HINT_C1IN, HINT_C1T, HINT_GWC_STEM_WLDS, HINT_NO_TILE, HINT_SMALL,  # noqa: E402
                                HINT_SMALL_W8, HINT_STEM, HINT_TILE, HINT_TILE_DMA_FLIP, HINT_TILE_PW, HINT_TILE_WLDS,
                                HINT_WIDE, HINT_WIDE3, HINT_WIDE_KS2, HINT_WIDET)
from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd.engine import ACT_GELU, ACT_NONE, ACT_SILU, Ctx, run_conv  # noqa: E402
from oracle import esm_oracle as O  # noqa: E402

DEV = torch.device("cuda")
B = 2

GENERAL, STEM, C1IN, SMALL, WIDE, WIDE3, WIDET, TILE3, TILE2, PW = (
    _lib.FORM_GENERAL, _lib.FORM_STEM, _lib.FORM_C1IN, _lib.FORM_SMALL, _lib.FORM_WIDE, _lib.FORM_WIDE3,
    _lib.FORM_WIDET, _lib.FORM_TILE3, _lib.FORM_TILE2, _lib.FORM_PW)


def _finite_close(y, ref, tol, what):
    assert bool(torch.isfinite(y).all()), f"{what}: a value from outside the logical extent reached the output"
    assert rel(y, ref) < tol, what


def _put(t, where, spatial=True):
    return embed(t, where, DEV, spatial=spatial)


def test_harness_on_the_device():
    """The harness itself on GPU memory (its CPU proof: tests/test_layouts_host.py): the surroundings read as NaN
    there too, and one cell written past the last row's end is caught."""
    for where in PLACEMENTS + ("carved",):
        v = _put(torch.zeros(B, 5, 7, 19), where)
        snap = guard_snapshot(v)
        flat = torch.empty(0, device=DEV).set_(v.untyped_storage())
        assert int(snap.inside.sum()) == v.numel() and bool(torch.isnan(flat[~snap.inside]).all())
        v.fill_(1.0)
        assert_guards_intact(v, snap)
        last = v.storage_offset() + sum((n - 1) * s for n, s in zip(v.shape, v.stride()))
        flat[last + 1] = 1.0
        with pytest.raises(AssertionError, match="1 guard cell"):
            assert_guards_intact(v, snap)


# ----------------------------------------------------------------------------- convs


def _form(pc, srcs, out, **kw):
    d, _, _ = EN._conv_desc(Ctx(DEV), pc, srcs, out, **kw)
    return _lib.lib.esm_conv_form(ctypes.byref(d))


class Case:
    """One conv row: geometry, the hints to force, the form they must give, the epilogue operands."""

    def __init__(self, name, nd, cins, cout, k, s, shape, hints, form, *, tr=False, p=None, epi="", bn=True,
                 act=ACT_GELU, shuffle=1, post=1.0, spatial=True, loose=None, other=None):
        self.name, self.nd, self.cins, self.cout, self.k, self.s, self.shape = name, nd, cins, cout, k, s, shape
        self.hints, self.form, self.tr, self.epi = hints, form, tr, set(epi.split()) if epi else set()
        self.p = (1 if tr else k // 2) if p is None else p
        self.bn, self.act, self.shuffle, self.post, self.spatial = bn, act, shuffle, post, spatial
        self.loose = loose      # index of a source left contiguous (its row stride then differs from the others')
        self.other = other or {}  # placement -> the form the query must report there instead (a documented fall-back)


def _each(form, *fields):
    """One forced form with each setting of its fields (0: the form bit alone)."""
    return [form | v for v in fields]


CONV_CASES = [
    # general forms: LDS-staged (0x11, 0x44), direct K-split (0x241), the automatic direct choice (NO_TILE | NO_STEM
    # keeps the lean / stem forms away)
    Case("general-2d-k3s1", 2, (12,), 24, 3, 1, (9, 37), [0x11, 0x44, 0x241], GENERAL),
    Case("general-2d-k3s2", 2, (12,), 24, 3, 2, (9, 37), [0x11, 0x44, 0x241], GENERAL),
    Case("general-2d-convT", 2, (12,), 12, 4, 2, (9, 19), [0x11, 0x44, 0x241], GENERAL, tr=True),
    Case("general-3d-k3", 3, (12,), 12, 3, 1, (5, 7, 21), [0x11, 0x44, 0x241], GENERAL),
    Case("general-2d-multisource-k1", 2, (16, 8), 24, 1, 1, (9, 37), [0x11, 0x241, 0x212], GENERAL),
    # row-streaming form
    Case("rows-2d", 2, (16,), 16, 3, 1, (9, 29), [0x411], GENERAL),
    Case("rows-3d", 3, (8,), 8, 3, 1, (5, 7, 19), [0x411], GENERAL),
    Case("rows-2d-k5-mul-res", 2, (1,), 16, 5, 1, (9, 29), [0x411], GENERAL, epi="mul res"),
    # 16-block narrow-output form
    Case("stem-3d", 3, (12,), 12, 3, 1, (5, 6, 21), [HINT_STEM], STEM),
    Case("stem-2d", 2, (16,), 8, 3, 1, (9, 37), [HINT_STEM], STEM),
    Case("stem-3d-mul-res", 3, (1,), 8, 3, 1, (5, 6, 21), [HINT_STEM], STEM, epi="mul res"),
    # VALU single-input-channel form (the source: one channel between poisoned neighbours)
    Case("c1in-k3s2", 2, (1,), 16, 3, 2, (13, 37), [HINT_C1IN], C1IN),
    Case("c1in-k5", 2, (1,), 16, 5, 1, (13, 37), [HINT_C1IN], C1IN),
    Case("c1in-k3s1-32", 2, (1,), 32, 3, 1, (13, 37), [HINT_C1IN], C1IN),
    # lean K-split form, 4 and 8 waves
    Case("small-2d-k1-3src", 2, (16, 16, 32), 16, 1, 1, (9, 37), _each(HINT_SMALL, 0, HINT_SMALL_W8), SMALL),
    Case("small-3d-k3s2", 3, (16,), 24, 3, 2, (3, 6, 20), [HINT_SMALL], SMALL),
    Case("small-3d-convT", 3, (24,), 16, 4, 2, (2, 3, 10), _each(HINT_SMALL, 0, HINT_SMALL_W8), SMALL, tr=True),
    Case("small-2d-k3-res-out2", 2, (16, 32), 16, 3, 1, (9, 21), _each(HINT_SMALL, 0, HINT_SMALL_W8), SMALL,
         epi="res out2"),
    Case("small-2d-k5", 2, (1,), 16, 5, 1, (9, 21), [HINT_SMALL], SMALL),
    Case("small-2d-k3", 2, (16,), 16, 3, 1, (9, 21), [HINT_SMALL], SMALL),
    # register-weight row-streaming form: every rows-per-wave block, the two-wave K split
    Case("wide-k3", 2, (16,), 16, 3, 1, (9, 37), _each(HINT_WIDE, 0, ROWS(1), ROWS(2), ROWS(3),
         ROWS(2) | HINT_WIDE_KS2, ROWS(3) | HINT_WIDE_KS2), WIDE),
    Case("wide-k3-2src", 2, (16, 24), 16, 3, 1, (9, 37), _each(HINT_WIDE, 0, ROWS(2) | HINT_WIDE_KS2), WIDE),
    Case("wide-k5", 2, (1,), 16, 5, 1, (9, 37), _each(HINT_WIDE, 0, ROWS(1)), WIDE),
    Case("wide-k1-32", 2, (16, 16), 32, 1, 1, (9, 37), [HINT_WIDE], WIDE),
    Case("wide-k3-res-out2", 2, (16,), 16, 3, 1, (9, 37), _each(HINT_WIDE, 0, ROWS(3) | HINT_WIDE_KS2), WIDE,
         epi="res out2"),
    # sources with different row strides: the wide form steps aside for the automatic rules (the lean form here)
    Case("wide-steps-aside", 2, (16, 24), 16, 3, 1, (9, 37), [HINT_WIDE], SMALL, loose=1),
    # register-weight plane-streaming 3-D form: plane pairs / row ring (32 -> 8), 3 groups
    Case("wide3-32to8", 3, (32,), 8, 3, 1, (5, 7, 19), [HINT_WIDE3], WIDE3),
    Case("wide3-12to12", 3, (12,), 12, 3, 1, (5, 7, 19), [HINT_WIDE3], WIDE3),
    Case("wide3-8to8-mul-res", 3, (8,), 8, 3, 1, (5, 7, 19), [HINT_WIDE3], WIDE3, epi="mul res"),
    Case("wide3-1to8", 3, (1,), 8, 3, 1, (5, 7, 19), [HINT_WIDE3], WIDE3),
    # register-weight ConvTranspose2d form
    Case("widet-8to16", 2, (8,), 16, 4, 2, (7, 21), _each(HINT_WIDET, 0, ROWS(1), ROWS(2)), WIDET, tr=True),
    Case("widet-16to1-res", 2, (16,), 1, 4, 2, (7, 21), [HINT_WIDET], WIDET, tr=True, epi="res", bn=False,
         act=ACT_NONE),
    # LDS-tiled 3-D form: plane pairs (8 couts) with both stagings and weight homes, the plane-pair hybrid (24) and
    # its padded MT variant, stride 2 with register / LDS weights, 1x1x1 over two sources, ConvTranspose3d
    Case("tile3-8to8", 3, (8,), 8, 3, 1, (5, 7, 19), _each(HINT_TILE, 0, ROWS(1), ROWS(2), ROWS(3),
         ROWS(1) | HINT_TILE_DMA_FLIP, HINT_TILE_WLDS), TILE3),
    Case("tile3-24to24", 3, (24,), 24, 3, 1, (5, 7, 19), _each(HINT_TILE, 0, ROWS(1), ROWS(2) | HINT_TILE_WLDS), TILE3),
    Case("tile3-s2-8to24", 3, (8,), 24, 3, 2, (5, 7, 19), _each(HINT_TILE, 0, ROWS(2), ROWS(3), HINT_TILE_DMA_FLIP,
         HINT_TILE_WLDS), TILE3),
    Case("tile3-k1-2src", 3, (24, 24), 24, 1, 1, (5, 7, 19), _each(HINT_TILE, 0, ROWS(1), ROWS(3)), TILE3),
    Case("tile3-convT", 3, (24,), 16, 4, 2, (3, 5, 9), _each(HINT_TILE, 0, ROWS(1), ROWS(3)), TILE3, tr=True),
    Case("tile3-mul-res-out2", 3, (8,), 8, 3, 1, (5, 7, 19), [HINT_TILE], TILE3, epi="mul res out2"),
    # LDS-tiled 2-D form
    Case("tile2-k3", 2, (16, 16), 32, 3, 1, (9, 23), _each(HINT_TILE, 0, ROWS(1), ROWS(2), ROWS(3)), TILE2),
    Case("tile2-k3s2", 2, (16, 16), 32, 3, 2, (9, 23), _each(HINT_TILE, 0, ROWS(1)), TILE2),
    Case("tile2-convT", 2, (16,), 16, 4, 2, (9, 23), _each(HINT_TILE, 0, ROWS(1), ROWS(3)), TILE2, tr=True),
    Case("tile2-res-out2", 2, (16, 16), 32, 3, 1, (9, 23), _each(HINT_TILE, 0, ROWS(2)), TILE2, epi="res out2"),
    # pointwise streaming form: whole contiguous planes, so batch and channel margins only; an "odd" base is
    # not 16-byte aligned and pw_ok hands the layer to the LDS-tiled 1x1 form the TILE3 bit names
    Case("pointwise-2d", 2, (16, 16), 16, 1, 1, (6, 20), [HINT_TILE | HINT_TILE_PW], PW, spatial=False,
         other={"odd": TILE2}),
    Case("pointwise-3d", 3, (16, 16), 16, 1, 1, (2, 6, 10), [HINT_TILE | HINT_TILE_PW], PW, spatial=False,
         other={"odd": TILE3}),
    # rows and columns embedded as well: never the pointwise form
    Case("pointwise-strided-planes", 2, (16, 16), 16, 1, 1, (6, 20), [HINT_TILE | HINT_TILE_PW], TILE2),
    # VALU single-output-channel ConvTranspose (the existing test_convt_c1_form stays): blocked and per-class forms
    Case("convt-c1-2d-up-out2", 2, (16,), 1, 4, 2, (7, 19), _each(HINT_C1T, 0, ROWS(1)), GENERAL, tr=True,
         epi="up out2", bn=False, act=ACT_NONE, post=4.0),
    Case("convt-c1-3d", 3, (12,), 1, 4, 2, (3, 7, 19), _each(HINT_C1T, 0, ROWS(1)), GENERAL, tr=True, bn=False,
         act=ACT_NONE),
    # general epilogues: PixelShuffle(4) (16-byte store / its scalar fall-back), bilinear add, * mul over D
    Case("epilogue-shuffle4", 2, (8,), 64, 1, 1, (9, 21), [0x11, 0x411, 0x211], GENERAL, shuffle=4, bn=False,
         act=ACT_SILU),
    Case("epilogue-bilinear", 2, (16,), 1, 3, 1, (10, 38), [0x11, 0x411, 0x211], GENERAL, epi="up", bn=False,
         act=ACT_NONE, post=4.0),
    Case("epilogue-mul-over-d", 3, (12,), 12, 3, 1, (5, 7, 21), [0x11, 0x211], GENERAL, epi="mul res out2"),
]


def conv_case(c):
    """A Case's layer and CPU operands: (packed conv, sources, epilogue operands by name, further run_conv keywords,
    fp64 reference, output shape).  Shared with tests/test_gpu_lds_poison.py."""
    conv, bn = _mk(c.nd, sum(c.cins), c.cout, c.k, c.s, c.p, transposed=c.tr, bn=c.bn, bias=not c.bn and c.shuffle > 1,
                   seed=sum(c.cins) + c.cout)
    g = torch.Generator().manual_seed(len(c.name) + c.cout)
    xs = [torch.randn(B, ci, *c.shape, generator=g) for ci in c.cins]
    plain = _ref_conv(xs, conv, bn, c.act, shuffle=c.shuffle)
    oshape = tuple(plain.shape)
    ops = {}
    if "mul" in c.epi:  # [B, Cout, Ho, Wo], broadcast over D
        ops["mul"] = torch.rand(oshape[:2] + oshape[-2:], generator=g) + 0.5
    if "res" in c.epi:
        ops["res"] = torch.randn(oshape, generator=g)
    if "up" in c.epi:
        ops["up"] = torch.randn(B, 1, oshape[-2] // 2, oshape[-1] // 2, generator=g)
    kw = dict(up_f=2) if "up" in c.epi else {}
    ref = _ref_conv(xs, conv, bn, c.act, shuffle=c.shuffle, **ops, **kw)
    return pk(conv, bn, c.act), xs, ops, kw, ref, oshape


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c.name)
def test_conv_layouts(case, where):
    c = case
    pc, xs, ops, kw, ref, oshape = conv_case(c)

    def operands(place):
        srcs = [x.to(DEV) if (place is None or i == c.loose) else _put(x, where, c.spatial) for i, x in enumerate(xs)]
        o = {k: (v.to(DEV) if place is None else _put(v, where, c.spatial)) for k, v in ops.items()}
        zero = torch.zeros(oshape)
        outs = [zero.to(DEV) if place is None else _put(zero, where, c.spatial) for _ in range(2 if "out2" in c.epi else 1)]
        return srcs, o, outs

    for hint in c.hints:
        what = f"{c.name} {where} hint {hint:#x}"
        srcs, o, outs = operands(where)
        ckw = dict(o, shuffle=c.shuffle, post_scale=c.post, hint=hint, **kw)
        if len(outs) == 2:
            assert outs[1].stride() == outs[0].stride()
            ckw.update(out2=outs[1], post_scale2=0.5)
        want = c.other.get(where, c.form)
        assert _form(pc, srcs, outs[0], **ckw) == want, what                                     # (c)
        snaps = [guard_snapshot(t) for t in outs]
        y = run_conv(Ctx(DEV), pc, srcs, outs[0], **ckw)
        torch.cuda.synchronize()
        _finite_close(y, ref * c.post, 1e-5, what)                                                 # (d)
        if len(outs) == 2:
            _finite_close(outs[1], ref * 0.5, 1e-5, what + " out2")
        for t, snap in zip(outs, snaps):
            assert_guards_intact(t, snap, what)                                                    # (e)
        csrcs, co, couts = operands(None)
        cckw = dict(ckw, **co)
        if len(couts) == 2:
            cckw.update(out2=couts[1])
        if _form(pc, csrcs, couts[0], **cckw) != want:
            continue  # another form runs the contiguous layout: its sum order is its own
        yc = run_conv(Ctx(DEV), pc, csrcs, couts[0], **cckw)
        assert torch.equal(y.contiguous(), yc), what + ": differs bitwise from the contiguous layout"  # (f)
        if len(outs) == 2:
            assert torch.equal(outs[1].contiguous(), couts[1]), what + " out2"


def test_conv_form_query_errors_and_automatic_rules():
    """esm_conv_form: the automatic rules' choice without a hint, a negative status (and the usual message) for a
    bad descriptor, nothing launched."""
    conv, bn = _mk(2, 16, 16, 3, 1, 1, seed=1)
    pc = pk(conv, bn, ACT_GELU)
    x = torch.randn(B, 16, 9, 37, device=DEV)
    out = torch.full((B, 16, 9, 37), 7.0, device=DEV)
    d, _, _ = EN._conv_desc(Ctx(DEV), pc, [x], out, hint=HINT_NO_TILE)  # NO_TILE alone: the automatic rules
    assert _lib.lib.esm_conv_form(ctypes.byref(d)) == SMALL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # a query, not a launch
    d.cin_pad = 8
    assert _lib.lib.esm_conv_form(ctypes.byref(d)) == -1 and b"cin_pad" in _lib.lib.esm_last_error()
    assert _lib.lib.esm_conv_form(None) == -1
    c3, b3 = _mk(3, 8, 8, 3, 1, 1, seed=2)
    x3 = torch.randn(1, 8, 5, 7, 19, device=DEV)
    assert _form(pk(c3, b3, ACT_GELU), [x3], None, hint=HINT_NO_TILE) == STEM  # 3-D 8-cout stems at every size
    # a forced form that cannot take the layer is reported as forced, and its launcher refuses
    with pytest.raises(E.EsmError):
        run_conv(Ctx(DEV), pk(c3, b3, ACT_GELU), [x3], hint=HINT_WIDET)


# ----------------------------------------------------------------------------- fused conv launches


def _check_out(y, ref, snaps, outs, what, tol=1e-5):
    torch.cuda.synchronize()
    _finite_close(y, ref, tol, what)
    for t, snap in zip(outs, snaps):
        assert_guards_intact(t, snap, what)


PAIR_CASES = [  # (name, nd, cins, kA, sA, pA, kB, coutB, shape, K-split form)
    ("lds-2src", 2, (16, 32), 3, 1, 1, 3, 16, (9, 21), False),
    ("ksplit-2src", 2, (16, 32), 3, 1, 1, 3, 16, (9, 21), True),
    ("lds-s2", 2, (16,), 3, 2, 1, 3, 16, (9, 21), False),
    ("ksplit-s2-12", 2, (12,), 3, 2, 1, 3, 12, (9, 21), True),
    ("lds-k5-head", 2, (1,), 5, 1, 1, 3, 16, (9, 21), False),
    ("lds-k1-3src", 2, (16, 16, 32), 1, 1, 0, 3, 16, (9, 21), False),
    ("ksplit-3d", 3, (16,), 3, 1, 1, 3, 16, (3, 6, 20), True),
    ("ksplit-3d-s2", 3, (16,), 3, 2, 1, 3, 16, (3, 6, 20), True),
]


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("name,nd,cins,ka,sa,pa,kb,coutb,shape,ksplit", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_conv_pair_layouts(name, nd, cins, ka, sa, pa, kb, coutb, shape, ksplit, where):
    """Two BasicConvs in one launch, LDS-staged (conv_pair2.hip) and K-split (conv_pairk.hip, 2-D and 3-D)."""
    from esmstereo_amd.engine import run_pair2
    ca, ba = _mk(nd, sum(cins), 16, ka, sa, pa, seed=31 + len(name))
    cb, bb = _mk(nd, 16, coutb, kb, 1, kb // 2, seed=32 + len(name))
    xs = [torch.randn(B, c, *shape) for c in cins]
    ref = _ref_conv([_ref_conv(xs, ca, ba, ACT_GELU)], cb, bb, ACT_GELU)
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    xe = [_put(x, where) for x in xs]
    out = _put(torch.zeros(ref.shape), where)
    snap = guard_snapshot(out)
    ctx = Ctx(DEV)
    y = run_pair2(ctx, pa_, xe, pb_, force=True, ksplit=ksplit, out=out)
    assert ctx.meta[-1]["kind"] == "conv_pair"  # one launch, the form asked for (run_pair2 raises if it cannot)
    _check_out(y, ref, [snap], [out], f"{name} {where}")
    yc = run_pair2(Ctx(DEV), pa_, [x.to(DEV) for x in xs], pb_, force=True, ksplit=ksplit)
    assert torch.equal(y.contiguous(), yc)


@pytest.mark.parametrize("where", PLACEMENTS)
def test_conv_pair_regress_layouts(where):
    """The regression source of the pair: the cost volume, the stored disparity map and the output all embedded."""
    from esmstereo_amd.engine import run_pair2
    D, H, W = 5, 7, 19
    ca, ba = _mk(2, 1, 16, 5, 1, 1, seed=41)
    cb, bb = _mk(2, 16, 16, 3, 1, 1, seed=42)
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    cost = torch.randn(B, D, H, W)
    rmap = (cost.double() * torch.arange(D, dtype=torch.float64).view(1, D, 1, 1)).sum(1, keepdim=True)
    ref = _ref_conv([_ref_conv([rmap], ca, ba, ACT_GELU)], cb, bb, ACT_GELU)
    coste = _put(cost, where)
    init = _put(torch.zeros(B, 1, H, W), where)
    out = _put(torch.zeros(ref.shape), where)
    snaps = [guard_snapshot(out), guard_snapshot(init)]
    ctx = Ctx(DEV)
    y = run_pair2(ctx, pa_, [init], pb_, force=True, regress=coste, out=out)
    assert ctx.meta[-1]["name"].startswith("disparity_regression+")  # the fused form, not a regression launch first
    _check_out(y, ref, snaps, [out, init], f"pair regress {where}")
    _finite_close(init, rmap.float(), 1e-6, "stored map")
    init_c = torch.zeros(B, 1, H, W, device=DEV)
    yc = run_pair2(Ctx(DEV), pa_, [init_c], pb_, force=True, regress=cost.to(DEV))
    assert torch.equal(y.contiguous(), yc) and torch.equal(init.contiguous(), init_c)


UP1_LAYOUT_CASES = [  # (name, nd, cin, cy, extra channels, coutb, input grid, crop, hint of the transposed conv)
    ("2d-lean", 2, 12, 12, (16,), 16, (11, 19), (21, 37), 0),
    ("2d-tiled", 2, 12, 12, (16,), 16, (11, 19), (21, 37), HINT_TILE | ROWS(2)),
    ("2d-tiled-rows1", 2, 12, 12, (16, 8), 16, (11, 19), (21, 37), HINT_TILE | ROWS(1)),
    ("3d-lean", 3, 24, 8, (4,), 12, (3, 7, 9), (5, 13, 17), 0),
    ("3d-lean-8waves", 3, 24, 8, (4,), 12, (3, 7, 9), (5, 13, 17), HINT_SMALL | HINT_SMALL_W8),
    ("3d-tiled", 3, 24, 8, (4,), 12, (3, 7, 9), (5, 13, 17), HINT_TILE | ROWS(1)),
    ("3d-tiled-two-cout-tiles", 3, 24, 20, (8, 4), 28, (3, 5, 9), (5, 9, 17), 0),
]


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("name,nd,cin,cy,cxs,coutb,grid,crop,hint", UP1_LAYOUT_CASES, ids=[c[0] for c in UP1_LAYOUT_CASES])
def test_convt_1x1_layouts(name, nd, cin, cy, cxs, coutb, grid, crop, hint, where):
    """ConvTranspose + crop + cat + 1x1 in one launch (conv_up1.hip), lean and LDS-tiled."""
    from esmstereo_amd.engine import convt_1x1_supported, run_convt_1x1
    ca, ba = _mk(nd, cin, cy, 4, 2, 1, transposed=True, seed=51 + cin)
    cb, bb = _mk(nd, cy + sum(cxs), coutb, 1, 1, 0, seed=52 + coutb)
    x = torch.randn(B, cin, *grid)
    xs = [torch.randn(B, c, *crop) for c in cxs]
    u = _ref_conv([x], ca, ba, ACT_GELU)
    u = u[(slice(None), slice(None)) + tuple(slice(0, n) for n in crop)]
    ref = _ref_conv([u, *xs], cb, bb, ACT_GELU)
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    assert convt_1x1_supported(pa_, pb_, xs)
    old = dict(EN.HINT_SET)
    EN.HINT_SET["convT"] = hint
    try:
        xe, xse = _put(x, where), [_put(t, where) for t in xs]
        out = _put(torch.zeros(ref.shape), where)
        snap = guard_snapshot(out)
        y = run_convt_1x1(Ctx(DEV), pa_, [xe], pb_, xse, out=out)
        _check_out(y, ref, [snap], [out], f"{name} {where}")
        yc = run_convt_1x1(Ctx(DEV), pa_, [x.to(DEV)], pb_, [t.to(DEV) for t in xs])
    finally:
        EN.HINT_SET.clear()
        EN.HINT_SET.update(old)
    assert torch.equal(y.contiguous(), yc)


@pytest.mark.parametrize("where", PLACEMENTS)
def test_gwc_stem_layouts(where):
    """gwc volume + group_stem in one launch: L and R carved (bare contiguous pointers), the output strided."""
    from esmstereo_amd.engine import run_gwc_stem
    G, D, H, W = 8, 5, 7, 20
    conv, bn = _mk(3, G, 8, 3, 1, 1, seed=G + D)
    L, R = feature_pair(B, 2 * G, H, W, 7, D)
    ref = _ref_conv([O.gwc_volume(L, R, D, G)], conv, bn, ACT_GELU)
    p = pk(conv, bn, ACT_GELU)
    for hint in (0, ROWS(2), ROWS(3), HINT_GWC_STEM_WLDS, ROWS(2) | HINT_GWC_STEM_WLDS):
        Lc, Rc = embed(L, "carved", DEV), embed(R, "carved", DEV)
        out = _put(torch.zeros(ref.shape), where)
        snap = guard_snapshot(out)
        y = run_gwc_stem(Ctx(DEV), p, Lc, Rc, G, D, hint=hint, out=out)
        _check_out(y, ref, [snap], [out], f"gwc_stem {where} hint {hint:#x}")
        assert torch.equal(y.contiguous(), run_gwc_stem(Ctx(DEV), p, L.to(DEV), R.to(DEV), G, D, hint=hint)), hex(hint)


# ----------------------------------------------------------------------------- upsampler heads, depthwise conv


def _head(nf, r, seed):
    torch.manual_seed(seed)
    up = torch.nn.Conv2d(nf, nf * r * r, 1, 1, 0)
    tail = torch.nn.Conv2d(nf, 1, 3, 1, 1)
    p = EN.pack_shuffle_tail(copy.deepcopy(up).to(DEV), copy.deepcopy(tail).to(DEV), r)

    def ref(x):
        return F.conv2d(F.silu(F.pixel_shuffle(F.conv2d(x.double(), up.weight.double(), up.bias.double()), r)),
                        tail.weight.double(), tail.bias.double(), 1, 1)
    return p, ref


SHUFFLE_TAIL_CASES = [(8, 4, 7, 21, (0, 1, 2, 3)), (16, 2, 5, 9, (0,)), (8, 2, 7, 21, (0,)), (16, 4, 5, 9, (0,))]
SHUFFLE_CONV_CASES = [(8, 4, 16, 7, 21, (0, 1, 2, 3)), (8, 2, 16, 7, 21, (0,)), (16, 2, 32, 5, 9, (0,))]
DWCONV_CASES = [(3, 1), (3, 2), (5, 1), (5, 2)]


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("nf,r,H,W,forms", SHUFFLE_TAIL_CASES)
def test_shuffle_tail_layouts(nf, r, H, W, forms, where):
    """upsampling + tail in one launch (shuffle_tail.hip), the window form and both row forms, x and out strided."""
    p, head = _head(nf, r, nf * 100 + r)
    x = torch.randn(B, nf, H, W)
    ref = head(x).float()
    for form in forms:
        xe = _put(x, where)
        out = _put(torch.zeros(ref.shape), where)
        snap = guard_snapshot(out)
        y = EN.run_shuffle_tail(Ctx(DEV), xe, p, out=out, form=form)
        _check_out(y, ref, [snap], [out], f"shuffle_tail {where} form {form}")
        assert torch.equal(y.contiguous(), EN.run_shuffle_tail(Ctx(DEV), x.to(DEV), p, form=form)), form


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("nf,r,C,H,W,forms", SHUFFLE_CONV_CASES)
def test_shuffle_conv_layouts(nf, r, C, H, W, forms, where):
    """The head + the refinement's first conv in one launch, x and out strided."""
    p, head = _head(nf, r, nf * 1000 + r * 10 + H)
    conv, bn = _mk(2, 1, C, 3, 2, 1, seed=H)
    pc = pk(conv, bn, ACT_GELU)
    x = torch.randn(B, nf, H, W)
    ref = _ref_conv([head(x)], conv, bn, ACT_GELU)
    for form in forms:
        xe = _put(x, where)
        out = _put(torch.zeros(ref.shape), where)
        snap = guard_snapshot(out)
        y = EN.run_shuffle_conv(Ctx(DEV), xe, p, pc, form=form, out=out)
        _check_out(y, ref, [snap], [out], f"shuffle_conv {where} form {form}")
        assert torch.equal(y.contiguous(), EN.run_shuffle_conv(Ctx(DEV), x.to(DEV), p, pc, form=form)), form


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("cp", [12, 16])
def test_shuffle_conv_pre_layouts(cp, where):
    """The row-form launch with the stage's spx conv computed inside it (pre_x), and with conv1[1] behind it."""
    H, W = 7, 21
    p, head = _head(8, 4, cp * 100 + H)
    pconv, pbn = _mk(2, cp, 8, 3, 1, 1, seed=H + 1)
    conv, bn = _mk(2, 1, 16, 3, 2, 1, seed=H)
    conv2, bn2 = _mk(2, 16, 16, 3, 1, 1, seed=H + 2)
    pc, pp, pc2 = pk(conv, bn, ACT_GELU), pk(pconv, pbn, ACT_GELU), pk(conv2, bn2, ACT_GELU)
    c = torch.randn(B, cp, H, W)
    ref = _ref_conv([head(_ref_conv([c], pconv, pbn, ACT_GELU))], conv, bn, ACT_GELU)
    ref2 = _ref_conv([ref.double()], conv2, bn2, ACT_GELU)
    for form, second in ((2, None), (3, None), (0, pc2)):
        want = ref if second is None else ref2
        ce = _put(c, where)
        out = _put(torch.zeros(want.shape), where)
        snap = guard_snapshot(out)
        y = EN.run_shuffle_conv(Ctx(DEV), ce, p, pc, pre=pp, form=form, conv2=second, out=out)
        _check_out(y, want, [snap], [out], f"shuffle_conv pre {where} form {form} conv2 {second is not None}")
        yc = EN.run_shuffle_conv(Ctx(DEV), c.to(DEV), p, pc, pre=pp, form=form, conv2=second)
        assert torch.equal(y.contiguous(), yc), (form, second is not None)


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("k,s", DWCONV_CASES)
def test_dwconv_layouts(k, s, where):
    """Depthwise conv (dwconv.hip), x and out strided, 5 channels."""
    torch.manual_seed(k * 10 + s)
    C, H, W = 5, 9, 21
    x = torch.randn(B, C, H, W)
    w = torch.randn(C, 1, k, k) * 0.3
    sc, sh = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    p = (k - 1) // 2 if s == 1 else ((s - 1) + (k - 1)) // 2
    ref = F.silu(F.conv2d(x.double(), w.double(), None, s, p, 1, C) * sc.double().view(1, C, 1, 1) +
                 sh.double().view(1, C, 1, 1)).float()
    args = (w.reshape(C, k * k).contiguous().to(DEV), sc.to(DEV), sh.to(DEV), k, s, p, ACT_SILU)
    xe = _put(x, where)
    out = _put(torch.zeros(ref.shape), where)
    snap = guard_snapshot(out)
    y = EN.run_dwconv(Ctx(DEV), xe, *args, out=out)
    _check_out(y, ref, [snap], [out], f"dwconv k{k} s{s} {where}")
    assert torch.equal(y.contiguous(), EN.run_dwconv(Ctx(DEV), x.to(DEV), *args))


# ----------------------------------------------------------------------------- bare-pointer entry points: carved


def _carve(t):
    return embed(t, "carved", DEV)


def _carved_out(*shape, dtype=torch.float32):
    out = embed(torch.zeros(shape, dtype=dtype), "carved", DEV)
    return out, guard_snapshot(out)


@pytest.mark.parametrize("C", [8, 16])
def test_smix_fmnet_carved(C):
    """ShuffleMixer launches (smix.hip) on buffers carved out of a poisoned arena: the whole FMBlock as one launch
    and as two, and the three smix launches, vs the fp64 oracle (1e-5) and bitwise vs fresh tensors."""
    H, W = 7, 13
    torch.manual_seed(7)
    blk = E.FMBlock(C, 7, 2).eval()
    with torch.no_grad():
        for n, prm in blk.named_parameters():
            if n.endswith("norm1.body.weight") or n.endswith("norm2.body.weight"):
                prm.uniform_(0.8, 1.2)
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    x = torch.randn(B, C, H, W)
    ref = O.fm_block(sd, "", x)
    p = blk.to(DEV)._packed()
    st = [p["a1"], p["a2"], p["b1"], p["b2"]]
    xd = x.to(DEV)
    for two in (False, True):
        out, snap = _carved_out(B, C, H, W)
        work, wsnap = _carved_out(B, C, H, W)  # the two-launch form's scratch buffer (smix.hip fm2a / fm2b)
        y = EN.run_fmnet(Ctx(DEV), _carve(x), st, p["dw0"], p["dw1"], out=out, conv=p["cw"], two_launch=two, work=work)
        _check_out(y, ref, [snap, wsnap], [out, work], f"fmnet whole block, two launches {two}")
        assert torch.equal(y, EN.run_fmnet(Ctx(DEV), xd, st, p["dw0"], p["dw1"], conv=p["cw"], two_launch=two)), two
    net, snap = _carved_out(B, C, H, W)
    EN.run_fmnet(Ctx(DEV), _carve(x), st, p["dw0"], p["dw1"], out=net)
    torch.cuda.synchronize()
    assert_guards_intact(net, snap, "fmnet net")
    ctx = Ctx(DEV)
    xc = _carve(x)
    outs = [_carved_out(B, C, H, W) for _ in range(3)]
    t1 = EN.run_smix(ctx, xc, [p["a1"]], out=outs[0][0])
    t2 = EN.run_smix(ctx, t1, [p["a2"], p["b1"]], dw=p["dw0"], out=outs[1][0])
    t3 = EN.run_smix(ctx, t2, [p["b2"]], dw=p["dw1"], res=xc, out=outs[2][0])
    torch.cuda.synchronize()
    for t, snap in outs:
        assert bool(torch.isfinite(t).all())
        assert_guards_intact(t, snap, "smix")
    assert rel(net, t3) < 1e-6  # as test_fmnet_fused_bitwise
    assert rel(EN.run_conv(ctx, p["c2"], [EN.run_conv(ctx, p["c0"], [t3])], res=t3), ref) < 1e-5
    u1 = EN.run_smix(ctx, xd, [p["a1"]])
    u3 = EN.run_smix(ctx, EN.run_smix(ctx, u1, [p["a2"], p["b1"]], dw=p["dw0"]), [p["b2"]], dw=p["dw1"], res=xd)
    assert torch.equal(t1, u1) and torch.equal(t3, u3)


def test_volumes_carved():
    """Cost volumes and regressions (volumes.hip, regression.hip) on carved buffers, H x W = 5 x 19, D 9: the
    tolerances of test_ops_golden / test_volumes_vs_oracle / test_regression_topk_any_k."""
    C, G, D, H, W = 16, 8, 9, 5, 19
    L, R = feature_pair(B, C, H, W, 5, D)
    att = torch.rand(B, G, H, W) + 0.5
    ctx = Ctx(DEV)
    V, snap = _carved_out(B, G, D, H, W)
    ctx.gwc(_carve(L), _carve(R), None, V, B, C, H, W, D, G)
    torch.cuda.synchronize()
    assert_guards_intact(V, snap, "gwc")
    assert torch.equal(V.cpu(), O.gwc_volume(L, R, D, G))  # 2-channel groups: bit-exact
    Va, snap = _carved_out(B, G, D, H, W)
    ctx.gwc(_carve(L), _carve(R), _carve(att), Va, B, C, H, W, D, G)
    torch.cuda.synchronize()
    assert_guards_intact(Va, snap, "gwc * att")
    assert bool(torch.isfinite(Va).all())
    assert torch.equal(Va, E.build_gwc_volume(L.to(DEV), R.to(DEV), D, G, att=att.to(DEV)))
    assert rel(Va, O.gwc_volume(L, R, D, G).double() * att.double().unsqueeze(2)) < 1e-6
    Vc, snap = _carved_out(B, 2 * C, D, H, W)
    ctx.concat(_carve(L), _carve(R), Vc, B, C, H, W, D)
    torch.cuda.synchronize()
    assert_guards_intact(Vc, snap, "concat")
    assert torch.equal(Vc.cpu(), O.concat_volume(L, R, D))
    Vn, snap = _carved_out(B, 1, D, H, W)
    work, wsnap = _carved_out(2, B, C, H, W)
    ctx.normcorr(_carve(L), _carve(R), Vn, work, B, C, H, W, D)
    torch.cuda.synchronize()
    assert_guards_intact(Vn, snap, "normcorr")
    assert_guards_intact(work, wsnap, "normcorr work")
    _finite_close(Vn, O.normcorr_volume(L, R, D), 1e-5, "normcorr")
    assert torch.equal(Vn, E.build_norm_correlation_volume(L.to(DEV), R.to(DEV), D))

    g = torch.Generator().manual_seed(3)
    cost = torch.randn(B, D, H, W, generator=g)
    cost[0, 2, 0, :4] = cost[0, 6, 0, :4] = 10.0  # exact ties
    samples = torch.rand(B, D, H, W, generator=g) * D
    r, snap = _carved_out(B, 1, H, W)
    ctx.regression(0, _carve(cost), r, B, D, H, W)
    torch.cuda.synchronize()
    assert_guards_intact(r, snap, "disparity_regression")
    _finite_close(r[:, 0], O.disparity_regression(cost, D), 1e-6, "disparity_regression")
    assert torch.equal(r[:, 0], E.disparity_regression(cost.to(DEV), D))
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for smp in (None, samples):
        t2, snap = _carved_out(B, 1, H, W)
        sc = _carve(smp) if smp is not None else None
        cc = _carve(cost)
        _lib.check(_lib.lib.esm_topk2_regression_f32(cc.data_ptr(), sc.data_ptr() if sc is not None else None,
                                                     t2.data_ptr(), B, D, H, W, stream), "topk2")
        torch.cuda.synchronize()
        assert_guards_intact(t2, snap, "topk2")
        _finite_close(t2, O.regression_topk(cost, smp, 2), 1e-6, "topk2")
        for k in (3, 9):
            tk, snap = _carved_out(B, 1, H, W)
            ctx.regression(1, cc, tk, B, D, H, W, samples=sc, k=k)
            torch.cuda.synchronize()
            assert_guards_intact(tk, snap, f"topk{k}")
            _finite_close(tk, O.regression_topk(cost, smp, k), 1e-6, f"topk{k}")
            assert torch.equal(tk, E.regression_topk(cost.to(DEV), None if smp is None else smp.to(DEV), k))


def test_confidence_ops_carved():
    """The five esm_conf_f32 stages on carved operands, the bounds of test_gpu_confidence.py."""
    from esmstereo_amd._lib import CONF_ATTEND, CONF_COMBINE, CONF_COST_FEATURES, CONF_ENLARGE, CONF_SIGMOID
    from oracle import conf_oracle as CO
    g = torch.Generator().manual_seed(5)
    C, D, H, W = 5, 9, 5, 19

    def stage(op, xs, oshape, c, d, h, w, want, tol, what):
        out, snap = _carved_out(*oshape)
        Ctx(DEV).conf(op, [_carve(x) for x in xs], out, B, c, d, h, w)
        plain = torch.empty(oshape, device=DEV)
        Ctx(DEV).conf(op, [x.to(DEV) for x in xs], plain, B, c, d, h, w)
        torch.cuda.synchronize()
        assert_guards_intact(out, snap, what)
        assert bool(torch.isfinite(out).all()), what
        assert float((out.double().cpu() - want.double()).abs().max()) < tol, what
        assert torch.equal(out, plain), what

    cost = torch.randn(B, D, H, W, generator=g)
    stage(CONF_COST_FEATURES, [cost], (B, 7, H, W), 0, D, H, W, CO.cost_features(cost), 2e-6, "cost features")
    xs = [torch.randn(B, C, H, W, generator=g) for _ in range(3)]
    lg = torch.randn(B, 3, H, W, generator=g)
    a = F.softmax(lg, 1)
    stage(CONF_ATTEND, xs + [lg], (B, 3 * C, H, W), C, 0, H, W, torch.cat([xs[k] * a[:, k:k + 1] for k in range(3)], 1),
          1e-6, "attend")
    feat = torch.randn(B, C, H, W, generator=g)
    scale = 2 * torch.sigmoid(3 * torch.randn(B, 1, H, W, generator=g))
    big = F.grid_sample(feat, CO.enlarge_grid(scale), align_corners=True)
    s2d = big.view(B, C, H, 3, W, 3).permute(0, 1, 3, 5, 2, 4).reshape(B, 9 * C, H, W)
    stage(CONF_ENLARGE, [feat, scale], (B, 9 * C, H, W), C, 0, H, W, s2d, 2e-5, "enlarge")
    lg9 = torch.randn(B, 9, 4 * H, 4 * W, generator=g)
    init = torch.randn(B, 1, H, W, generator=g)
    unf = F.unfold(init, 3, 1, 1).reshape(B, -1, H, W)
    unf = F.interpolate(unf, (4 * H, 4 * W), mode="nearest").reshape(B, 9, 4 * H, 4 * W)
    stage(CONF_COMBINE, [lg9, init], (B, 1, 4 * H, 4 * W), 0, 0, H, W, (unf * F.softmax(lg9, 1)).sum(1).unsqueeze(1),
          2e-6, "combine")
    x = torch.randn(B, 1, H, W, generator=g) * 8
    stage(CONF_SIGMOID, [x], (B, 1, H, W), 1, 0, H, W, torch.sigmoid(x), 1e-7, "sigmoid")


def test_io_carved():
    """Input / output kernels (io.hip) on carved u8 / u16 / float buffers with byte sentinels: bit-exact vs the
    oracle (test_gpu_io.py, test_node.py)."""
    import numpy as np
    from oracle import io_oracle as IO
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    h, w = 37, 61
    u8 = np.random.default_rng(3).integers(0, 256, size=(B, h, w, 3), dtype=np.uint8)
    refs = [IO.kitti_test_transform(u8[b]) for b in range(B)]
    top, left = refs[0][1]
    Hp, Wp = h + top, w + left
    img = _carve(torch.from_numpy(u8))
    out, snap = _carved_out(B, 3, Hp, Wp)
    _lib.check(_lib.lib.esm_preprocess_u8(img.data_ptr(), out.data_ptr(), B, h, w, Hp, Wp, top, left, 1, stream), "preprocess")
    torch.cuda.synchronize()
    assert_guards_intact(out, snap, "preprocess")
    for b in range(B):
        assert np.array_equal(out[b].cpu().numpy(), refs[b][0])

    g = torch.Generator().manual_seed(5)
    d = torch.rand(B, Hp, Wp, generator=g) * 200
    d[0, top + 1, left:left + 8] = torch.tensor([0.0, 1 / 512, 3 / 512, 5 / 512, 100.25, 7 / 512, 255.998, 2.5 / 256])
    dc = _carve(d)
    u16, snap = _carved_out(B, h, w, dtype=torch.int16)
    _lib.check(_lib.lib.esm_disp_to_u16(dc.data_ptr(), u16.data_ptr(), B, Hp, Wp, top, left, h, w, stream), "disp_to_u16")
    torch.cuda.synchronize()
    assert_guards_intact(u16, snap, "disp_to_u16")
    assert np.array_equal(u16.view(torch.uint16).cpu().numpy(), IO.disp_to_u16(d.numpy(), top, left, h, w))

    d[:, ::7, ::5] = -1.0   # values the node's range mask drops
    d[:, 3::11, 2::9] = 250.0
    dc = _carve(d)
    u16, snap = _carved_out(B, h, w, dtype=torch.int16)
    filt, fsnap = _carved_out(B, h, w)
    _lib.check(_lib.lib.esm_node_filter_u16(dc.data_ptr(), u16.data_ptr(), filt.data_ptr(), B, Hp, Wp, top, left, h, w,
                                            192.0, stream), "node filter")
    torch.cuda.synchronize()
    assert_guards_intact(u16, snap, "node filter u16")
    assert_guards_intact(filt, fsnap, "node filter map")
    for b in range(B):
        ru16, rf = IO.node_filter_u16(d[b].numpy(), top, left, h, w, 192.0)
        assert np.array_equal(u16[b].view(torch.uint16).cpu().numpy(), ru16)
        assert np.array_equal(filt[b].cpu().numpy(), rf)
