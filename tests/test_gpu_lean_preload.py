"""The lean form behind its first-load record (conv_small.hip lconv_rec_kernel / lconv_up1_rec_kernel, conv_lean_rec.h).

A lean launch whose layer the 14-dword record describes reads everything ahead of its first loads from the kernel's
leading scalar arguments, and its BN constants through the weight pointer; HINT_SMALL_NO_RECORD keeps the
struct-argument kernel.  Both run the same loads, MFMAs, LDS sums and epilogue expressions, so every case is checked
* against fp64 torch at relative 1e-5 (the bound of the conv tests),
* against the struct-argument kernel bitwise,
* against itself on a second run bitwise,
at batch 2, on odd-strided views inside poisoned allocations (layouts.py), at the smallest shapes that reach each
code path.  Which kernel a descriptor runs is asserted through esm_lean_record_pack.
"""
from __future__ import annotations

import ctypes

import pytest
import torch

from layouts import assert_guards_intact, embed, guard_snapshot
from test_gpu_parity import _mk, _ref_conv, pk, rel

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd._lib import (HINT_SMALL, HINT_SMALL_NO_RECORD, HINT_SMALL_NO_ZSPLIT, HINT_SMALL_W8,  # noqa: E402
                                HINT_XCD_SLAB, lib)
from esmstereo_amd.engine import ACT_GELU, ACT_NONE, Ctx, run_conv, run_convt_1x1  # noqa: E402

DEV = torch.device("cuda")
B = 2


def behind_record(d) -> bool:
    rec, fields = (ctypes.c_uint32 * 14)(), (ctypes.c_int64 * 19)()
    rc = lib.esm_lean_record_pack(ctypes.byref(d), rec, fields)
    assert rc in (0, 1)
    return rc == 1


CASES = [  # (name, nd, source channels, cout, k, stride, pad, input extent, extra hint bits, runs behind the record)
    ("2d 3x3 s1, ragged second column tile", 2, (16,), 16, 3, 1, 1, (5, 19), 0, True),
    ("2d 3x3 s2", 2, (16,), 16, 3, 2, 1, (13, 21), 0, True),
    ("2d 1x1", 2, (24,), 12, 1, 1, 0, (3, 17), 0, True),
    ("2d 5x5, one input channel", 2, (1,), 16, 5, 1, 2, (6, 18), 0, True),
    ("3d s2: tap-plane split, G 2, 8 waves", 3, (8,), 12, 3, 2, 1, (4, 6, 18), 0, True),
    ("3d s1: G 3, 12 waves", 3, (12,), 12, 3, 1, 1, (2, 3, 10), 0, True),
    ("3d s1: G 6, two cout tiles, 16 waves", 3, (24,), 24, 3, 1, 1, (2, 3, 10), 0, True),
    ("3d s1: G 7, the plain loop", 3, (28,), 8, 3, 1, 1, (2, 3, 10), 0, True),
    ("3d s1: the plain loop forced", 3, (12,), 12, 3, 1, 1, (2, 3, 10), HINT_SMALL_NO_ZSPLIT, True),
    ("3d: a one-plane volume", 3, (8,), 8, 3, 1, 1, (1, 5, 19), 0, True),
    ("2d 3x3, 8 waves", 2, (24,), 16, 3, 1, 1, (5, 19), HINT_SMALL_W8, True),
    ("2d 3x3, XCD slab order", 2, (16,), 16, 3, 1, 1, (5, 19), HINT_XCD_SLAB, True),
    ("2d 3x3 over two sources: the struct-argument kernel", 2, (16, 8), 16, 3, 1, 1, (5, 19), 0, False),
]


def run_case(p, xs, ref, hint, **kw):
    out = embed(torch.zeros(ref.shape), "odd", DEV)
    snap = guard_snapshot(out)
    y = run_conv(Ctx(DEV), p, xs, out, hint=hint, **kw)
    torch.cuda.synchronize()
    assert_guards_intact(out, snap, "odd")
    return y.contiguous().clone()


@pytest.mark.parametrize("name,nd,cins,cout,k,s,pad,ext,bits,record", CASES, ids=[c[0] for c in CASES])
def test_lean_record_conv(name, nd, cins, cout, k, s, pad, ext, bits, record):
    conv, bn = _mk(nd, sum(cins), cout, k, s, pad, seed=11 + sum(cins) + k)
    xs = [torch.randn(B, c, *ext) for c in cins]
    ref = _ref_conv(xs, conv, bn, ACT_GELU)
    p = pk(conv, bn, ACT_GELU)
    xd = [embed(x, "odd", DEV) for x in xs]
    hint = HINT_SMALL | bits
    assert behind_record(EN._conv_desc(Ctx(DEV), p, xd, hint=hint)[0]) == record
    assert not behind_record(EN._conv_desc(Ctx(DEV), p, xd, hint=hint | HINT_SMALL_NO_RECORD)[0])
    y = run_case(p, xd, ref, hint)
    assert bool(torch.isfinite(y).all()), "a value from outside the logical extent reached the output"
    assert rel(y, ref) < 1e-5
    assert torch.equal(y, run_case(p, xd, ref, hint | HINT_SMALL_NO_RECORD))
    assert torch.equal(y, run_case(p, xd, ref, hint))


@pytest.mark.parametrize("nd,ext", [(2, (3, 10)), (3, (1, 3, 10))], ids=["2d", "3d"])
def test_lean_record_transposed(nd, ext):
    conv, bn = _mk(nd, 16, 12, 4, 2, 1, transposed=True, seed=23 + nd)
    x = torch.randn(B, 16, *ext)
    ref = _ref_conv([x], conv, bn, ACT_GELU)
    p = pk(conv, bn, ACT_GELU)
    xd = [embed(x, "odd", DEV)]
    assert behind_record(EN._conv_desc(Ctx(DEV), p, xd, hint=HINT_SMALL)[0])
    y = run_case(p, xd, ref, HINT_SMALL)
    assert bool(torch.isfinite(y).all())
    assert rel(y, ref) < 1e-5
    assert torch.equal(y, run_case(p, xd, ref, HINT_SMALL | HINT_SMALL_NO_RECORD))
    assert torch.equal(y, run_case(p, xd, ref, HINT_SMALL))


def test_lean_record_residual_second_output():
    """The general epilogue (residual, second copy, no folded activation) behind the record; a bias-only layer, so the
    record carries no scale."""
    conv, _ = _mk(2, 16, 16, 3, 1, 1, bias=True, bn=False, seed=31)
    x, res = torch.randn(B, 16, 5, 19), torch.randn(B, 16, 5, 19)
    ref = _ref_conv([x], conv, None, ACT_NONE, res=res)
    p = pk(conv, None, ACT_NONE)
    xd, rd = [embed(x, "odd", DEV)], embed(res, "odd", DEV)
    d = EN._conv_desc(Ctx(DEV), p, xd, res=rd, out2=torch.empty(ref.shape, device=DEV), post_scale2=0.5, hint=HINT_SMALL)[0]
    assert behind_record(d)
    got = {}
    for key, hint in (("rec", HINT_SMALL), ("struct", HINT_SMALL | HINT_SMALL_NO_RECORD), ("again", HINT_SMALL)):
        out2 = embed(torch.zeros(ref.shape), "odd", DEV)
        snap2 = guard_snapshot(out2)
        y = run_case(p, xd, ref, hint, res=rd, out2=out2, post_scale2=0.5)
        assert_guards_intact(out2, snap2, "odd")
        got[key] = (y, out2.contiguous().clone())
    y, y2 = got["rec"]
    assert rel(y, ref) < 1e-5 and rel(y2, 0.5 * ref) < 1e-5
    for other in ("struct", "again"):
        assert torch.equal(y, got[other][0]) and torch.equal(y2, got[other][1])


@pytest.mark.parametrize("nd,grid,crop", [(2, (3, 10), (5, 19)), (3, (1, 3, 10), (2, 5, 19))], ids=["2d", "3d"])
def test_lean_record_convt_1x1(nd, grid, crop):
    """The fused ConvTranspose + 1x1 in the lean form, with two extra sources and a cropped skip."""
    ca, ba = _mk(nd, 16, 12, 4, 2, 1, transposed=True, seed=41 + nd)
    cb, bb = _mk(nd, 12 + 8 + 4, 12, 1, 1, 0, seed=43 + nd)
    x = torch.randn(B, 16, *grid)
    xs = [torch.randn(B, c, *crop) for c in (8, 4)]
    u = _ref_conv([x], ca, ba, ACT_GELU)[(slice(None), slice(None)) + tuple(slice(0, n) for n in crop)]
    ref = _ref_conv([u, *xs], cb, bb, ACT_GELU)
    pa, pb = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    xd, xsd = embed(x, "odd", DEV), [embed(t, "odd", DEV) for t in xs]
    assert EN.convt_1x1_supported(pa, pb, xsd)
    old = dict(EN.HINT_SET)
    got = []
    try:
        for hint, record in ((HINT_SMALL, True), (HINT_SMALL | HINT_SMALL_NO_RECORD, False), (HINT_SMALL, True)):
            EN.HINT_SET["convT"] = hint
            assert behind_record(EN._conv_desc(Ctx(DEV), pa, [xd], tag="convT", alloc_out=False)[0]) == record
            out = embed(torch.zeros(ref.shape), "odd", DEV)
            snap = guard_snapshot(out)
            ctx = Ctx(DEV)
            y = run_convt_1x1(ctx, pa, [xd], pb, xsd, out=out)
            torch.cuda.synchronize()
            assert ctx.meta[-1]["form"] == "lean"
            assert_guards_intact(out, snap, "odd")
            got.append(y.contiguous().clone())
    finally:
        EN.HINT_SET.clear()
        EN.HINT_SET.update(old)
    assert bool(torch.isfinite(got[0]).all())
    assert rel(got[0], ref) < 1e-5
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


def test_lean_record_hot_path_S():
    """The S hot path at the fixture size, with the record on and off, eager and as a replayed graph, before and
    after a rebind to new input tensors: every output bitwise equal."""
    from helpers import load_golden
    from test_gpu_parity import _model_from_manifest, cu
    g = load_golden("hot_S_gwc.npz")
    ml, mr, att = cu(g["match_left"]), cu(g["match_right"]), cu(g["att"])
    up = [cu(g[f"up_{i}"]) for i in range(sum(1 for k in g if k.startswith("up_")))]
    ml2, mr2, up2 = ml * 1.1, mr.clone(), [u + 0.01 for u in up]  # fresh allocations: the bound pointers move
    outs = {}
    old = EN.SMALL_RECORD
    try:
        for record in (True, False):
            for graph in (True, False):
                EN.SMALL_RECORD = record
                model, _, _ = _model_from_manifest("hot_S_gwc.npz")
                model.use_graph = graph
                with torch.no_grad():
                    first = [t.clone() for t in model.hot_path(ml, mr, att, up)]
                    moved = [t.clone() for t in model.hot_path(ml2, mr2, att, up2)]
                hints = [m.get("hint", 0) for hp in model._plans.values() for m in hp.ctx.meta]
                assert any(h & HINT_SMALL and h & HINT_SMALL_NO_RECORD for h in hints) != record
                outs[(record, graph)] = first + moved
    finally:
        EN.SMALL_RECORD = old
    want = outs[(True, True)]
    assert not torch.equal(want[0], want[len(want) // 2])  # the rebound inputs were read
    for key, got in outs.items():
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), key
