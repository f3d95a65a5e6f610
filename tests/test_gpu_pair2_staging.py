"""The LDS pair behind its staging record (conv_pair2.hip pair2_rec_kernel / P2Stage, conv_pair2_rec.h).

A pair the 20-dword record describes issues every staging load from the kernel's leading scalar arguments: the
input window through per-thread slots fixed once and a wave-uniform channel offset, both weight slabs in 16-byte
pieces, the BN constants through the weight pointers.  HINT_PAIR_NO_RECORD keeps the struct-argument prologue.  Both
leave the same LDS image in front of the same MFMA phases and epilogues, so every case is checked
* against the struct-argument kernel bitwise (the stored regression map too),
* against fp64 torch at relative 1e-5 (the bound of the conv tests),
at batch 2, for each (kA, sA, kB) of the form and each tile height the launcher can pick, at the smallest shapes at
which staging can go wrong: a map narrower than one tile (W 9), one column wider than whole tiles (W 15, 29, 79; the
tiles are 14 or 16 columns), H no multiple of the tile rows (7, 25), Cin 1 / 16 / 48 over three sources, convB with
5 and 16 couts, odd-strided views inside poisoned allocations (layouts.py), D 5 and 12 for the regression source.
Which kernel a launch runs is asserted through esm_pair2_record_pack on the descriptors the launch was given.

The issue's condition for the linear weight copy (cin_pad == CINMAX and cout_pad == 16) never holds for weights
engine.pack_weight packs (cout_pad is a multiple of 32, cin_pad of 16, so the heads' CINMAX 4 never matches); the
record takes pack_weight's own layout instead (cin_pad = Cin rounded up to 16, cout_pad 32) and copies 64-byte rows.
A cin_pad other than that -- 32 for 16 channels below, != CINMAX 16 -- and BN constants outside the weights'
allocation run the struct-argument kernel through the default entry."""
from __future__ import annotations

import ctypes
import dataclasses
import itertools

import pytest
import torch

from layouts import assert_guards_intact, embed, guard_snapshot
from test_gpu_parity import _mk, _ref_conv, pk, rel

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd._lib import lib  # noqa: E402
from esmstereo_amd.engine import ACT_GELU, Ctx, PackedConv, run_pair2  # noqa: E402

DEV = torch.device("cuda")
B = 2
SHAPES = [(7, 9), (7, 15), (25, 29), (7, 79)]  # (H, W)
FORMS = [(5, 1, 3), (3, 1, 1), (3, 1, 3), (1, 1, 3), (3, 2, 3)]  # (kA, sA, kB); (5, 1, 3) + regress: its own test
CINS = [(1,), (16,), (16, 12, 20)]  # 48 over three sources split at 4-channel boundaries


def behind_record(da, db) -> bool:
    rec, fields = (ctypes.c_uint32 * 20)(), (ctypes.c_int64 * 24)()
    rc = lib.esm_pair2_record_pack(ctypes.byref(da), ctypes.byref(db), rec, fields)
    assert rc in (0, 1)
    return rc == 1


class Spy(Ctx):
    """An eager context that notes, per pair launch, whether it ran behind the record."""

    def __init__(self):
        super().__init__(DEV)
        self.record = []

    def pair2(self, a, b):
        self.record.append(behind_record(a, b))
        super().pair2(a, b)


def run(pa, xs, pb, sel, record, out, regress=None):
    """One forced LDS-form launch with tile rows ROWS(sel), behind the record or not -> (output copy, ran behind it)."""
    old = EN.PAIR2_RECORD, dict(EN.PAIR2_TH)
    try:
        EN.PAIR2_RECORD = record
        EN.PAIR2_TH.update({s: (("convA",) if s == sel else ()) for s in (1, 2, 3)})
        ctx = Spy()
        snap = guard_snapshot(out)
        y = run_pair2(ctx, pa, xs, pb, force=True, ksplit=False, regress=regress, out=out)
        torch.cuda.synchronize()
        assert_guards_intact(out, snap, "pair output")
        assert len(ctx.record) == 1 and ctx.meta[-1]["kind"] == "conv_pair"
        return y.contiguous().clone(), ctx.record[0]
    finally:
        EN.PAIR2_RECORD = old[0]
        EN.PAIR2_TH.clear()
        EN.PAIR2_TH.update(old[1])


_REFS = {}


def case(ka, sa, kb, cins, coutb, H, W):
    """(packed convA, packed convB, CPU sources, fp64 reference), built once per case."""
    key = (ka, sa, kb, cins, coutb, H, W)
    if key not in _REFS:
        pa_ = {5: 2, 3: 1, 1: 0}[ka]
        ca, ba = _mk(2, sum(cins), 16, ka, sa, pa_, seed=7 + ka + sum(cins))
        cb, bb = _mk(2, 16, coutb, kb, 1, kb // 2, seed=9 + kb + coutb)
        g = torch.Generator().manual_seed(H * 100 + W)
        xs = [torch.randn(B, c, H, W, generator=g) for c in cins]
        ref = _ref_conv([_ref_conv(xs, ca, ba, ACT_GELU)], cb, bb, ACT_GELU)
        _REFS[key] = (pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU), xs, ref)
    return _REFS[key]


def tile_sels(cins):
    return (1, 2, 3) if sum(cins) <= 16 else (1, 2)  # 8-row tiles: up to 16 input channels


# every form x tile height x channel layout, the shapes and convB's couts dealt round-robin over them, then
# every shape and both couts on each form's 16-channel, 4-row kernel
CASES = []
for n, ((ka, sa, kb), cins) in enumerate(itertools.product(FORMS, CINS)):
    for m, sel in enumerate(tile_sels(cins)):
        H, W = SHAPES[(n + m) % len(SHAPES)]
        CASES.append((ka, sa, kb, cins, (5, 16)[(n + m) % 2], H, W, sel, ("odd", "plain")[(n + m) % 2]))
for n, (ka, sa, kb) in enumerate(FORMS):
    for m, (H, W) in enumerate(SHAPES):
        c = (ka, sa, kb, (16,), (16, 5)[(n + m) % 2], H, W, 2, ("plain", "odd")[m % 2])
        if c not in CASES:
            CASES.append(c)


def _id(c):
    ka, sa, kb, cins, coutb, H, W, sel, where = c
    return f"k{ka}s{sa}+k{kb}-cin{'+'.join(map(str, cins))}-cout{coutb}-{H}x{W}-rows{2 << (sel - 1)}-{where}"


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_pair2_record_matches_struct_kernel(c):
    ka, sa, kb, cins, coutb, H, W, sel, where = c
    pa, pb, xs, ref = case(ka, sa, kb, cins, coutb, H, W)
    put = (lambda t: embed(t, "odd", DEV)) if where == "odd" else (lambda t: t.to(DEV))
    xd = [put(x) for x in xs]
    y, rec = run(pa, xd, pb, sel, True, put(torch.zeros(ref.shape)))
    assert rec, "the record describes this pair"
    assert bool(torch.isfinite(y).all()), "a value from outside the logical extent reached the output"
    y0, rec0 = run(pa, xd, pb, sel, False, put(torch.zeros(ref.shape)))
    assert not rec0
    err = rel(y, ref)
    print(f"{_id(c)}: rel {err:.3g}, equal {torch.equal(y, y0)}")
    assert torch.equal(y, y0)
    assert err < 1e-5


REG_CASES = [(D, H, W, sel, where) for (D, (H, W), sel, where) in
             [(5, (7, 9), 1, "odd"), (12, (7, 15), 2, "plain"), (5, (25, 29), 3, "odd"), (12, (7, 79), 1, "plain"),
              (12, (25, 29), 2, "odd"), (5, (7, 79), 3, "plain")]]


@pytest.mark.parametrize("D,H,W,sel,where", REG_CASES)
def test_pair2_record_regress(D, H, W, sel, where):
    """The regression source: the stored map and the pair's output bitwise the struct-argument kernel's."""
    ca, ba = _mk(2, 1, 16, 5, 1, 2, seed=41 + W)
    cb, bb = _mk(2, 16, 16, 3, 1, 1, seed=42 + H)
    pa, pb = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    cost = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(D + W))
    rmap = (cost.double() * torch.arange(D, dtype=torch.float64).view(1, D, 1, 1)).sum(1, keepdim=True)
    ref = _ref_conv([_ref_conv([rmap], ca, ba, ACT_GELU)], cb, bb, ACT_GELU)
    put = (lambda t: embed(t, "odd", DEV)) if where == "odd" else (lambda t: t.to(DEV))
    costd = put(cost)
    got = {}
    for record in (True, False):
        init = put(torch.full((B, 1, H, W), float("nan")))
        snap = guard_snapshot(init)
        y, rec = run(pa, [init], pb, sel, record, put(torch.zeros(ref.shape)), regress=costd)
        assert_guards_intact(init, snap, "stored map")
        assert rec == record
        got[record] = (y, init.contiguous().clone())
    y, m = got[True]
    print(f"regress D{D} {H}x{W} rows{2 << (sel - 1)} {where}: rel {rel(y, ref):.3g}, map rel {rel(m, rmap.float()):.3g}")
    assert torch.equal(y, got[False][0]) and torch.equal(m, got[False][1])
    assert rel(m, rmap.float()) < 1e-6 and rel(y, ref) < 1e-5


def _moved_bn(p: PackedConv) -> PackedConv:
    """The same layer with its BN constants in allocations of their own."""
    return dataclasses.replace(p, scale=p.scale.clone(), shift=p.shift.clone())


def _wider_cin_pad(p: PackedConv, cin_pad: int) -> PackedConv:
    """The same layer packed with more zero rows per tap: [taps][cin_pad][cout_pad] | scale | shift."""
    taps, old, cout_pad = p.w.shape
    n = taps * cin_pad * cout_pad
    buf = torch.zeros(n + 2 * cout_pad, device=p.w.device)
    w = buf[:n].view(taps, cin_pad, cout_pad)
    w[:, :old] = p.w
    buf[n:n + p.cout] = p.scale
    buf[n + cout_pad:n + cout_pad + p.cout] = p.shift
    return dataclasses.replace(p, w=w, scale=buf[n:n + p.cout], shift=buf[n + cout_pad:n + cout_pad + p.cout],
                               cin_pad=cin_pad)


@pytest.mark.parametrize("what", ["bn elsewhere", "cin_pad 32 != CINMAX 16"])
def test_pair2_undescribed_pairs_run_the_struct_kernel(what):
    """Through the default entry (no hint): the record refuses the pair, the struct-argument kernel runs it, and the
    result is the described pair's, bitwise."""
    pa, pb, xs, ref = case(3, 1, 3, (16,), 16, 7, 15)
    xd = [x.to(DEV) for x in xs]
    y, rec = run(pa, xd, pb, 2, True, torch.zeros(ref.shape, device=DEV))
    assert rec
    pa2 = _moved_bn(pa) if what == "bn elsewhere" else _wider_cin_pad(pa, 32)
    y2, rec2 = run(pa2, xd, pb, 2, True, torch.zeros(ref.shape, device=DEV))
    assert not rec2
    assert torch.equal(y, y2) and rel(y2, ref) < 1e-5
    if what == "bn elsewhere":  # convB's too
        y3, rec3 = run(pa, xd, _moved_bn(pb), 2, True, torch.zeros(ref.shape, device=DEV))
        assert not rec3 and torch.equal(y, y3)


def test_pair2_record_plan_replay_after_rebind():
    """A plan's pair behind the record, replayed as a graph before and after its source moves to another allocation
    (esm_plan_rebind re-captures the launch, so the patched pointer reaches the record's dwords)."""
    pa, pb, xs, _ = case(3, 1, 1, (16,), 16, 7, 15)
    x0 = xs[0].to(DEV)
    x1 = (xs[0] * -0.5 + 0.25).to(DEV)
    plan = Ctx(DEV, plan=True)
    seen = []
    add = plan.pair2
    plan.pair2 = lambda a, b: (seen.append(behind_record(a, b)), add(a, b))[1]
    y = run_pair2(plan, pa, [x0], pb, force=True, ksplit=False)
    assert seen == [True]
    eager = Ctx(DEV)
    plan.launch(graph=True)
    torch.cuda.synchronize()
    want0 = run_pair2(eager, pa, [x0], pb, force=True, ksplit=False)
    assert torch.equal(y, want0)
    n = 1
    rc = lib.esm_plan_rebind(plan.plan, n, (_lib.c_void_p * n)(x0.data_ptr()), (ctypes.c_uint64 * n)(4 * x0.numel()),
                             (_lib.c_void_p * n)(x1.data_ptr()))
    assert rc >= 1, lib.esm_last_error()  # the number of pointers moved: convA's source (and convB's unread one)
    x0.fill_(float("nan"))  # the old allocation is no longer read
    plan.launch(graph=True)
    torch.cuda.synchronize()
    want1 = run_pair2(eager, pa, [x1], pb, force=True, ksplit=False)
    assert torch.equal(y, want1) and not torch.equal(want0, want1)
    plan.close()
