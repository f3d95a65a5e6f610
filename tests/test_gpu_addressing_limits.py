"""GPU tests at the 32-bit addressing limits of the strided kernels (DESIGN.md "Addressing limits").

Most conv forms address their operands with 32-bit byte offsets through buffer descriptors, lanes outside the tensor
marked ``kOOB = 2^30`` (csrc/conv_direct.h): sound while an operand's span per batch item stays below 1 GiB.  Every
launcher guards that on the host and hands a layer beyond it to a 64-bit form, or refuses it.  Here every case of
tests/test_gpu_layouts.py runs at its own small extents and B = 2 with ONE operand at a time -- source 0, the last
source, ``out`` (with ``out2``), ``res``, ``mul`` -- placed far (tests/layouts.py ``embed_far``), the others contiguous:

  near    the channel stride (a one-channel operand: the plane stride in 3-D, the row stride in 2-D) that puts
          ``4 * last`` in [kOOB - 4096, kOOB): the last layout every form must still run;
  over    the stride that puts it in [kOOB, kOOB + 4096), and 4 GiB of sentinel cells behind every item's base: a
          wrapped offset or a mark taken for an address reads NaN or writes a guard cell of the test's own allocation;
  stride  that axis 2^28 + 4 elements apart, the same tail (only where the axis has at most 5 entries: more would
          not fit the 12 GiB a test may hold);
  batch   a batch stride of 2^30 + 64 elements: item 1 starts past 4 GiB.

Per run: the launch raises ``EsmError`` or its output is finite and within the op's tolerance of the fp64 reference
(1e-5, as tests/test_gpu_layouts.py); ``near`` and ``batch`` never raise, nor does hint 0 anywhere; every cell outside a
far ``out`` / ``out2`` is untouched; where the same form runs the contiguous copy the results are bitwise equal; and a
forced form ends as the table in DESIGN.md says: its launcher's refusal, or the form it steps aside for.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import feature_pair
from layouts import FarArena, assert_guards_intact, embed_far, far_tail_elems, guard_snapshot
from test_addressing_limits_host import BITS32, KOOB, far_stride
from test_gpu_layouts import (B, CONV_CASES, DEV, DWCONV_CASES, GENERAL, PAIR_CASES, PW, SHUFFLE_CONV_CASES,
                              SHUFFLE_TAIL_CASES, TILE2, TILE3, UP1_LAYOUT_CASES, _finite_close, _form, _head, conv_case)
from test_gpu_parity import _mk, _ref_conv, pk

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

import esmstereo_amd as E  # noqa: E402
from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd._lib import HINT_ROWS as ROWS  # noqa: E402
from esmstereo_amd._lib import (HINT_C1IN, HINT_C1T, HINT_DIRECT, HINT_GWC_STEM_WLDS, HINT_ROWS_FORM, HINT_SMALL,  # noqa: E402
                                HINT_STEM, HINT_TILE, HINT_WIDE, HINT_WIDE3, HINT_WIDET)
from esmstereo_amd.engine import ACT_GELU, ACT_SILU, Ctx, run_conv  # noqa: E402
from oracle import esm_oracle as O  # noqa: E402

PLACES = ("near", "over", "stride", "batch")
TAIL = 4 << 30             # bytes behind every item's base at "over" / "stride": every 32-bit byte offset
STRIDE_MAX_ENTRIES = 5     # "stride": (n - 1) GiB per item, twice for B = 2 (8 GiB at 5 entries)
BATCH_STRIDE = (1 << 30) + 64
ARENA_STEP = 1 << 27      # elements (0.5 GiB): a test's far operands, all of nearly one size, share one allocation
# (two cases are about the embedding itself: with every other operand contiguous they are wide-k3-2src and pointwise-2d)
FAR_CASES = [c for c in CONV_CASES if c.loose is None and c.name != "pointwise-strided-planes"]


def far_axis(t):
    """The axis the placements move: the outermost one below the batch with at least two entries (an axis outside
    the moved one would multiply the allocation by its extent), its entries and the packed elements of one."""
    for i, name in zip(range(1, t.dim() - 1), "cdh" if t.dim() == 5 else "ch"):
        if t.shape[i] >= 2:
            return name, int(t.shape[i]), math.prod(int(v) for v in t.shape[i + 1:])
    return None


def place(t, how, arena=None, tail=TAIL):
    """``t`` on the device: contiguous (``how`` None) or far, in ``arena``'s allocation (the one far view of a test at a
    time: layouts.FarArena); None where the placement does not exist for ``t``."""
    if how is None:
        return t.to(DEV)
    if how == "batch":
        return embed_far(t, "b", BATCH_STRIDE, DEV, arena=arena)
    ax = far_axis(t)
    if ax is None or (how == "stride" and ax[1] > STRIDE_MAX_ENTRIES):
        return None
    name, n, inner = ax
    v = embed_far(t, name, far_stride(how, n, inner), DEV, tail_bytes=0 if how == "near" else tail, arena=arena)
    last = sum((k - 1) * s for k, s in zip(v.shape[1:], v.stride()[1:])) + 1
    if how == "near":
        assert KOOB - 4096 <= 4 * last < KOOB
    elif how == "over":
        assert KOOB <= 4 * last < KOOB + 4096
    if how != "near":
        assert 4 * far_tail_elems(v) >= tail
    return v


def entries(channels, spatial):
    """Entries of the axis ``far_axis`` picks for an operand [B, channels, *spatial]."""
    return next((int(n) for n in (channels,) + tuple(spatial[:-1]) if n >= 2), 0)


def stride_exists(*operands):
    """Whether "stride" can place at least one of the (channels, spatial extent) operands: 2 to STRIDE_MAX_ENTRIES
    entries on its axis.  The other combinations are not parametrised: they would launch nothing."""
    return any(2 <= entries(c, sp) <= STRIDE_MAX_ENTRIES for c, sp in operands)


def conv_operands(c):
    """(channels, spatial extent) of every operand of a conv Case the placements move."""
    out_sp = tuple(2 * v if c.tr else (v + 2 * c.p - c.k) // c.s + 1 for v in c.shape)
    r = c.shuffle
    oc, osp = c.cout // (r * r), out_sp[:-2] + (out_sp[-2] * r, out_sp[-1] * r)
    ops = [(ci, c.shape) for ci in (c.cins[0], c.cins[-1])] + [(oc, osp)]
    if "res" in c.epi:
        ops.append((oc, osp))
    if "mul" in c.epi:
        ops.append((c.cout, out_sp[-2:]))
    return ops


def places(*operands):
    return [how for how in PLACES if how != "stride" or stride_exists(*operands)]


def release(*arenas):
    """Free the far allocations (the callers drop their own views first)."""
    for a in arenas:
        a.release()
    torch.cuda.empty_cache()


def test_far_placements_on_the_device():
    """``embed_far`` and the snapshot that keeps no copy, on GPU memory at the sizes used below: the values, the
    sentinel behind the item's base up to 4 GiB, and one stray cell 2^30 bytes from the base caught."""
    t = torch.randn(B, 3, 7, 19)
    v = place(t, "over")
    assert torch.equal(v.cpu(), t) and v.stride(1) >= (KOOB // 4 - 7 * 19) // 2
    snap = guard_snapshot(v)
    assert snap.sparse and snap.bits is None
    flat = torch.empty(0, device=DEV).set_(v.untyped_storage())
    base1 = v.storage_offset() + v.stride(0)
    assert bool(torch.isnan(flat[base1 + TAIL // 4 - 1])) and bool(torch.isnan(flat[v.storage_offset() + 7 * 19]))
    v.fill_(1.0)
    assert_guards_intact(v, snap)
    stray = KOOB // 4 + 4096  # elements from item 1's base: what a store at (mark + a row), taken for an address, writes
    flat[base1 + stray] = 1.0
    with pytest.raises(AssertionError, match=rf"1 guard cell.*\[{v.stride(0) + stray}\]"):
        assert_guards_intact(v, snap)
    del flat, snap, v
    release()
    assert torch.cuda.memory_allocated() < 1 << 30


# ----------------------------------------------------------------------------- convs


def test_conv_operand_shapes_as_parametrised():
    """``conv_operands`` (which decides at collection whether a case has a "stride" test) names the shapes the
    case's tensors really have."""
    for c in FAR_CASES:
        pc, xs, ops, kw, ref, oshape = conv_case(c)
        real = [(x.shape[1], tuple(x.shape[2:])) for x in (xs[0], xs[-1])] + [(oshape[1], tuple(oshape[2:]))]
        real += [(ops[k].shape[1], tuple(ops[k].shape[2:])) for k in ("res", "mul") if k in ops]
        assert [(int(a), tuple(int(v) for v in b)) for a, b in real] == \
            [(int(a), tuple(int(v) for v in b)) for a, b in conv_operands(c)], c.name


def forced_source_outcome(c, hint):
    """What a forced form does with a source past the limit (DESIGN.md "Addressing limits"): "raise" (its launcher's
    check refuses), "auto" (it steps aside for the automatic rules) or "run" (64-bit addressing)."""
    if hint & HINT_WIDE:
        return "auto"
    if c.form == GENERAL:
        return "raise" if hint & (HINT_DIRECT | HINT_ROWS_FORM | HINT_C1T) else "run"
    if hint & HINT_C1IN:
        return "run"
    assert hint & (HINT_STEM | HINT_SMALL | HINT_WIDE3 | HINT_WIDET | HINT_TILE), hex(hint)
    return "raise"  # (the pointwise form steps aside for the LDS-tiled one, which refuses)


CONV_FAR = [pytest.param(c, how, id=f"{c.name}-{how}") for c in FAR_CASES for how in places(*conv_operands(c))]


@pytest.mark.parametrize("case,how", CONV_FAR)
def test_conv_far(case, how):
    c = case
    pc, xs, ops, kw, ref, oshape = conv_case(c)
    two = "out2" in c.epi
    hints = [c.hints[0], 0]
    tile = TILE3 if c.nd == 3 else TILE2
    arenas = [FarArena(DEV, ARENA_STEP), FarArena(DEV, ARENA_STEP)]  # the far operand's allocation; out2's, when out is the far one

    def operands(which, where):
        """Every operand contiguous but ``which``; None where the placement does not exist for it."""
        srcs = [place(x, where if which == ("src0" if i == 0 else "srcN" if i == len(xs) - 1 else None) else None, arenas[0])
                for i, x in enumerate(xs)]
        o = {k: place(v, where if which == k else None, arenas[0]) for k, v in ops.items() if k != "up"}
        if "up" in ops:
            o["up"] = ops["up"].to(DEV)
        outs = [place(torch.zeros(oshape), where if which == "out" else None, arenas[i]) for i in range(2 if two else 1)]
        if any(t is None for t in srcs + list(o.values()) + outs):
            return None
        return srcs, o, outs

    def keywords(o, outs, hint):
        ckw = dict(o, shuffle=c.shuffle, post_scale=c.post, hint=hint, **kw)
        if two:
            ckw.update(out2=outs[1], post_scale2=0.5)
        return ckw

    cont = {}  # hint -> (form, y, out2) on contiguous operands
    for hint in hints:
        srcs, o, outs = operands(None, None)
        ckw = keywords(o, outs, hint)
        form = _form(pc, srcs, outs[0], **ckw)
        if hint:
            assert form == c.form, f"{c.name} hint {hint:#x}"
        y = run_conv(Ctx(DEV), pc, srcs, outs[0], **ckw)
        cont[hint] = (form, y, outs[1] if two else None)
    torch.cuda.synchronize()

    names = ["src0"] + (["srcN"] if len(xs) > 1 else []) + ["out"] + [k for k in ("res", "mul") if k in ops]
    ran = 0
    for which in names:
        for hint in hints:
            what = f"{c.name} {how} {which} far, hint {hint:#x}"
            got = operands(which, how)
            if got is None:
                continue  # ("stride" on an axis of more than STRIDE_MAX_ENTRIES entries)
            ran += 1
            srcs, o, outs = got
            ckw = keywords(o, outs, hint)
            form = _form(pc, srcs, outs[0], **ckw)
            past = how in ("over", "stride")
            want, refuse = cont[hint][0], False
            if past and hint == 0:
                assert form not in BITS32[which], what           # the automatic rules leave the 32-bit forms
            elif past and which.startswith("src"):
                outcome = forced_source_outcome(c, hint)
                refuse = outcome == "raise"
                if outcome == "auto":
                    want = _form(pc, srcs, outs[0], **dict(ckw, hint=0))
                elif c.form == PW:
                    want = tile
                assert form == want, what
            elif past and which == "out" and c.form == PW:
                assert form == tile, what                        # steps aside; the LDS-tiled form stores 64-bit
            else:
                assert form == want, what                        # near, batch; res / mul / out past the limit
            snaps = [guard_snapshot(t) for t in outs] if which == "out" else []
            try:
                if refuse:
                    with pytest.raises(E.EsmError):
                        run_conv(Ctx(DEV), pc, srcs, outs[0], **ckw)
                else:
                    y = run_conv(Ctx(DEV), pc, srcs, outs[0], **ckw)  # (near, batch, hint 0: never refused)
                    torch.cuda.synchronize()
                    _finite_close(y, ref * c.post, 1e-5, what)
                    if two:
                        _finite_close(outs[1], ref * 0.5, 1e-5, what + " out2")
                    # (GENERAL names the direct, row-streaming, VALU ConvTranspose and LDS-staged kernels alike: with
                    # hint 0 a source past the limit moves the layer among them, each with its own sum order)
                    moved = past and hint == 0 and which.startswith("src") and form == GENERAL
                    if form == cont[hint][0] and not moved:
                        assert torch.equal(y.contiguous(), cont[hint][1]), what + ": differs bitwise from the contiguous layout"
                        if two:
                            assert torch.equal(outs[1].contiguous(), cont[hint][2]), what + " out2"
                    y = None
                for t, snap in zip(outs, snaps):
                    assert_guards_intact(t, snap, what)
            except BaseException:
                release(*arenas)
                raise
            finally:
                srcs = o = outs = ckw = got = snaps = None
    release(*arenas)
    assert ran, c.name


# ----------------------------------------------------------------------------- fused launches and the other strided ops


def _far_launch(run, tensors, out_shape, how, ref, what, tol=1e-5, contiguous=None, tail=TAIL):
    """``run(tensors, out)`` with each of ``tensors`` (CPU), then the output, far in turn.  "near" / "batch": runs,
    and bitwise as ``contiguous``; past the limit: an EsmError, or a result within ``tol`` (another form may serve
    the launch, with its own sum order).  Every guard cell of a far output is untouched either way."""
    ran = 0
    arena = FarArena(DEV, ARENA_STEP)
    for k in list(range(len(tensors))) + ["out"]:
        ts = [place(t, how if i == k else None, arena, tail) for i, t in enumerate(tensors)]
        out = place(torch.zeros(out_shape), how, arena, tail) if k == "out" else torch.zeros(out_shape, device=DEV)
        if out is None or any(t is None for t in ts):
            ts = out = None
            continue
        ran += 1
        snap = guard_snapshot(out) if k == "out" else None
        try:
            try:
                y = run(ts, out)
            except E.EsmError:
                assert how in ("over", "stride"), f"{what} {how} operand {k}: refused below the limit"
                y = None
            torch.cuda.synchronize()
            if y is not None:
                _finite_close(y, ref, tol, f"{what} {how} operand {k}")
                if how in ("near", "batch") and contiguous is not None:
                    assert torch.equal(y.contiguous(), contiguous), f"{what} {how} operand {k}"
            if snap is not None:
                assert_guards_intact(out, snap, f"{what} {how} operand {k}")
        except BaseException:
            release(arena)
            raise
        finally:
            y = ts = out = snap = None
    release(arena)
    assert ran, f"{what} {how}: nothing placed"
    return ran


def _pair_operands(c):
    name, nd, cins, ka, sa, pa, kb, coutb, shape, ksplit = c
    return [(cins[0], shape), (cins[-1], shape), (coutb, tuple((v + 2 * pa - ka) // sa + 1 for v in shape))]


PAIR_FAR = [pytest.param(*c, how, id=f"{c[0]}-{how}") for c in PAIR_CASES for how in places(*_pair_operands(c))]


@pytest.mark.parametrize("name,nd,cins,ka,sa,pa,kb,coutb,shape,ksplit,how", PAIR_FAR)
def test_conv_pair_far(name, nd, cins, ka, sa, pa, kb, coutb, shape, ksplit, how):
    from esmstereo_amd.engine import run_pair2
    ca, ba = _mk(nd, sum(cins), 16, ka, sa, pa, seed=31 + len(name))
    cb, bb = _mk(nd, 16, coutb, kb, 1, kb // 2, seed=32 + len(name))
    xs = [torch.randn(B, c, *shape) for c in cins]
    ref = _ref_conv([_ref_conv(xs, ca, ba, ACT_GELU)], cb, bb, ACT_GELU)
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    yc = run_pair2(Ctx(DEV), pa_, [x.to(DEV) for x in xs], pb_, force=True, ksplit=ksplit)
    far = [xs[0]] + ([xs[-1]] if len(xs) > 1 else [])  # source 0 and the last one

    def run(ts, out):
        srcs = [ts[0]] + [x.to(DEV) for x in xs[1:-1]] + ([ts[-1]] if len(xs) > 1 else [])
        return run_pair2(Ctx(DEV), pa_, srcs, pb_, force=True, ksplit=ksplit, out=out)

    _far_launch(run, far, ref.shape, how, ref, f"pair {name}", contiguous=yc)


UP1_FAR = [pytest.param(*c, how, id=f"{c[0]}-{how}") for c in UP1_LAYOUT_CASES
           for how in places((c[2], c[6]), (c[4][-1], c[7]), (c[5], c[7]))]  # the ConvT's source, the last extra source, out


@pytest.mark.parametrize("name,nd,cin,cy,cxs,coutb,grid,crop,hint,how", UP1_FAR)
def test_convt_1x1_far(name, nd, cin, cy, cxs, coutb, grid, crop, hint, how):
    from esmstereo_amd.engine import run_convt_1x1
    ca, ba = _mk(nd, cin, cy, 4, 2, 1, transposed=True, seed=51 + cin)
    cb, bb = _mk(nd, cy + sum(cxs), coutb, 1, 1, 0, seed=52 + coutb)
    x = torch.randn(B, cin, *grid)
    xs = [torch.randn(B, c, *crop) for c in cxs]
    u = _ref_conv([x], ca, ba, ACT_GELU)
    u = u[(slice(None), slice(None)) + tuple(slice(0, n) for n in crop)]
    ref = _ref_conv([u, *xs], cb, bb, ACT_GELU)
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    old = dict(EN.HINT_SET)
    EN.HINT_SET["convT"] = hint
    try:
        yc = run_convt_1x1(Ctx(DEV), pa_, [x.to(DEV)], pb_, [t.to(DEV) for t in xs])

        def run(ts, out):  # the transposed conv's source and the last extra source far in turn
            extra = [t.to(DEV) for t in xs[:-1]] + [ts[1]]
            return run_convt_1x1(Ctx(DEV), pa_, [ts[0]], pb_, extra, out=out)

        _far_launch(run, [x, xs[-1]], ref.shape, how, ref, f"convt_1x1 {name}", contiguous=yc)
    finally:
        EN.HINT_SET.clear()
        EN.HINT_SET.update(old)


@pytest.mark.parametrize("how", places((8, (5, 7, 20))))
def test_gwc_stem_far(how):
    """L and R are bare contiguous pointers: the output far, with every hint of test_gwc_stem_layouts."""
    from esmstereo_amd.engine import run_gwc_stem
    G, D, H, W = 8, 5, 7, 20
    conv, bn = _mk(3, G, 8, 3, 1, 1, seed=G + D)
    L, R = feature_pair(B, 2 * G, H, W, 7, D)
    ref = _ref_conv([O.gwc_volume(L, R, D, G)], conv, bn, ACT_GELU)
    p = pk(conv, bn, ACT_GELU)
    Ld, Rd = L.to(DEV), R.to(DEV)
    for hint in (0, ROWS(2), ROWS(3), HINT_GWC_STEM_WLDS, ROWS(2) | HINT_GWC_STEM_WLDS):
        yc = run_gwc_stem(Ctx(DEV), p, Ld, Rd, G, D, hint=hint)
        _far_launch(lambda ts, out: run_gwc_stem(Ctx(DEV), p, Ld, Rd, G, D, hint=hint, out=out), [], ref.shape, how, ref,
                    f"gwc_stem hint {hint:#x}", contiguous=yc)


TAIL_FAR = [pytest.param(*c, how, id=f"{c[0]}-{c[1]}-{c[2]}x{c[3]}-{how}") for c in SHUFFLE_TAIL_CASES
            for how in places((c[0], c[2:4]), (1, (c[2] * c[1], c[3] * c[1])))]


@pytest.mark.parametrize("nf,r,H,W,forms,how", TAIL_FAR)
def test_shuffle_tail_far(nf, r, H, W, forms, how):
    """Every form of the case (the window form and both row forms), x and the one-channel output far in turn."""
    p, head = _head(nf, r, nf * 100 + r)
    x = torch.randn(B, nf, H, W)
    ref = head(x).float()
    for form in forms:
        yc = EN.run_shuffle_tail(Ctx(DEV), x.to(DEV), p, form=form)
        _far_launch(lambda ts, out: EN.run_shuffle_tail(Ctx(DEV), ts[0], p, out=out, form=form), [x], ref.shape, how,
                    ref, f"shuffle_tail form {form}", contiguous=yc)


SC_FAR = [pytest.param(*c, how, id=f"{c[0]}-{c[1]}-{c[2]}-{how}") for c in SHUFFLE_CONV_CASES
          for how in places((c[0], c[3:5]), (c[2], ((c[3] * c[1] + 1) // 2, (c[4] * c[1] + 1) // 2)))]


@pytest.mark.parametrize("nf,r,C,H,W,forms,how", SC_FAR)
def test_shuffle_conv_far(nf, r, C, H, W, forms, how):
    p, head = _head(nf, r, nf * 1000 + r * 10 + H)
    conv, bn = _mk(2, 1, C, 3, 2, 1, seed=H)
    pc = pk(conv, bn, ACT_GELU)
    x = torch.randn(B, nf, H, W)
    ref = _ref_conv([head(x)], conv, bn, ACT_GELU)
    for form in forms:
        yc = EN.run_shuffle_conv(Ctx(DEV), x.to(DEV), p, pc, form=form)
        _far_launch(lambda ts, out: EN.run_shuffle_conv(Ctx(DEV), ts[0], p, pc, form=form, out=out), [x], ref.shape, how,
                    ref, f"shuffle_conv form {form}", contiguous=yc)


@pytest.mark.parametrize("how", places((5, (9, 21))))
@pytest.mark.parametrize("k,s", DWCONV_CASES)
def test_dwconv_far(k, s, how):
    torch.manual_seed(k * 10 + s)
    C, H, W = 5, 9, 21
    x = torch.randn(B, C, H, W)
    w = torch.randn(C, 1, k, k) * 0.3
    sc, sh = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    p = (k - 1) // 2 if s == 1 else ((s - 1) + (k - 1)) // 2
    ref = F.silu(F.conv2d(x.double(), w.double(), None, s, p, 1, C) * sc.double().view(1, C, 1, 1) +
                 sh.double().view(1, C, 1, 1)).float()
    args = (w.reshape(C, k * k).contiguous().to(DEV), sc.to(DEV), sh.to(DEV), k, s, p, ACT_SILU)
    yc = EN.run_dwconv(Ctx(DEV), x.to(DEV), *args)
    ran = _far_launch(lambda ts, out: EN.run_dwconv(Ctx(DEV), ts[0], *args, out=out), [x], ref.shape, how, ref,
                      f"dwconv k{k} s{s}", contiguous=yc, tail=0)  # (64-bit pointers only: no 32-bit offset to catch)
    assert ran == 2  # 5 channels: every placement exists, and the 64-bit kernel runs them all
