"""Every row of the tuned-hint table (esmstereo_amd/tuned_hints.json) run at its OWN shape and batch.

The table is data that selects code: a launch whose shape key (``engine.conv_key``) is a row gets the row's hint,
which picks the kernel form, its tile, its K split and its weight home, and a forced form is only checked by its
launcher.  A smaller tensor has another key and never meets the hint, so each case builds a seeded layer and
device inputs of exactly the row's batch and extent and runs it the way the hot path does (``hint=0``: the lookup).

Per case:
  1. the launch reports the row's key and the table's hint (bit 30, the tile order, is the engine's own);
  2. ``esm_conv_form`` names a form for the descriptor and the launch does not raise;
  3. a few output windows (tests/tuned_rows.py: corners, one interior, items 0 / B // 2 / B - 1) are finite and
     within 1e-5 (max |diff| / max |ref| over the window, ``rel()`` applied to the window) of the fp64 torch
     reference computed from the input crop alone, through the same BN / activation / epilogue;
  4. the whole tensor agrees, per batch item and on the device, with the same layer run through the general
     LDS-staged form (hint 0x11) to 2e-5: each side is within 1e-5 of fp64, so the bound is their sum.

``test_conv_forms_large_batch`` runs one small layer per kernel form at B = 33 and B = 257, and
``test_hot_path_L_K_batch32`` the whole ESMStereo-L hot path at the global batch of BASELINE configs[3] on one GPU.
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

from helpers import fullsize_inputs
from parity import flip_masked
from tuned_rows import load_table, parse_key, window_expect, windows

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd.engine import ACT_GELU, ACT_NONE, ACT_RELU6, ACT_SILU, Ctx, run_conv  # noqa: E402
from test_gpu_layouts import CONV_CASES  # noqa: E402
from hot_checks import flips_and_margin as _flips_and_margin, hip_cost as _hip_cost  # noqa: E402
from test_gpu_parity import _mk, _model_from_manifest, _ref_conv, cu, pk, rel  # noqa: E402

DEV = torch.device("cuda")
TABLE = load_table()
HINT_GENERAL = 0x11  # the LDS-staged implicit GEMM, one N tile, no K split (conv_impl.h)
FORM_NAMES = ("general", "stem", "c1in", "small", "wide", "wide3", "widet", "tile3", "tile2", "pointwise")
ACTS = {ACT_GELU: ("gelu", F.gelu), ACT_SILU: ("silu", F.silu), ACT_RELU6: ("relu6", F.relu6),
        ACT_NONE: ("linear", lambda t: t)}


def _row_cases():
    for key in sorted(TABLE):
        spec = parse_key(key)
        yield pytest.param(key, ACT_GELU, id=key)  # BN + GELU: how BasicConv meets the row
        if spec.B == 2 and spec.nd == 2:  # the backbone's rows: its SiLU, ReLU6 and linear epilogues too
            for act in (ACT_SILU, ACT_RELU6, ACT_NONE):
                yield pytest.param(key, act, id=f"{key} {ACTS[act][0]}")


def _form(pc, srcs, out, **kw):
    d, _, _ = EN._conv_desc(Ctx(DEV), pc, srcs, out, **kw)
    return _lib.lib.esm_conv_form(ctypes.byref(d))


def _per_item_rel(a, b):
    """max |a - b| / max |b| per batch item, on the device; ``a`` is overwritten."""
    dims = tuple(range(1, a.dim()))
    return a.sub_(b).abs_().amax(dims) / b.abs().amax(dims).clamp_min(1e-30)


@pytest.mark.parametrize("key,act", _row_cases())
def test_tuned_row(key, act):
    spec = parse_key(key)
    assert spec.shuffle == 1, "a PixelShuffle row: extend the windowed reference before tuning one"
    seed = zlib.crc32(key.encode()) & 0x7fffffff
    conv, bn = _mk(spec.nd, spec.cin, spec.cout, spec.k, spec.s, spec.p, transposed=spec.transposed, seed=seed & 0xffff)
    pc = pk(conv, bn, act)
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    B, ext = spec.B, spec.out_ext
    srcs = [rn(B, c, *spec.in_ext) for c in spec.cins]
    ops, kw = {}, {}
    if spec.u:  # the refinement heads' `+ bilinear(previous disparity, 2)` (ESMStereo.py:307, 316)
        ops["up"] = rn(B, 1, ext[-2] // 2, ext[-1] // 2)
        kw["up_f"] = 2
    if spec.m:  # broadcast over D
        ops["mul"] = torch.rand(B, spec.cout, ext[-2], ext[-1], device=DEV, generator=g) + 0.5
    if spec.r:
        ops["res"] = rn(B, spec.cout, *ext)
    outs = {h: torch.empty(B, spec.cout, *ext, device=DEV) for h in (0, HINT_GENERAL)}
    out2 = {h: torch.empty_like(outs[h]) for h in outs} if spec.two else {}

    def call(h):
        return dict(ops, **kw, hint=h, **(dict(out2=out2[h], post_scale2=0.5) if spec.two else {}))

    # 1, 2: the lookup gives this launch the row's hint, a form takes it, the launch does not raise
    ctx = Ctx(DEV)
    y = run_conv(ctx, pc, srcs, outs[0], **call(0))
    meta = ctx.meta[-1]
    assert meta["key"] == key
    assert meta["hint"] & ~EN.HINT_XCD_SLAB == TABLE[key], (hex(meta["hint"]), hex(TABLE[key]))
    form = _form(pc, srcs, outs[0], **call(0))
    assert 0 <= form < len(FORM_NAMES), _lib.lib.esm_last_error()
    print(f"row B{B} [{key}] {ACTS[act][0]}: hint {TABLE[key]:#x} -> form {FORM_NAMES[form]}")

    # 3: fp64 windows, from the input crop alone
    sc = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).detach()
    sh = (bn.bias.double() - bn.running_mean.double() * sc).detach()
    ups = {}
    worst = 0.0
    for b, lo, hi in windows(spec):
        win = (slice(None),) + tuple(slice(a, e) for a, e in zip(lo, hi))
        if spec.u and b not in ups:  # the item's one-channel map, interpolated whole in fp64 (it is small)
            ups[b] = F.interpolate(ops["up"][b:b + 1].double().cpu(), scale_factor=2, mode="bilinear",
                                   align_corners=False)[0]
        ref = window_expect([s[b] for s in srcs], conv.weight, spec, lo, hi, sc, sh, ACTS[act][1],
                            mul_b=ops["mul"][b] if spec.m else None, res_b=ops["res"][b] if spec.r else None,
                            up_b=ups.get(b))
        got = y[b][win].double().cpu()
        assert bool(torch.isfinite(got).all()), (key, b, lo)
        e = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        worst = max(worst, e)
        assert e <= 1e-5, (key, "item", b, "window", lo, hi, e)
        if spec.two:
            g2 = out2[0][b][win].double().cpu()
            assert float((g2 - 0.5 * ref).abs().max() / (0.5 * ref).abs().max().clamp_min(1e-30)) <= 1e-5, (key, b, lo)

    # 4: the whole tensor against the general LDS-staged form, per batch item, on the device
    if TABLE[key] == HINT_GENERAL:
        return
    assert _form(pc, srcs, outs[HINT_GENERAL], **call(HINT_GENERAL)) == _lib.FORM_GENERAL
    yg = run_conv(Ctx(DEV), pc, srcs, outs[HINT_GENERAL], **call(HINT_GENERAL))
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(yg).all()), key
    pairs = [(y, yg)] + ([(out2[0], out2[HINT_GENERAL])] if spec.two else [])
    for a, ref in pairs:
        r = _per_item_rel(a, ref)
        wb = int(r.argmax())
        print(f"    windows {worst:.2e}; whole tensor vs general form: worst item {wb} at {float(r[wb]):.2e}")
        assert float(r[wb]) <= 2e-5, (key, "worst batch item", wb, float(r[wb]), r.tolist())


# ----------------------------------------------------------------------------- every form at a large batch

LARGE_BATCH_ROWS = ("general-2d-k3s1", "rows-2d", "stem-3d", "c1in-k3s2", "small-3d-convT", "wide-k3", "wide3-32to8",
                    "widet-8to16", "tile3-convT", "tile2-k3", "pointwise-2d")
_BY_NAME = {c.name: c for c in CONV_CASES}


@pytest.mark.parametrize("B", [33, 257])
@pytest.mark.parametrize("name", LARGE_BATCH_ROWS)
def test_conv_forms_large_batch(name, B):
    """One small layer per kernel form with its forced hints at B = 33 and B = 257 (no op-level test had a batch
    above 3).  Batch shares grid y / z with planes, parity classes and cout tiles, split in some forms by
    host-computed reciprocals: 257 items of the ConvTranspose3d rows put 4112 and 6168 workgroup planes on z.
    Full fp64 torch reference, 1e-5 relative.  A form whose launcher refuses the grid must say so ("too large")."""
    c = _BY_NAME[name]
    conv, bn = _mk(c.nd, sum(c.cins), c.cout, c.k, c.s, c.p, transposed=c.tr, bn=c.bn, seed=sum(c.cins) + c.cout)
    gen = torch.Generator().manual_seed(B + len(name))
    xs = [torch.randn(B, ci, *c.shape, generator=gen) for ci in c.cins]
    ref = _ref_conv(xs, conv, bn, c.act)
    pc = pk(conv, bn, c.act)
    srcs = [x.to(DEV) for x in xs]
    for hint in c.hints:
        what = f"{name} B{B} hint {hint:#x}"
        out = torch.zeros(tuple(ref.shape), device=DEV)
        assert _form(pc, srcs, out, hint=hint) == c.form, what
        try:
            y = run_conv(Ctx(DEV), pc, srcs, out, hint=hint)
        except _lib.EsmError as e:
            assert "too large" in str(e), what
            print(f"{what}: refused ({e})")
            continue
        assert bool(torch.isfinite(y).all()), what
        assert rel(y, ref) < 1e-5, what


# ----------------------------------------------------------------------------- batch 32 through the whole hot path


def test_hot_path_L_K_batch32():
    """ESMStereo-L, gwc, 384x1248, maxdisp 192 at B = 32 (BASELINE configs[3]'s global batch on one GPU) against
    the same 32 items run as eight B = 4 plans (the plan ``test_hot_path_full_size_vs_oracle`` pins to the oracle):
    every item's aggregated cost to 2e-5 relative (two fp32 paths, each within 1e-5 of fp64), every output through
    the flip-masked metric of tests/parity.py with its own caps, and every tuned B32 row looked up by the plan."""
    model, sd, m = _model_from_manifest("hot_L_gwc.npz", maxdisp=192)
    chunks = []
    for i in range(8):
        ml, mr, _, up = fullsize_inputs(4, 4, 384, 1248, 192, 102 + i, att=False)
        chunks.append((cu(ml), cu(mr), [cu(u) for u in up]))
    ml32 = torch.cat([c[0] for c in chunks], 0)
    mr32 = torch.cat([c[1] for c in chunks], 0)
    up32 = [torch.cat([c[2][j] for c in chunks], 0) for j in range(len(chunks[0][2]))]
    out32 = [o.clone() for o in model.hot_path(ml32, mr32, None, up32, True)]
    plan = next(hp for k, hp in model._plans.items() if k[0][0] == 32)
    looked_up = 0
    for op in plan.ctx.meta:
        if op["kind"] == "conv" and op.get("key") in TABLE:
            assert op["hint"] & ~EN.HINT_XCD_SLAB == TABLE[op["key"]], (op["name"], op["key"])
            assert parse_key(op["key"]).B == 32
            looked_up += 1
    b32_rows = {k for k in TABLE if parse_key(k).B == 32}
    seen = {op["key"] for op in plan.ctx.meta if op["kind"] == "conv" and op.get("key") in TABLE}
    print(f"L-K B32 plan: {len(plan.ctx.meta)} launches, {looked_up} plain convs with a tuned row, "
          f"{len(seen)} of the {len(b32_rows)} B32 rows as plain convs")
    # (the other B32 rows are met inside fused launches: gwc volume + stem, ConvTranspose + 1x1)
    assert looked_up and seen <= b32_rows and len(seen) >= len(b32_rows) - 2
    cost32 = _hip_cost(model, ml32, mr32, None, 48)
    out4, cost4 = [], []
    for ml, mr, up in chunks:
        out4.append([o.clone() for o in model.hot_path(ml, mr, None, up, True)])
        cost4.append(_hip_cost(model, ml, mr, None, 48))
    cost4 = torch.cat(cost4, 0)
    assert cost32.shape == cost4.shape and bool(torch.isfinite(cost32).all())
    assert float(cost4.abs().amax((1, 2, 3, 4)).min()) > 0  # (no item of the reference is a blank volume)
    r = _per_item_rel(cost32.clone(), cost4)
    wb = int(r.argmax())
    print(f"aggregated cost B32 vs 8 x B4: worst item {wb} at {float(r[wb]):.2e}")
    assert float(r[wb]) <= 2e-5, ("worst batch item", wb, r.tolist())
    flips, margin = _flips_and_margin(cost32[:, 0], cost4[:, 0])
    assert len(out32) == len(out4[0])
    for i, got in enumerate(out32):
        ref = torch.cat([o[i] for o in out4], 0)
        assert got.shape == ref.shape and got.shape[0] == 32
        rep = flip_masked(f"L-K B32 disp_{i}", got, ref, flips, margin, 4)
        print(f"L-K B32 vs 8 x B4 disp_{i}: {rep}")
