"""GPU descriptor-domain tests: every conv entry point over every descriptor it accepts (tests/conv_domain.py).

The parity and layout tests run each kernel form at the handful of descriptors the hot path sends.  ``conv_check``
accepts far more, and each form decides in its own ``*_ok`` predicate what it runs.  One test per (form, geometry)
base walks that base's cases (one axis at a time: padding 0..k, every extent over 1..9 and the tile edges, channel
counts and source splits, the six activations, BN / bias / neither, every epilogue operand, batch, the form's hint
fields; plus the form's seeded random combinations) and holds each launch, with the forced hint and with hint 0, to

  * acceptance implies correctness: where ``ACCEPTS[form]`` is true the query reports the form, the launch returns
    ESM_OK, the output is finite and ``|y - ref| <= 1e-5 * max A`` over every element (``out2`` the same against
    ``ref * post_scale2``);
  * refusal is the documented one: where it is false, ``REFUSAL[form]``: the message through ESM_ERR_ARG, or the form it
    steps aside for, held to the same comparison.  An undocumented acceptance fails;
  * hint 0 never refuses in the supported geometry, and is ESM_ERR_UNSUPPORTED outside it at every size.

``ref`` is ``_ref_conv`` in fp64.  ``A`` is the same expression on ``|x|``, ``|w|``, ``|scale|``, ``|shift|``, ``|mul|``,
``|res|``, ``|up|`` without the activation, the forward-error scale of the sum (1 for a sigmoid, whose value lies in
[0, 1]): these outputs can have one or two elements, where a cancelling sum makes ``max |ref|`` arbitrarily small.
Contiguous device tensors, the default stream, B <= 3; every operand is a real tensor of its descriptor's size.

Worst ``|y - ref| / max A`` per form (MI355X): DESIGN 5, "Descriptor domain".
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conv_domain import ACCEPTS, BASES, FORM_ID, FORM_NAME, OUTSIDE, SUPPORTED_GEOMETRY, cases_of, expected
from test_gpu_parity import _mk, _ref_conv, pk

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd._lib import ACT_SIGMOID  # noqa: E402
from esmstereo_amd.engine import Ctx  # noqa: E402

DEV = torch.device("cuda")
TOL = 1e-5       # the project's conv tolerance
POST2 = 0.5      # out2's scale
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def affine64(conv, bn):
    """The folded epilogue constants (engine.pack_conv) in fp64: per-cout scale and shift."""
    cout = conv.out_channels
    bias = conv.bias.detach().double() if conv.bias is not None else torch.zeros(cout, dtype=torch.float64)
    if bn is None:
        return torch.ones(cout, dtype=torch.float64), bias
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.double() * scale + bias * scale


def error_scale(xs, conv, bn, act, shuffle, mul=None, res=None, up=None):
    """A: ``_ref_conv``'s expression on absolute values, without the activation."""
    nd = conv.weight.dim() - 2
    tr = isinstance(conv, (torch.nn.ConvTranspose2d, torch.nn.ConvTranspose3d))
    fn = {(2, False): F.conv2d, (3, False): F.conv3d, (2, True): F.conv_transpose2d, (3, True): F.conv_transpose3d}[(nd, tr)]
    a = fn(torch.cat([t.double().abs() for t in xs], 1), conv.weight.detach().double().abs(), None, conv.stride, conv.padding)
    scale, shift = affine64(conv, bn)
    bc = (None, slice(None)) + (None,) * nd
    a = a * scale.abs()[bc] + shift.abs()[bc]
    if shuffle > 1:
        a = F.pixel_shuffle(a, shuffle)
    if act == ACT_SIGMOID:
        a = torch.ones_like(a)
    if mul is not None:
        a = a * (mul.double().abs().unsqueeze(2) if nd == 3 else mul.double().abs())
    if res is not None:
        a = a + res.double().abs()
    if up is not None:
        a = a + F.interpolate(up.double().abs(), scale_factor=2, mode="bilinear", align_corners=False)
    return a


class Operands:
    """A case's layer, CPU operands, fp64 reference and error scale, and their device copies."""

    def __init__(self, c):
        s = c.spec
        conv, bn = _mk(s.nd, s.cin, s.cout, s.k, s.s, s.p, transposed=s.transposed, bn=c.bn == "bn", bias=c.bn == "bias",
                       seed=c.seed)
        if bn is not None:
            bn.weight.data *= c.gain
        g = torch.Generator().manual_seed(c.seed)
        xs = [torch.randn(s.B, ci, *s.in_ext, generator=g) for ci in s.cins]
        r = s.shuffle
        ext = s.out_ext
        self.oshape = (s.B, s.cout // (r * r), ext[0] * r, ext[1] * r) if r > 1 else (s.B, s.cout) + ext
        ops = {}
        if s.m:  # [B, Cout, Ho, Wo], broadcast over D
            ops["mul"] = torch.rand((s.B, s.cout) + ext[-2:], generator=g) + 0.5
        if s.r:
            ops["res"] = torch.randn(self.oshape, generator=g)
        if s.u:
            ops["up"] = torch.randn(s.B, 1, ext[-2] // 2, ext[-1] // 2, generator=g)
        self.ref = _ref_conv(xs, conv, bn, c.act, shuffle=r, up_f=2 if s.u else 0, **ops).detach().double()
        assert tuple(self.ref.shape) == self.oshape
        self.amax = float(error_scale(xs, conv, bn, c.act, r, **ops).max())
        self.pc = pk(conv, bn, c.act)
        self.srcs = [x.to(DEV) for x in xs]
        self.ops = {k: v.to(DEV) for k, v in ops.items()}
        self.case = c

    def launch(self, hint):
        """(reported form, status, message, out, out2) of one esm_conv_f32 call with ``hint`` exactly."""
        c, s = self.case, self.case.spec
        out = torch.full(self.oshape, float("nan"), device=DEV)
        out2 = torch.full(self.oshape, float("nan"), device=DEV) if s.two else None
        ctx = Ctx(DEV)
        d, _, _ = EN._conv_desc(ctx, self.pc, self.srcs, out, up_f=2 if s.u else 0, post_scale=c.post, shuffle=s.shuffle,
                                out2=out2, post_scale2=POST2, hint=hint, **self.ops)
        d.hint = hint  # (no tuned row, no tile-order bit)
        form = _lib.lib.esm_conv_form(ctypes.byref(d))
        rc = _lib.lib.esm_conv_f32(ctypes.byref(d), ctx.stream)
        msg = (_lib.lib.esm_last_error() or b"").decode() if rc < 0 else ""
        return form, rc, msg, out, out2

    def error(self, out, out2):
        """Worst ``|y - ref| / max A`` over out and out2 (inf: a cell not finite or not written)."""
        worst = 0.0
        for y, scale in ((out, self.case.post), (out2, POST2)):
            if y is None:
                continue
            y = y.double().cpu()
            if not bool(torch.isfinite(y).all()):
                return float("inf")
            worst = max(worst, float((y - self.ref * scale).abs().max()) / (self.amax * scale))
        return worst


def walk(cases):
    """Every case with its forced hint and with hint 0; returns (failures, worst error of the forced form's own runs,
    forms hint 0 took)."""
    fails, worst, autos = [], 0.0, {}
    for c in cases:
        o = Operands(c)
        kind, form = expected(c)
        f0, rc0, msg0, y0, y20 = o.launch(0)
        if rc0 != 0:
            fails.append((c.id, "hint 0 refused", rc0, msg0))
        else:
            e0 = o.error(y0, y20)
            autos[FORM_NAME[f0]] = max(autos.get(FORM_NAME[f0], 0.0), e0)
            if not e0 <= TOL:
                fails.append((c.id, f"hint 0 ({FORM_NAME[f0]})", e0))
            if not ACCEPTS[FORM_NAME[f0]](c):
                fails.append((c.id, "hint 0 took a form that does not run the case", FORM_NAME[f0]))
        f, rc, msg, y, y2 = o.launch(c.hint)
        if kind == "refused":
            if rc != ERR_ARG or form not in msg:
                fails.append((c.id, "undocumented outcome of a refusal", rc, msg, f))
            continue
        if rc != 0:
            fails.append((c.id, "refused", rc, msg))
            continue
        if kind == "runs" and f != FORM_ID[form]:
            fails.append((c.id, "another form ran", f, form))
        if kind == "auto" and (f != f0 or f == FORM_ID[c.form]):
            fails.append((c.id, "did not step aside for the automatic rules", f, f0))
        e = o.error(y, y2)
        if kind == "runs":
            worst = max(worst, e)
        if not e <= TOL:
            fails.append((c.id, f"forced ({kind})", e))
    return fails, worst, autos


@pytest.mark.parametrize("base", BASES, ids=lambda b: b.name)
def test_conv_domain(base):
    cases = cases_of(base)
    assert all(SUPPORTED_GEOMETRY(c) for c in cases)
    fails, worst, autos = walk(cases)
    print(f"\nDOMAIN {base.name}: {len(cases)} cases, {len(fails)} failures, worst forced {worst:.2e}, hint 0 "
          + " ".join(f"{k} {v:.2e}" for k, v in sorted(autos.items())))
    assert not fails, f"{len(fails)} of {len(cases)} cases: " + "; ".join(map(str, fails[:6]))


@pytest.mark.parametrize("case", OUTSIDE, ids=lambda c: c.value)
def test_outside_the_supported_geometry_is_unsupported(case):
    """A (kernel, stride) pair no form instantiates: ESM_ERR_UNSUPPORTED with hint 0, whatever the map size, and
    nothing is written."""
    s = case.spec
    conv, bn = _mk(s.nd, s.cin, s.cout, s.k, s.s, s.p, seed=1)
    x = torch.zeros(s.B, s.cin, *s.in_ext, device=DEV)
    out = torch.full((s.B, s.cout) + s.out_ext, 7.0, device=DEV)
    ctx = Ctx(DEV)
    d, _, _ = EN._conv_desc(ctx, pk(conv, bn, case.act), [x], out, hint=0)
    d.hint = 0
    assert _lib.lib.esm_conv_form(ctypes.byref(d)) == _lib.FORM_GENERAL
    assert _lib.lib.esm_conv_f32(ctypes.byref(d), ctx.stream) == ERR_UNSUPPORTED
    assert b"unsupported kernel/stride" in _lib.lib.esm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ----------------------------------------------------------------------------- fused launches

from conv_domain_fused import PAIR_CASES, UP1_CASES, pair_query, up1_query  # noqa: E402
from esmstereo_amd._lib import ACT_GELU, HINT_PAIRK  # noqa: E402


def _dev_tensor(*shape):
    return torch.empty(shape, device=DEV)


_WORST = [0.0]  # the worst error of the fused cases walked so far (printed per test)


def _held(y, ref, amax):
    """``|y - ref| / max A`` (inf where a cell is not finite)."""
    y = y.double().cpu()
    e = float((y - ref).abs().max()) / amax if bool(torch.isfinite(y).all()) else float("inf")
    _WORST[0] = max(_WORST[0], e)
    return e


def _check_pair(c):
    lds, ks = pair_query(c, _dev_tensor)
    ca, ba = _mk(c.nd, sum(c.cins), c.couta, c.ka, c.sa, c.pa, seed=len(c.id))
    cb, bb = _mk(c.nd, c.couta, c.coutb, c.kb, 1, c.pb, seed=len(c.id) + 1)
    g = torch.Generator().manual_seed(len(c.id))
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    out = []
    if c.regress:  # the pair's first input is the disparity regression of a cost volume, computed in the launch
        D = 5
        cost = torch.randn(c.B, D, *c.shape, generator=g)
        dd = torch.arange(D, dtype=torch.float64).view(1, D, 1, 1)
        xs = [(cost.double() * dd).sum(1, keepdim=True)]
        xabs = [(cost.double().abs() * dd).sum(1, keepdim=True)]
    else:
        xs = [torch.randn(c.B, ci, *c.shape, generator=g) for ci in c.cins]
        xabs = xs
    ref = _ref_conv([_ref_conv(xs, ca, ba, ACT_GELU).double()], cb, bb, ACT_GELU).detach().double()
    amax = float(error_scale([error_scale(xabs, ca, ba, ACT_GELU, 1)], cb, bb, ACT_GELU, 1).max())
    if c.regress:  # through the engine alone (it builds the cost volume's descriptor)
        init = torch.full((c.B, 1) + c.shape, float("nan"), device=DEV)
        ctx = Ctx(DEV)
        try:
            y = EN.run_pair2(ctx, pa_, [init], pb_, force=True, regress=cost.to(DEV))
        except _lib.EsmError as e:
            return [(c.id, f"query lds {lds}, the launcher refused", str(e))]
        fused = ctx.meta[-1]["name"].startswith("disparity_regression+")
        if fused != (lds and c.kb == 3):
            out.append((c.id, "regression fused", fused, lds))
        e = max(_held(y, ref, amax), _held(init, xs[0], float(xabs[0].max())))
        return out + ([(c.id, "regress pair", e)] if not e <= TOL else [])
    srcs = [x.to(DEV) for x in xs]
    ctx = Ctx(DEV)
    da, _, _ = EN._conv_desc(ctx, pa_, srcs, hint=1, alloc_out=False)  # (as engine.run_pair2 builds the two)
    da.hint = 0
    virt = srcs[0].as_strided((c.B, c.couta) + c.mid_ext, (0,) * (c.nd + 1) + (1,))
    y = torch.full((c.B, c.coutb) + c.out_ext, float("nan"), device=DEV)
    db, _, _ = EN._conv_desc(ctx, pb_, [virt], y, hint=1)
    db.hint = HINT_PAIRK if c.ksplit else 0
    rc = _lib.lib.esm_conv_pair2_f32(ctypes.byref(da), ctypes.byref(db), ctx.stream)
    if (rc == 0) != (lds or ks):
        return [(c.id, f"query lds {lds} ksplit {ks}, launcher status", rc, _lib.lib.esm_last_error())]
    if rc != 0:
        return [] if rc == ERR_ARG else [(c.id, "status", rc)]
    e = _held(y, ref, amax)
    if not e <= TOL:
        out.append((c.id, "pair", e))
    if (ks if c.ksplit else lds):  # the engine's own path to the same form
        ctx = Ctx(DEV)
        y2 = EN.run_pair2(ctx, pa_, srcs, pb_, force=True, ksplit=c.ksplit)
        if ctx.meta[-1]["kind"] != "conv_pair" or not torch.equal(y2, y):
            out.append((c.id, "engine.run_pair2 differs from the direct call"))
    return out


def _check_up1(c):
    want = up1_query(c, _dev_tensor)
    ca, ba = _mk(c.nd, c.cin, c.cy, 4, 2, 1, transposed=True, seed=len(c.id))
    cb, bb = _mk(c.nd, c.cy + sum(c.cxs), c.coutb, 1, 1, 0, seed=len(c.id) + 1)
    g = torch.Generator().manual_seed(len(c.id))
    x = torch.randn(c.B, c.cin, *c.grid, generator=g)
    xs = [torch.randn(c.B, cx, *c.out_ext, generator=g) for cx in c.cxs]
    crop = (slice(None), slice(None)) + tuple(slice(0, n) for n in c.out_ext)
    ref = _ref_conv([_ref_conv([x], ca, ba, ACT_GELU)[crop].double(), *xs], cb, bb, ACT_GELU).detach().double()
    amax = float(error_scale([error_scale([x], ca, ba, ACT_GELU, 1)[crop], *xs], cb, bb, ACT_GELU, 1).max())
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    xd, xsd = x.to(DEV), [t.to(DEV) for t in xs]
    ctx = Ctx(DEV)
    da, _, _ = EN._conv_desc(ctx, pa_, [xd], hint=1, alloc_out=False)  # (as engine.run_convt_1x1 builds the two)
    da.hint = c.hint
    virt = xd.as_strided((c.B, c.cy) + c.out_ext, (0,) * (c.nd + 1) + (1,))
    y = torch.full((c.B, c.coutb) + c.out_ext, float("nan"), device=DEV)
    db, _, _ = EN._conv_desc(ctx, pb_, [virt, *xsd], y, hint=1)
    db.hint = 0
    rc = _lib.lib.esm_convt_1x1_f32(ctypes.byref(da), ctypes.byref(db), ctx.stream)
    if (rc == 0) != want:
        return [(c.id, f"query {want}, launcher status", rc, _lib.lib.esm_last_error())]
    if rc != 0:
        return [] if rc == ERR_ARG else [(c.id, "status", rc)]
    e = _held(y, ref, amax)
    return [(c.id, "convt_1x1", e)] if not e <= TOL else []


def _walk_fused(cases, check, what):
    _WORST[0] = 0.0
    fails = [f for c in cases for f in check(c)]
    print(f"\nDOMAIN {what}: {len(cases)} cases, {len(fails)} failures, worst {_WORST[0]:.2e}")
    assert not fails, f"{len(fails)} failures in {len(cases)} cases: " + "; ".join(map(str, fails[:6]))


@pytest.mark.parametrize("name", sorted({c.name for c in PAIR_CASES}))
def test_conv_pair_domain(name):
    """esm_conv_pair2_f32 around each base: ESM_OK exactly where an engine predicate says a form runs the pair (and then
    the fp64 composed reference at 1e-5 of the composed error scale), ESM_ERR_ARG elsewhere."""
    _walk_fused([c for c in PAIR_CASES if c.name == name], _check_pair, f"pair {name}")


@pytest.mark.parametrize("name", sorted({c.name for c in UP1_CASES}))
def test_convt_1x1_domain(name):
    """esm_convt_1x1_f32 around each base, lean and tiled: ESM_OK exactly where engine.convt_1x1_supported says so."""
    _walk_fused([c for c in UP1_CASES if c.name == name], _check_up1, f"convt_1x1 {name}")
