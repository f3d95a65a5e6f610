"""GPU tests on poisoned LDS (tests/lds_poison.py): no kernel's result may depend on what the previous kernel left
in LDS.

(a) The premise, measured on the machine: a pattern written by esm_lds_fill_u32 is what the next launch finds in every
    word of every CU's LDS (0 mismatches per workgroup of the probe, every CU seen), and the probe, a kernel whose
    output depends on leftovers only, reports all 40,960 words when the pattern is another one: the positive control
    of ``assert_leftover_free``.  Where the pattern does not survive (the driver clears LDS between dispatches, or
    another process interleaves) the remaining tests skip with that reason.
(b) Every op family at the shapes of tests/test_gpu_layouts.py (ragged on purpose: Cin no multiple of 4, Cout no
    multiple of 16, W no multiple of 16, odd D, B 2), contiguous placement, each forced form asserted: one plain run,
    then a run behind each poison pattern, bitwise the same and finite wherever the plain run is.  There is no CPU
    reference here: the fp64 parity of the same cases is asserted by the layouts and parity tests.
(c) Every launch of the real launch lists (tests/shape_classes.py CASES up to KITTI size at B 1, and the six hot_*
    fixtures): the plan's ops stepped one by one with a fill before each, outputs bitwise the plain run's.  A failure
    names the first op whose poisoning alone changes the result.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

import shape_classes as S
from helpers import feature_pair, load_golden
from lds_poison import LDS_WORDS, PATTERNS, assert_leftover_free, fill, probe

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

import esmstereo_amd as E  # noqa: E402
from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd._lib import HINT_GWC_STEM_WLDS  # noqa: E402
from esmstereo_amd._lib import HINT_ROWS as ROWS  # noqa: E402
from esmstereo_amd.backbone import StubFeature  # noqa: E402
from esmstereo_amd.engine import ACT_GELU, ACT_SILU, Ctx, run_conv  # noqa: E402
from test_gpu_layouts import (CONV_CASES, DWCONV_CASES, PAIR_CASES, SHUFFLE_CONV_CASES, SHUFFLE_TAIL_CASES,  # noqa: E402
                              UP1_LAYOUT_CASES, _form, _head, conv_case)
from test_gpu_parity import HOT, _mk, _model_from_manifest, cu, pk  # noqa: E402

DEV = torch.device("cuda")
B = 2


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


# ----------------------------------------------------------------------------- (a) the premise


@pytest.fixture(scope="module")
def premise():
    a, b = PATTERNS
    fill(a)
    same = probe(a)
    fill(b)
    other = probe(a)
    return dict(same=same, other=other, cus=int(torch.unique(same[:, 1]).numel()),
                holds=bool((same[:, 0] == 0).all()) and bool((other[:, 0] == LDS_WORDS).all()))


@pytest.fixture
def poisoned(premise):
    if not premise["holds"]:
        pytest.skip("LDS patterns do not survive to the next launch on this machine "
                    f"(mismatching words per workgroup: same pattern up to {int(premise['same'][:, 0].max())}, "
                    f"other pattern down to {int(premise['other'][:, 0].min())} of {LDS_WORDS})")


def test_fill_reaches_every_cu_and_the_probe_sees_leftovers(premise):
    same, other = premise["same"], premise["other"]
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    print(f"LDS premise: {same.shape[0]} probe workgroups on {premise['cus']} distinct CUs (device: {cus}); "
          f"mismatching words per workgroup, same pattern: max {int(same[:, 0].max())}; "
          f"other pattern: min {int(other[:, 0].min())} max {int(other[:, 0].max())} of {LDS_WORDS}")
    assert same.shape[0] == 8 * cus
    assert bool((same[:, 0] == 0).all()), "a filled pattern must be what the next launch finds in every LDS word"
    assert premise["cus"] == cus, "the probe's workgroups must have run on every CU"
    # the positive control: a kernel whose output depends on leftovers, and the harness sees it
    assert bool((other[:, 0] == LDS_WORDS).all())
    assert int(torch.unique(other[:, 1]).numel()) == cus


# ----------------------------------------------------------------------------- (b) op families


# (two rows of the table are about the placement alone: contiguous, "wide-steps-aside" is the launch of "wide-k3-2src"
# and "pointwise-strided-planes" that of "pointwise-2d")
CONTIGUOUS_CONV_CASES = [c for c in CONV_CASES if c.name not in ("wide-steps-aside", "pointwise-strided-planes")]


@pytest.mark.parametrize("case", CONTIGUOUS_CONV_CASES, ids=lambda c: c.name)
def test_conv_forms(case, poisoned):
    c = case
    pc, xs, ops, kw, _, oshape = conv_case(c)
    srcs = [x.to(DEV) for x in xs]
    o = {k: v.to(DEV) for k, v in ops.items()}
    outs = [torch.zeros(oshape, device=DEV) for _ in range(2 if "out2" in c.epi else 1)]
    for hint in c.hints:
        ckw = dict(o, shuffle=c.shuffle, post_scale=c.post, hint=hint, **kw)
        if len(outs) == 2:
            ckw.update(out2=outs[1], post_scale2=0.5)
        assert _form(pc, srcs, outs[0], **ckw) == c.form, (c.name, hex(hint))
        ctx = Ctx(DEV)
        assert_leftover_free(lambda: run_conv(ctx, pc, srcs, outs[0], **ckw), outs, f"{c.name} hint {hint:#x}")


@pytest.mark.parametrize("name,nd,cins,ka,sa,pa,kb,coutb,shape,ksplit", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_conv_pair(name, nd, cins, ka, sa, pa, kb, coutb, shape, ksplit, poisoned):
    from esmstereo_amd.engine import run_pair2
    ca, ba = _mk(nd, sum(cins), 16, ka, sa, pa, seed=31 + len(name))
    cb, bb = _mk(nd, 16, coutb, kb, 1, kb // 2, seed=32 + len(name))
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    xs = [_randn(B, c, *shape, seed=i) for i, c in enumerate(cins)]
    ctx = Ctx(DEV)
    out = run_pair2(ctx, pa_, xs, pb_, force=True, ksplit=ksplit)
    assert ctx.meta[-1]["kind"] == "conv_pair" and ctx.meta[-1]["form"] == ("ksplit" if ksplit else "lds")
    assert_leftover_free(lambda: run_pair2(ctx, pa_, xs, pb_, force=True, ksplit=ksplit, out=out), [out], name)


def test_conv_pair_regress(poisoned):
    from esmstereo_amd.engine import run_pair2
    D, H, W = 5, 7, 19
    ca, ba = _mk(2, 1, 16, 5, 1, 1, seed=41)
    cb, bb = _mk(2, 16, 16, 3, 1, 1, seed=42)
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    cost = _randn(B, D, H, W)
    init = torch.zeros(B, 1, H, W, device=DEV)
    ctx = Ctx(DEV)
    out = run_pair2(ctx, pa_, [init], pb_, force=True, regress=cost)
    assert ctx.meta[-1]["name"].startswith("disparity_regression+")
    assert_leftover_free(lambda: run_pair2(ctx, pa_, [init], pb_, force=True, regress=cost, out=out), [out, init],
                         "pair regress")


@pytest.mark.parametrize("name,nd,cin,cy,cxs,coutb,grid,crop,hint", UP1_LAYOUT_CASES, ids=[c[0] for c in UP1_LAYOUT_CASES])
def test_convt_1x1(name, nd, cin, cy, cxs, coutb, grid, crop, hint, poisoned):
    from esmstereo_amd.engine import convt_1x1_supported, run_convt_1x1
    ca, ba = _mk(nd, cin, cy, 4, 2, 1, transposed=True, seed=51 + cin)
    cb, bb = _mk(nd, cy + sum(cxs), coutb, 1, 1, 0, seed=52 + coutb)
    pa_, pb_ = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    x = _randn(B, cin, *grid)
    xs = [_randn(B, c, *crop, seed=1 + i) for i, c in enumerate(cxs)]
    assert convt_1x1_supported(pa_, pb_, xs)
    ctx = Ctx(DEV)
    old = dict(EN.HINT_SET)
    EN.HINT_SET["convT"] = hint
    try:
        out = run_convt_1x1(ctx, pa_, [x], pb_, xs)
        assert_leftover_free(lambda: run_convt_1x1(ctx, pa_, [x], pb_, xs, out=out), [out], name)
    finally:
        EN.HINT_SET.clear()
        EN.HINT_SET.update(old)


def test_gwc_stem(poisoned):
    from esmstereo_amd.engine import run_gwc_stem
    G, D, H, W = 8, 5, 7, 20
    conv, bn = _mk(3, G, 8, 3, 1, 1, seed=G + D)
    p = pk(conv, bn, ACT_GELU)
    L, R = (t.to(DEV) for t in feature_pair(B, 2 * G, H, W, 7, D))
    ctx = Ctx(DEV)
    for hint in (0, ROWS(2), ROWS(3), HINT_GWC_STEM_WLDS, ROWS(2) | HINT_GWC_STEM_WLDS):
        out = run_gwc_stem(ctx, p, L, R, G, D, hint=hint)
        assert_leftover_free(lambda: run_gwc_stem(ctx, p, L, R, G, D, hint=hint, out=out), [out], f"gwc_stem {hint:#x}")


@pytest.mark.parametrize("nf,r,H,W,forms", SHUFFLE_TAIL_CASES)
def test_shuffle_tail(nf, r, H, W, forms, poisoned):
    p, _ = _head(nf, r, nf * 100 + r)
    x = _randn(B, nf, H, W)
    ctx = Ctx(DEV)
    for form in forms:
        out = EN.run_shuffle_tail(ctx, x, p, form=form)
        assert_leftover_free(lambda: EN.run_shuffle_tail(ctx, x, p, out=out, form=form), [out], f"shuffle_tail form {form}")


@pytest.mark.parametrize("nf,r,C,H,W,forms", SHUFFLE_CONV_CASES)
def test_shuffle_conv(nf, r, C, H, W, forms, poisoned):
    p, _ = _head(nf, r, nf * 1000 + r * 10 + H)
    conv, bn = _mk(2, 1, C, 3, 2, 1, seed=H)
    pc = pk(conv, bn, ACT_GELU)
    x = _randn(B, nf, H, W)
    ctx = Ctx(DEV)
    for form in forms:
        out = EN.run_shuffle_conv(ctx, x, p, pc, form=form)
        assert_leftover_free(lambda: EN.run_shuffle_conv(ctx, x, p, pc, form=form, out=out), [out],
                             f"shuffle_conv form {form}")


@pytest.mark.parametrize("cp", [12, 16])
def test_shuffle_conv_pre(cp, poisoned):
    """The row-form launch with the stage's spx conv inside it, and with conv1[1] behind it at each of its tiles."""
    H, W = 7, 21
    p, _ = _head(8, 4, cp * 100 + H)
    pconv, pbn = _mk(2, cp, 8, 3, 1, 1, seed=H + 1)
    conv, bn = _mk(2, 1, 16, 3, 2, 1, seed=H)
    conv2, bn2 = _mk(2, 16, 16, 3, 1, 1, seed=H + 2)
    pc, pp, pc2 = pk(conv, bn, ACT_GELU), pk(pconv, pbn, ACT_GELU), pk(conv2, bn2, ACT_GELU)
    c = _randn(B, cp, H, W)
    ctx = Ctx(DEV)
    old = EN.SC11_TILE
    try:
        for form, second, tile in ((2, None, old), (3, None, old), (0, pc2, 0), (0, pc2, 1), (0, pc2, 2)):
            EN.SC11_TILE = tile
            out = EN.run_shuffle_conv(ctx, c, p, pc, pre=pp, form=form, conv2=second)
            if second is not None:
                assert ctx.meta[-1]["form"] == f"row+pre+conv2/tile{tile}"
            assert_leftover_free(lambda: EN.run_shuffle_conv(ctx, c, p, pc, pre=pp, form=form, conv2=second, out=out),
                                 [out], f"shuffle_conv pre form {form} conv2 {second is not None} tile {tile}")
    finally:
        EN.SC11_TILE = old


@pytest.mark.parametrize("k,s", DWCONV_CASES)
def test_dwconv(k, s, poisoned):
    C, H, W = 5, 9, 21
    g = torch.Generator().manual_seed(k * 10 + s)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    w = (torch.randn(C, k * k, generator=g) * 0.3).to(DEV)
    sc, sh = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    p = (k - 1) // 2 if s == 1 else ((s - 1) + (k - 1)) // 2
    ctx = Ctx(DEV)
    out = EN.run_dwconv(ctx, x, w, sc, sh, k, s, p, ACT_SILU)
    assert_leftover_free(lambda: EN.run_dwconv(ctx, x, w, sc, sh, k, s, p, ACT_SILU, out=out), [out], f"dwconv k{k} s{s}")


@pytest.mark.parametrize("C", [8, 16])
def test_smix_fmnet(C, poisoned):
    """ShuffleMixer launches (smix.hip): the three smix launches, FMBlock.net in one launch, the whole block in one
    launch and in two."""
    H, W = 7, 13
    torch.manual_seed(7)
    blk = E.FMBlock(C, 7, 2).eval()
    with torch.no_grad():
        for n, prm in blk.named_parameters():
            if n.endswith("norm1.body.weight") or n.endswith("norm2.body.weight"):
                prm.uniform_(0.8, 1.2)
    p = blk.to(DEV)._packed()
    st = [p["a1"], p["a2"], p["b1"], p["b2"]]
    x = _randn(B, C, H, W)
    ctx = Ctx(DEV)
    out, work = torch.zeros(B, C, H, W, device=DEV), torch.zeros(B, C, H, W, device=DEV)
    assert_leftover_free(lambda: EN.run_fmnet(ctx, x, st, p["dw0"], p["dw1"], out=out), [out], "fmnet net")
    assert_leftover_free(lambda: EN.run_fmnet(ctx, x, st, p["dw0"], p["dw1"], out=out, conv=p["cw"], two_launch=False),
                         [out], "fmnet whole block")
    assert_leftover_free(lambda: EN.run_fmnet(ctx, x, st, p["dw0"], p["dw1"], out=out, conv=p["cw"], two_launch=True,
                                              work=work), [out, work], "fmnet two launches")
    t1, t2, t3 = (torch.zeros(B, C, H, W, device=DEV) for _ in range(3))
    assert_leftover_free(lambda: EN.run_smix(ctx, x, [p["a1"]], out=t1), [t1], "smix 1")
    assert_leftover_free(lambda: EN.run_smix(ctx, t1, [p["a2"], p["b1"]], dw=p["dw0"], out=t2), [t2], "smix 2 + dw")
    assert_leftover_free(lambda: EN.run_smix(ctx, t2, [p["b2"]], dw=p["dw1"], res=x, out=t3), [t3], "smix 3 + dw + res")


def test_volumes(poisoned):
    """The gwc (with and without attention), concat and norm-corr volumes (volumes.hip), H x W = 5 x 19, D 9."""
    C, G, D, H, W = 16, 8, 9, 5, 19
    L, R = (t.to(DEV) for t in feature_pair(B, C, H, W, 5, D))
    att = (torch.rand(B, G, H, W, generator=torch.Generator().manual_seed(1)) + 0.5).to(DEV)
    ctx = Ctx(DEV)
    V = torch.zeros(B, G, D, H, W, device=DEV)
    assert_leftover_free(lambda: ctx.gwc(L, R, None, V, B, C, H, W, D, G), [V], "gwc")
    assert_leftover_free(lambda: ctx.gwc(L, R, att, V, B, C, H, W, D, G), [V], "gwc * att")
    Vc = torch.zeros(B, 2 * C, D, H, W, device=DEV)
    assert_leftover_free(lambda: ctx.concat(L, R, Vc, B, C, H, W, D), [Vc], "concat")
    Vn, work = torch.zeros(B, 1, D, H, W, device=DEV), torch.zeros(2, B, C, H, W, device=DEV)
    assert_leftover_free(lambda: ctx.normcorr(L, R, Vn, work, B, C, H, W, D), [Vn], "normcorr")


def test_confidence_ops(poisoned):
    """The five esm_conf_f32 stages (confidence.hip) at the shapes of test_confidence_ops_carved."""
    from esmstereo_amd._lib import CONF_ATTEND, CONF_COMBINE, CONF_COST_FEATURES, CONF_ENLARGE, CONF_SIGMOID
    C, D, H, W = 5, 9, 5, 19
    ctx = Ctx(DEV)

    def stage(op, xs, oshape, c, d, what):
        out = torch.zeros(oshape, device=DEV)
        assert_leftover_free(lambda: ctx.conf(op, xs, out, B, c, d, H, W), [out], what)

    stage(CONF_COST_FEATURES, [_randn(B, D, H, W, seed=1)], (B, 7, H, W), 0, D, "cost features")
    stage(CONF_ATTEND, [_randn(B, C, H, W, seed=2 + i) for i in range(3)] + [_randn(B, 3, H, W, seed=5)],
          (B, 3 * C, H, W), C, 0, "attend")
    scale = 2 * torch.sigmoid(3 * _randn(B, 1, H, W, seed=7))
    stage(CONF_ENLARGE, [_randn(B, C, H, W, seed=6), scale], (B, 9 * C, H, W), C, 0, "enlarge")
    stage(CONF_COMBINE, [_randn(B, 9, 4 * H, 4 * W, seed=8), _randn(B, 1, H, W, seed=9)], (B, 1, 4 * H, 4 * W), 0, 0,
          "combine")
    stage(CONF_SIGMOID, [_randn(B, 1, H, W, seed=10) * 8], (B, 1, H, W), 1, 0, "sigmoid")


@pytest.mark.parametrize("name", ["c37", "c312"])
def test_metrics(name, poisoned):
    """disparity_metrics (both launches) and the error image (metrics.hip).  The front ends allocate their outputs
    per call (torch.empty: no launch), so the outputs are read off the last call."""
    import metrics_ref as MR
    from esmstereo_amd import metrics as EM
    est, gt, mask, _ = MR.make_inputs(name)
    e, g, m = (torch.from_numpy(np.array(a)).to(DEV) for a in (est, gt, mask))
    last = []

    def metrics():
        r = EM.disparity_metrics(e, g, m)
        last[:] = [r.records, r.values, r.batch]

    def vis():
        last[:] = [EM.vis(e, g)]

    assert_leftover_free(metrics, lambda: last, f"disparity_metrics {name}")
    assert_leftover_free(vis, lambda: last, f"vis {name}")


@pytest.mark.parametrize("mode", ["scale", "range", "depth"])
def test_render(mode, poisoned):
    """One case per mode of tests/test_gpu_render.py (render.hip keeps its colour table in LDS): 3 x 67 x 131, five
    workgroups and partial ranges per image."""
    import test_gpu_render as TR
    d, lut = TR.dev(TR.CASES["3x67x131"]), TR.dev(TR.LUT)
    top = TR.dev(TR.frames("3x67x131")) if mode == "scale" else None
    last = []

    def launch():
        last[:] = [TR.run(mode, d, lut, top)]

    assert_leftover_free(launch, lambda: last, f"render {mode}")


# ----------------------------------------------------------------------------- (c) the real launch lists, stepped

KITTI_PIX = 384 * 1248
_CFG = {c: i for i, c in enumerate(S.CONFIGS)}
LIST_CASES = sorted((c for c in S.CASES if c[2] * c[3] * c[4] <= KITTI_PIX),
                    key=lambda c: (_CFG[c[0]], c[1], c[2] * c[3] * c[4], c[2], c[3], c[4]))


def _stepped(hp, pattern, only=None):
    """The plan's ops one by one, LDS filled with ``pattern`` before each (``only``: before that op alone)."""
    for i in range(hp.num_ops):
        if only is None or i == only:
            fill(pattern)
        hp.run_op(i)
    torch.cuda.synchronize()


def _same(hp, want):
    return all(torch.equal(a, b) for a, b in zip(hp.outputs, want))


def _check_launch_list(model, inputs, name):
    want = model.hot_path(*inputs, True)  # (clones of the plan's output buffers)
    torch.cuda.synchronize()
    hp = next(reversed(model._plans.values()))
    assert len(want) == len(hp.outputs) and hp.num_ops == len(hp.ctx.meta)
    for pattern in PATTERNS:
        _stepped(hp, pattern)
        if _same(hp, want):
            continue
        for j in range(hp.num_ops):  # bisect: which op's own poisoning changes the result
            _stepped(hp, pattern, only=j)
            if not _same(hp, want):
                m = hp.ctx.meta[j]
                raise AssertionError(f"{name}: op {j} of {hp.num_ops}, {m['name']} ({m['kind']}, {m.get('shape', '')}), "
                                     f"depends on LDS leftovers (pattern {pattern:#010x})")
        raise AssertionError(f"{name}: the outputs change with LDS pattern {pattern:#010x} before every op, "
                             "but with no single op's poisoning alone")


@pytest.fixture(scope="module")
def group():
    """The model of the current (config, maxdisp), as tests/test_gpu_shape_classes.py shares it."""
    st = {"key": None, "model": None}
    yield st
    if st["model"] is not None:
        st["model"].invalidate_plans()


@pytest.mark.parametrize("case", LIST_CASES, ids=S.case_id)
def test_launch_list_stepped(case, group, poisoned):
    cfg, md = case[:2]
    if group["key"] != (cfg, md):
        if group["model"] is not None:
            group["model"].invalidate_plans()
        _, cv, bb, cvs, _ = S.CONFIGS[cfg]
        with contextlib.redirect_stdout(io.StringIO()):  # (the constructor names its cost volume)
            model = E.ESMStereo(md, cv == "gwc", cv == "nc", bb, cvs, feature_cls=StubFeature)
        model.load_state_dict(S.state(cfg))
        group.update(key=(cfg, md), model=model.eval().to(DEV))
    ml, mr, att, up = S.case_inputs(case)
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    _check_launch_list(group["model"], (dev(ml), dev(mr), dev(att), [dev(u) for u in up]), S.case_id(case))


@pytest.mark.parametrize("name", HOT)
def test_hot_fixture_stepped(name, poisoned):
    model, _, _ = _model_from_manifest(name)
    g = load_golden(name)
    up = [cu(g[f"up_{i}"]) for i in range(4) if f"up_{i}" in g]
    att = cu(g["att"]) if "att" in g else None
    try:
        _check_launch_list(model, (cu(g["match_left"]), cu(g["match_right"]), att, up), name)
    finally:
        model.invalidate_plans()
