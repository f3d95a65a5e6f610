"""The fused launches' form queries on the CPU: ``esm_conv_pair2_form``, ``esm_convt_1x1_form``, ``esm_shuffle_tail_form``,
``esm_shuffle_conv_form`` and ``esm_gwc_stem_check`` over descriptors with fake addresses.

They apply the checks and the rules of the launches they are named after and launch nothing, so everything here runs
without a device.  ``engine.py``'s predicates are these queries asked about the descriptors a launch would get: for every
case of tests/conv_domain_fused.py the predicate's answer is the answer of the query called directly, on a descriptor
built here from the case alone (test_conv_forms_host.build_desc), and tests/test_gpu_conv_domain.py holds the launchers
to the same answers.  The shuffle heads' automatic rules are pinned on both sides of their thresholds.
"""
import ctypes
from dataclasses import replace

import pytest
import torch

from conv_domain_fused import PAIR_CASES, UP1_CASES, _packed, pair_query, up1_query
from esmstereo_amd import _lib
from esmstereo_amd import engine as EN
from esmstereo_amd._lib import HINT_PAIR_REGRESS, HINT_PAIRK, HINT_SMALL, HINT_TILE
from test_conv_forms_host import build_desc
from tuned_rows import Spec

LIB = _lib.lib
ERR_ARG, ERR_UNSUPPORTED = -1, -3  # ESM_ERR_ARG, ESM_ERR_UNSUPPORTED
FAKE = 1 << 24  # a non-null, 256-aligned address no query reads through


def _shape_only(*shape):
    return torch.empty(shape, device="meta")


def _spec(nd, transposed, k, s, p, cins, cout, B, ext):
    Di, Hi, Wi = ext if nd == 3 else (1,) + tuple(ext)
    return Spec(nd, transposed, k, s, p, tuple(cins), cout, B, Di, Hi, Wi, 1, False, False, False, False)


def pair_descs(c, ksplit=False, regress=False):
    a = build_desc(_spec(c.nd, False, c.ka, c.sa, c.pa, c.cins, c.couta, c.B, c.shape), 0)
    b = build_desc(_spec(c.nd, False, c.kb, 1, c.pb, (c.couta,), c.coutb, c.B, c.mid_ext), HINT_PAIRK if ksplit else 0)
    if regress:  # convA's source: a contiguous [B, 5, H, W] cost volume; its output: the regressed [B, 1, H, W] map
        H, W = c.shape
        a.src[0].C, a.src[0].sb, a.src[0].sc, a.src[0].sh = 5, 5 * H * W, H * W, W
        a.out, a.ob, a.oc, a.oh = FAKE, H * W, H * W, W
        a.hint = HINT_PAIR_REGRESS
    return a, b


def pair_form(c, **kw):
    a, b = pair_descs(c, **kw)
    return LIB.esm_conv_pair2_form(ctypes.byref(a), ctypes.byref(b))


def up1_form(c, hint):
    a = build_desc(_spec(c.nd, True, 4, 2, 1, (c.cin,), c.cy, c.B, c.grid), hint)
    b = build_desc(_spec(c.nd, False, 1, 1, 0, (c.cy,) + c.cxs, c.coutb, c.B, c.out_ext), 0)
    return LIB.esm_convt_1x1_form(ctypes.byref(a), ctypes.byref(b))


def test_pair_predicates_are_the_query():
    """engine._pair2_lds_supported / pairk_supported on every PAIR_CASES entry: esm_conv_pair2_form without / with PAIRK
    names that form.  Each form is named and each is refused somewhere, and a refusal carries the launcher's message."""
    named = {"lds": 0, "ksplit": 0}
    refused = {"lds": 0, "ksplit": 0}
    for c in PAIR_CASES:
        lds, ks = pair_query(c, _shape_only)
        f0, f1 = pair_form(c), pair_form(c, ksplit=True)
        assert lds == (f0 == _lib.PAIR_FORM_LDS), (c.id, lds, f0)
        assert ks == (f1 == _lib.PAIR_FORM_KSPLIT), (c.id, ks, f1)
        assert f0 in (_lib.PAIR_FORM_LDS, _lib.PAIR_FORM_KSPLIT, ERR_ARG) and f1 in (_lib.PAIR_FORM_LDS, _lib.PAIR_FORM_KSPLIT, ERR_ARG)
        assert (f0 == ERR_ARG) == (not lds and not ks), (c.id, f0)  # hint 0: whichever form runs the pair
        named["lds"] += lds
        named["ksplit"] += ks
        refused["lds"] += f0 != _lib.PAIR_FORM_LDS
        refused["ksplit"] += f1 != _lib.PAIR_FORM_KSPLIT
        if f0 == ERR_ARG:
            assert b"conv pair" in LIB.esm_last_error(), c.id
    assert all(named.values()) and all(refused.values()), (named, refused)


def test_only_predicates_take_a_packed_conv_without_tensors():
    """A predicate reads a layer's geometry, so a PackedConv without tensors (weights None, BN constants a bare True)
    answers as one with shape-only tensors.  A launch does not take one: a missing operand raises on the host, in a dry
    emission too, and never becomes an address."""
    for c in PAIR_CASES[::7]:
        bare = [replace(_packed(c.nd, ci, co, k, s, p), w=None, scale=True, shift=True)
                for ci, co, k, s, p in ((sum(c.cins), c.couta, c.ka, c.sa, c.pa), (c.couta, c.coutb, c.kb, 1, c.pb))]
        srcs = [_shape_only(c.B, ci, *c.shape) for ci in c.cins]
        assert (EN._pair2_lds_supported(*bare, srcs), EN.pairk_supported(*bare, srcs)) == pair_query(c, _shape_only), c.id
    c = PAIR_CASES[0]
    assert any(pair_query(c, _shape_only))
    with EN.Ctx("meta", dry=True) as ctx:
        for launch in (lambda: EN.run_pair2(ctx, *bare_pair(c), force=True), lambda: EN.run_conv(ctx, bare_pair(c)[0], bare_pair(c)[1])):
            with pytest.raises((TypeError, AttributeError)):
                launch()
    assert ctx.num_ops == 0
    p = EN.PackedShuffleTail(None, _shape_only(1), _shape_only(1), None, 8, 4)
    with EN.Ctx("meta", dry=True) as ctx, pytest.raises((TypeError, AttributeError)):
        EN.run_shuffle_tail(ctx, _shape_only(1, 8, 8, 16), p)


def bare_pair(c):
    """(pa, srcs, pb) of a pair case with PackedConvs that carry no tensors."""
    pa = replace(_packed(c.nd, sum(c.cins), c.couta, c.ka, c.sa, c.pa), w=None, scale=True, shift=True)
    pb = replace(_packed(c.nd, c.couta, c.coutb, c.kb, 1, c.pb), w=None, scale=True, shift=True)
    return pa, [_shape_only(c.B, ci, *c.shape) for ci in c.cins], pb


def test_pair_regression_source_is_fused_where_the_query_names_the_lds_form():
    """engine.run_pair2 with a cost volume, dry: the regression goes into the pair exactly where esm_conv_pair2_form names
    the LDS form for the descriptors with PAIR_REGRESS; elsewhere it is a launch of its own."""
    cases = [c for c in PAIR_CASES if c.regress]
    cases += [replace(c, regress=True) for c in PAIR_CASES if c.name == "lds-k3s1" and c.axis == "cin" and c.cins == (1,)]
    fused = 0
    for c in cases:
        want = any(pair_query(c, _shape_only)) and pair_form(c, regress=True) == _lib.PAIR_FORM_LDS
        pa, pb = _packed(2, 1, c.couta, c.ka, c.sa, c.pa), _packed(2, c.couta, c.coutb, c.kb, 1, c.pb)
        with EN.Ctx("meta", dry=True) as ctx:
            EN.run_pair2(ctx, pa, [_shape_only(c.B, 1, *c.shape)], pb, force=True, regress=_shape_only(c.B, 5, *c.shape))
        got = ctx.meta[-1]["name"].startswith("disparity_regression+")
        assert got == want, (c.id, got, want)
        assert [m["kind"] for m in ctx.meta].count("regression") == int(not want), c.id
        if got:
            assert ctx.meta[-1]["form"] == "lds+regress"
        fused += got
    assert 0 < fused < len(cases)


def test_convt_1x1_predicate_is_the_query():
    """engine.convt_1x1_supported on every UP1_CASES entry: esm_convt_1x1_form names a form for the descriptors under the
    automatic hint.  Under the case's own hint (SMALL / TILE) each form is named and each is refused somewhere."""
    named = {_lib.UP1_FORM_LEAN: 0, _lib.UP1_FORM_TILED: 0}
    refused = {HINT_SMALL: 0, HINT_TILE: 0}
    for c in UP1_CASES:
        f = up1_form(c, 0)
        assert up1_query(c, _shape_only) == (f > 0), (c.id, f)
        assert f in (_lib.UP1_FORM_LEAN, _lib.UP1_FORM_TILED, ERR_ARG), (c.id, f)
        fh = up1_form(c, c.hint)
        assert (fh > 0) == (f > 0), (c.id, f, fh)  # what one form runs the other runs, in this domain
        if fh > 0:
            named[fh] += 1
            wide = c.cy > 16 or c.coutb > 16
            assert fh == (_lib.UP1_FORM_TILED if wide or c.hint & HINT_TILE else _lib.UP1_FORM_LEAN), (c.id, fh)
        else:
            refused[c.hint & (HINT_SMALL | HINT_TILE)] += 1
            assert b"convt_1x1" in LIB.esm_last_error() or b"conv:" in LIB.esm_last_error(), c.id
    assert all(named.values()) and all(refused.values()), (named, refused)


def test_convt_1x1_query_includes_what_the_forms_launchers_refuse():
    """A named form is a form that runs: a 2-D pair with more than 16 couts under TILE, and a grid past 65535 rows, are
    refused by the query with the launchers' messages."""
    base = next(c for c in UP1_CASES if c.name == "2d-tiled" and c.axis == "base")
    assert up1_form(base, base.hint) == _lib.UP1_FORM_TILED
    assert up1_form(replace(base, coutb=17), base.hint) == ERR_ARG
    lean = next(c for c in UP1_CASES if c.name == "2d-lean" and c.axis == "base")
    assert up1_form(lean, HINT_SMALL) == _lib.UP1_FORM_LEAN
    assert up1_form(replace(lean, grid=(65536, 2)), HINT_SMALL) == ERR_ARG and b"grid too large" in LIB.esm_last_error()
    assert up1_form(replace(lean, grid=(65535, 2)), HINT_SMALL) == _lib.UP1_FORM_LEAN


def test_convt_1x1_supported_without_an_input_takes_the_smallest_that_covers_the_extras():
    """``srcs`` omitted: ceil(extent / 2) per dimension; given: the crop condition is the library's (an input whose
    doubled extent does not cover the extras is refused)."""
    c = next(c for c in UP1_CASES if c.name == "3d-lean" and c.axis == "base")
    pa, pb = _packed(3, c.cin, c.cy, 4, 2, 1, transposed=True), _packed(3, c.cy + sum(c.cxs), c.coutb, 1, 1, 0)
    extra = [_shape_only(c.B, cx, *c.out_ext) for cx in c.cxs]
    assert EN.convt_1x1_supported(pa, pb, extra)
    assert EN.convt_1x1_supported(pa, pb, extra, [_shape_only(c.B, c.cin, *c.grid)])
    small = tuple(v - 1 for v in c.grid)
    assert min(small) > 0 and not EN.convt_1x1_supported(pa, pb, extra, [_shape_only(c.B, c.cin, *small)])


# ----------------------------------------------------------------------------- the shuffle heads


def tail_desc(nf, r, B, H, W, form=0):
    d = _lib.EsmShuffleTailDesc()
    d.x, d.xb, d.xc, d.xh = FAKE, nf * H * W, H * W, W
    d.up_w = d.up_b = d.tail_w = d.tail_b = FAKE
    d.out, d.ob, d.oh = FAKE, H * r * W * r, W * r
    d.B, d.nf, d.H, d.W, d.r = B, nf, H, W, r
    d.flags = (form & 3) << 1
    return d


def tail_form(*a, **kw):
    d = tail_desc(*a, **kw)
    return LIB.esm_shuffle_tail_form(ctypes.byref(d))


def test_shuffle_tail_form_rule_and_forced_forms():
    W, R8, R4 = _lib.SHUFFLE_TAIL_FORM_WINDOW, _lib.SHUFFLE_TAIL_FORM_ROW8, _lib.SHUFFLE_TAIL_FORM_ROW4
    # (nf 8, r 4), B 1, W 16: ceil(64 / 64) x ceil(4 H / 32) x 1 workgroups of 8 rows: 127 at H 1016, 128 at H 1024
    assert tail_form(8, 4, 1, 1016, 16) == W
    assert tail_form(8, 4, 1, 1024, 16) == R8
    for H in (1016, 1024):
        assert [tail_form(8, 4, 1, H, 16, form=f) for f in (1, 2, 3)] == [W, R4, R8]
    # the other heads have the window form only, whatever the flags ask for
    for nf, r in ((8, 2), (16, 2), (16, 4)):
        assert {tail_form(nf, r, 1, 1024, 16, form=f) for f in (0, 1, 2, 3)} == {W}
    assert tail_form(12, 4, 1, 8, 16) == ERR_UNSUPPORTED and b"(nf, r) must be one of" in LIB.esm_last_error()
    assert tail_form(8, 3, 1, 8, 16) == ERR_UNSUPPORTED
    d = tail_desc(8, 4, 1, 8, 16)
    d.out = None
    assert LIB.esm_shuffle_tail_form(ctypes.byref(d)) == ERR_ARG and b"null pointer" in LIB.esm_last_error()
    d = tail_desc(8, 4, 1, 8, 16)
    d.oh = 63
    assert LIB.esm_shuffle_tail_form(ctypes.byref(d)) == ERR_ARG and b"strides" in LIB.esm_last_error()
    assert LIB.esm_shuffle_tail_form(None) == ERR_ARG


def sc_desc(nf, r, C, B, H, W, form=0, pre=False, w2=False, tile=0):
    d = _lib.EsmShuffleConvDesc()
    t = d.st
    t.xb, t.xc, t.xh = nf * H * W, H * W, W
    t.up_w = t.up_b = t.tail_w = t.tail_b = FAKE
    t.B, t.nf, t.H, t.W, t.r = B, nf, H, W, r
    t.flags = (form & 3) << 1 | (tile & 3) << 3
    if pre:
        d.pre_x, d.pb, d.pc, d.ph = FAKE, 12 * H * W, H * W, W
        d.pre_w = d.pre_scale = d.pre_shift = FAKE
        d.pre_cin, d.pre_cin_pad, d.pre_cout_pad = 12, 16, 32
    else:
        t.x = FAKE
    Ho2, Wo2 = (H * r + 1) // 2, (W * r + 1) // 2
    d.w = d.scale = d.shift = d.out = FAKE
    d.ob, d.oc, d.oh = C * Ho2 * Wo2, Ho2 * Wo2, Wo2
    d.C, d.cin_pad, d.cout_pad = C, 16, 32
    if w2:
        d.w2 = d.scale2 = d.shift2 = FAKE
        d.cin_pad2, d.cout_pad2 = 16, 32
    return d


def sc_form(*a, **kw):
    d = sc_desc(*a, **kw)
    return LIB.esm_shuffle_conv_form(ctypes.byref(d))


def test_shuffle_conv_form_rule_pre_conv_second_conv_and_tiles():
    W, VALU, MFMA = _lib.SHUFFLE_CONV_FORM_WINDOW, _lib.SHUFFLE_CONV_FORM_ROW_VALU, _lib.SHUFFLE_CONV_FORM_ROW_MFMA
    PRE, CONV1 = _lib.SHUFFLE_CONV_FORM_PRE, _lib.SHUFFLE_CONV_FORM_CONV1
    # (8, 4, 16), B 1, W 16: ceil(W / 16) x ceil(H / 8) x B = 127 at H 1016, 128 at H 1024
    assert sc_form(8, 4, 16, 1, 1016, 16) == W
    assert sc_form(8, 4, 16, 1, 1024, 16) == MFMA
    for H in (1016, 1024):
        assert [sc_form(8, 4, 16, 1, H, 16, form=f) for f in (1, 2, 3)] == [W, VALU, MFMA]
        # with the pre-conv: a row form always, on the matrix cores unless form 2; the window form is refused
        assert [sc_form(8, 4, 16, 1, H, 16, form=f, pre=True) for f in (0, 2, 3)] == [MFMA | PRE, VALU | PRE, MFMA | PRE]
        assert sc_form(8, 4, 16, 1, H, 16, form=1, pre=True) == ERR_ARG and b"pre-conv needs" in LIB.esm_last_error()
        # the whole conv1 (w2): its tile is flags bits 3-4, as given
        for tile in (0, 1, 2, 3):
            assert sc_form(8, 4, 16, 1, H, 16, form=2, pre=True, w2=True, tile=tile) == CONV1 + tile
        assert sc_form(8, 4, 16, 1, H, 16, form=2, w2=True) == ERR_ARG and b"second conv needs" in LIB.esm_last_error()
        assert sc_form(8, 4, 16, 1, H, 16, form=1, pre=True, w2=True) == ERR_ARG
    for nf, r, C in ((8, 2, 16), (16, 2, 32), (16, 4, 32)):
        assert {sc_form(nf, r, C, 1, 1024, 16, form=f) for f in (0, 1, 2, 3)} == {W}
        assert sc_form(nf, r, C, 1, 1024, 16, pre=True) == ERR_ARG
    for bad in ((8, 4, 32), (16, 4, 16), (12, 2, 16), (8, 3, 16)):
        assert sc_form(*bad, 1, 8, 16) == ERR_UNSUPPORTED, bad
        assert b"(nf, r, C) must be one of (8, 4, 16), (8, 2, 16), (16, 2, 32), (16, 4, 32)" in LIB.esm_last_error()
    d = sc_desc(8, 4, 16, 1, 8, 16)
    d.oh -= 1
    assert LIB.esm_shuffle_conv_form(ctypes.byref(d)) == ERR_ARG and b"output strides" in LIB.esm_last_error()
    assert LIB.esm_shuffle_conv_form(None) == ERR_ARG


def test_engine_labels_are_the_shuffle_queries_answers():
    """``meta["form"]`` of a dry shuffle_tail emission at the two sides of the rule (the label strings of the parent)."""
    p = EN.PackedShuffleTail(*(_shape_only(1) for _ in range(4)), 8, 4)
    labels = []
    for H, form in ((1016, 0), (1024, 0), (1024, 2), (1024, 1)):
        with EN.Ctx("meta", dry=True) as ctx:
            EN.run_shuffle_tail(ctx, _shape_only(1, 8, H, 16), p, form=form)
        labels.append(ctx.meta[-1]["form"])
    assert labels == ["window", "row8", "row4", "window"]


# ----------------------------------------------------------------------------- the fused gwc volume + stem

G, C = 32, 64
STEMS = {"S": (12, 24, 78), "M": (24, 48, 156), "L": (48, 96, 312)}  # D x h x w at 384 x 1248, maxdisp 192


def stem_desc(ext, B=1, cout=8):
    return build_desc(_spec(3, False, 3, 1, 1, (G,), cout, B, ext), 0)


def stem_check(d, L=FAKE, R=FAKE, c=C, g=G):
    return LIB.esm_gwc_stem_check(ctypes.byref(d), L, R, c, g)


@pytest.mark.parametrize("cfg", sorted(STEMS))
def test_gwc_stem_check_takes_the_three_stems(cfg):
    assert stem_check(stem_desc(STEMS[cfg])) == 0, LIB.esm_last_error()
    assert stem_check(stem_desc(STEMS[cfg], B=4)) == 0, LIB.esm_last_error()


VIOLATIONS = [  # (what, edit of the descriptor or the arguments, a word of the message)
    ("null features", lambda d: dict(L=None), b"null"),
    ("null output", lambda d: setattr(d, "out", None), b"null"),
    ("G not a multiple of 4", lambda d: (setattr(d, "Cin", 30), dict(g=30, c=60))[1], b"multiple of 4"),
    ("C != 2 G", lambda d: dict(c=C + 4), b"C = 2 G"),
    ("Cin != G", lambda d: setattr(d, "Cin", 16), b"G -> <= 8"),
    ("more than 8 outputs", lambda d: setattr(d, "Cout", 12), b"G -> <= 8"),
    ("stride 2", lambda d: setattr(d, "stride", 2), b"3x3x3 stride-1 pad-1"),
    ("transposed", lambda d: setattr(d, "transposed", 1), b"3x3x3 stride-1 pad-1"),
    ("pad 0", lambda d: setattr(d, "ph", 0), b"3x3x3 stride-1 pad-1"),
    ("output extent", lambda d: setattr(d, "Ho", d.Ho - 2), b"extent"),
    ("a residual", lambda d: setattr(d, "res", FAKE), b"no mul / res"),
    ("weight padding", lambda d: setattr(d, "cin_pad", 40), b"padding"),
    ("output span", lambda d: setattr(d, "oc", 1 << 28), b"32-bit"),
    ("negative stride", lambda d: setattr(d, "oh", -d.oh), b"32-bit"),
]


@pytest.mark.parametrize("what,edit,word", VIOLATIONS, ids=[v[0] for v in VIOLATIONS])
def test_gwc_stem_check_refuses_one_violation_per_condition(what, edit, word):
    d = stem_desc(STEMS["M"])
    kw = edit(d) or {}
    assert stem_check(d, **kw) == ERR_ARG, what
    assert word in LIB.esm_last_error(), (what, LIB.esm_last_error())
    assert LIB.esm_gwc_stem_check(None, FAKE, FAKE, C, G) == ERR_ARG


def test_gwc_stem_supported_is_the_check_plus_the_size_policy():
    pc = _packed(3, G, 8, 3, 1, 1)
    big, small = _shape_only(1, C, 96, 312), _shape_only(1, C, 24, 78)
    assert EN.gwc_stem_supported(pc, big, G, 48, None)
    assert not EN.gwc_stem_supported(pc, small, G, 12, None)          # under 2^16 voxels: policy
    assert not EN.gwc_stem_supported(pc, big, G, 48, small)            # an attention map: its own launch
    assert not EN.gwc_stem_supported(_packed(3, G, 12, 3, 1, 1), big, G, 48, None)   # the library: <= 8 outputs
    assert not EN.gwc_stem_supported(pc, _shape_only(1, C + 8, 96, 312), G, 48, None)  # the library: C = 2 G
