"""lean_record_pack (csrc/conv_lean_rec.h) through its exported hook esm_lean_record_pack: the 14-dword first-load
record of the lean conv form.  Host only: the hook reads the descriptor's fields and never its pointers.

Checked: every packed field survives the round trip at its maximum; one past the maximum of each field, a stride
of 2^31, a second source, BN constants that are not behind the packed weights, and SMALL_NO_RECORD are refused (the
launcher then runs the struct-argument kernel); a cropped strided view keeps its own plane stride."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd._lib import EsmConvDesc, HINT_SMALL, HINT_SMALL_NO_RECORD, HINT_XCD_SLAB, lib  # noqa: E402

FIELDS = ("sb", "sc", "sd", "sh", "m_ds", "m_b", "Wi", "Hi", "Di", "Ws", "Ds", "B", "Cin", "cout_pad", "pd", "ph",
          "pw", "xcd", "scale")
SRC, W = 0x7F0000001000, 0x7E0000002000  # never dereferenced


def magic(d: int) -> int:
    return 0 if d <= 1 else ((1 << 32) + d - 1) // d


def desc(nd=3, k=3, stride=1, pad=1, cin=8, cout=8, ext=(4, 6, 18), B=2, transposed=False, strides=None,
         scale=True, hint=HINT_SMALL) -> EsmConvDesc:
    d = EsmConvDesc()
    Di, Hi, Wi = ext if nd == 3 else (1,) + tuple(ext[-2:])
    d.nsrc, d.B, d.Cin, d.Cout = 1, B, cin, cout
    d.Di, d.Hi, d.Wi = Di, Hi, Wi
    if transposed:
        d.Do, d.Ho, d.Wo = (2 * Di if nd == 3 else 1), 2 * Hi, 2 * Wi
    else:
        o = lambda n: (n + 2 * pad - k) // stride + 1  # noqa: E731
        d.Do, d.Ho, d.Wo = (o(Di) if nd == 3 else 1), o(Hi), o(Wi)
    d.kd, d.kh, d.kw = (k if nd == 3 else 1), k, k
    d.stride, d.transposed = stride, int(transposed)
    d.pd, d.ph, d.pw = (pad if nd == 3 else 0), pad, pad
    d.cin_pad, d.cout_pad = -(-cin // 16) * 16, -(-cout // 32) * 32
    sh, sd, sc = Wi, Hi * Wi, Di * Hi * Wi
    sb = cin * sc
    if strides:
        sb, sc, sd, sh = strides
    d.src[0].ptr, d.src[0].C = SRC, cin
    d.src[0].sb, d.src[0].sc, d.src[0].sd, d.src[0].sh = sb, sc, sd, sh
    nw = d.kd * k * k * d.cin_pad * d.cout_pad
    d.w = W
    d.scale = W + 4 * nw if scale else None
    d.shift = W + 4 * (nw + d.cout_pad)
    d.out = 0x7D0000003000
    d.ob, d.oc, d.od, d.oh = cout * d.Do * d.Ho * d.Wo, d.Do * d.Ho * d.Wo, d.Ho * d.Wo, d.Wo
    d.act, d.post_scale, d.hint = _lib.ACT_GELU, 1.0, hint
    return d


def pack(d: EsmConvDesc):
    rec = (ctypes.c_uint32 * 14)()
    fields = (ctypes.c_int64 * 19)()
    rc = lib.esm_lean_record_pack(ctypes.byref(d), rec, fields)
    assert rc in (0, 1), _lib.lib.esm_last_error()
    return rc, list(rec), dict(zip(FIELDS, fields))


def test_record_of_a_plain_layer():
    d = desc()
    rc, rec, f = pack(d)
    assert rc == 1
    assert rec[0] | rec[1] << 32 == SRC and rec[2] | rec[3] << 32 == W
    assert f == dict(sb=8 * 432, sc=432, sd=108, sh=18, m_ds=magic(4), m_b=magic(2), Wi=18, Hi=6, Di=4, Ws=18, Ds=4, B=2,
                     Cin=8, cout_pad=32, pd=1, ph=1, pw=1, xcd=0, scale=1)


def test_sub_grid_of_strided_and_transposed_layers():
    _, _, f = pack(desc(stride=2, ext=(4, 6, 18)))
    assert (f["Ws"], f["Ds"], f["m_ds"]) == (9, 2, magic(2))
    _, _, f = pack(desc(k=4, stride=2, transposed=True, ext=(1, 3, 10), cin=16, cout=12))
    assert (f["Ws"], f["Ds"], f["m_ds"]) == (10, 1, 0)  # the input grid; a one-plane volume needs no division
    _, _, f = pack(desc(nd=2, ext=(5, 19), cin=16, cout=16))
    assert (f["Di"], f["Ds"], f["pd"], f["Wi"], f["Hi"]) == (1, 1, 0, 19, 5)


def test_every_field_at_its_maximum():
    big = (1 << 31) - 1
    d = desc(nd=3, k=3, pad=1, cin=1023, cout=480, ext=(65535, 65535, 65535), B=65535, strides=(big, big, big, big),
             hint=HINT_SMALL | HINT_XCD_SLAB)
    d.pd = d.ph = d.pw = 7  # (the hook packs the fields; whether a launcher takes the geometry is its own check)
    rc, rec, f = pack(d)
    assert rc == 1
    assert f == dict(sb=big, sc=big, sd=big, sh=big, m_ds=magic(65535), m_b=magic(65535), Wi=65535, Hi=65535, Di=65535,
                     Ws=65535, Ds=65535, B=65535, Cin=1023, cout_pad=480, pd=7, ph=7, pw=7, xcd=1, scale=1)
    assert rec[13] >> 25 == 0  # the spare bits stay clear


@pytest.mark.parametrize("what", ["Wi", "Hi", "Di", "Wo", "Do", "B", "Cin", "cout_pad", "pd", "ph", "pw"])
def test_one_past_the_maximum_is_refused(what):
    d = desc()
    assert pack(d)[0] == 1
    if what == "Cin":
        d.Cin = d.src[0].C = 1024
        d.cin_pad = 1024
    elif what == "cout_pad":
        d.cout_pad = 512
    elif what in ("pd", "ph", "pw"):
        setattr(d, what, 8)
    else:  # Wo / Do are the sub-grid Ws / Ds of a plain conv
        setattr(d, what, 65536)
    nw = d.kd * d.kh * d.kw * d.cin_pad * d.cout_pad  # keep the BN constants behind the weights: not the reason
    d.scale, d.shift = W + 4 * nw, W + 4 * (nw + d.cout_pad)
    assert pack(d)[0] == 0


@pytest.mark.parametrize("which", ["sb", "sc", "sd", "sh"])
def test_stride_of_2_to_the_31_is_refused(which):
    d = desc()
    setattr(d.src[0], which, (1 << 31) - 1)
    assert pack(d)[0] == 1
    setattr(d.src[0], which, 1 << 31)
    assert pack(d)[0] == 0
    setattr(d.src[0], which, -1)
    assert pack(d)[0] == 0


def test_second_source_is_refused():
    d = desc(cin=16)
    d.nsrc = 2
    d.src[0].C = d.src[1].C = 8
    d.src[1].ptr = SRC + 4096
    d.src[1].sb, d.src[1].sc, d.src[1].sd, d.src[1].sh = d.src[0].sb, d.src[0].sc, d.src[0].sd, d.src[0].sh
    assert pack(d)[0] == 0


def test_bn_constants_elsewhere_are_refused():
    d = desc()
    d.shift += 4
    assert pack(d)[0] == 0
    d = desc()
    d.scale += 128
    assert pack(d)[0] == 0
    d = desc()
    d.shift = None
    assert pack(d)[0] == 0
    rc, _, f = pack(desc(scale=False))  # bias only: shift in its slot, no scale
    assert rc == 1 and f["scale"] == 0


def test_no_record_hint_is_refused():
    assert pack(desc(hint=HINT_SMALL | HINT_SMALL_NO_RECORD))[0] == 0


def test_cropped_strided_view_keeps_its_strides():
    """A 2 x 3 x 10 crop out of a 5 x 7 x 13 parent: plane stride 91 != Hi * Wi = 30."""
    d = desc(cin=12, cout=12, ext=(2, 3, 10), strides=(12 * 455, 455, 91, 13))
    rc, _, f = pack(d)
    assert rc == 1
    assert (f["sb"], f["sc"], f["sd"], f["sh"]) == (12 * 455, 455, 91, 13)
    assert (f["Di"], f["Hi"], f["Wi"]) == (2, 3, 10)
