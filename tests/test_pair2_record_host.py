"""pair2_record_pack (csrc/conv_pair2_rec.h) through its exported hook esm_pair2_record_pack: the 20-dword staging
record of the LDS pair form.  Host only: the hook reads the descriptors' fields and never their pointers.

Checked: every packed field survives the round trip, at its maximum where the pair's own rules allow one; a stride
of 2^31, a fourth source, an extent or a pad past its bits, sources with different strides, a source span past the
out-of-range mark, weights packed otherwise than engine.pack_weight packs them, BN constants that are not behind the
packed weights, and PAIR_NO_RECORD are refused (the launcher then runs the struct-argument kernel); the header and
_lib agree on the new bit; a pair the K-split form takes reports 0."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd._lib import (EsmConvDesc, HINT_PAIR_NO_RECORD, HINT_PAIR_REGRESS, HINT_PAIRK, HINT_ROWS,  # noqa: E402
                                HINT_XCD_SLAB, lib)

FIELDS = ("src0", "wa", "wb", "sb0", "sc", "sh", "Wi", "Hi", "Cin", "pa", "pb", "CoutB", "nsrc", "xcd", "D", "src1",
          "src2", "sb1", "sb2", "C0", "C01", "out", "ob", "oh")
SRC, WA, WB, OUT = 0x7F0000001000, 0x7E0000002000, 0x7E0000802000, 0x7D0000003000  # never dereferenced


def _bn_behind(d: EsmConvDesc, w: int):
    nw = d.kh * d.kw * d.cin_pad * d.cout_pad
    d.w, d.scale, d.shift = w, w + 4 * nw, w + 4 * (nw + d.cout_pad)


def pair(cins=(16,), ka=3, sa=1, pa=1, kb=3, coutb=16, H=7, W=15, B=2, regress=0, hint_a=0, hint_b=0):
    """(a, b) as engine.run_pair2 fills them: contiguous sources, weights and BN constants as pack_conv lays them out."""
    a, b = EsmConvDesc(), EsmConvDesc()
    cin = sum(cins)
    a.nsrc, a.B, a.Cin, a.Cout = len(cins), B, cin, 16
    a.Di, a.Hi, a.Wi = 1, H, W
    a.Do, a.Ho, a.Wo = 1, (H + 2 * pa - ka) // sa + 1, (W + 2 * pa - ka) // sa + 1
    a.kd, a.kh, a.kw, a.stride = 1, ka, ka, sa
    a.pd, a.ph, a.pw = 0, pa, pa
    a.cin_pad, a.cout_pad = -(-cin // 16) * 16, 32
    for i, c in enumerate(cins):
        s = a.src[i]
        s.ptr, s.C = SRC + i * 0x100000, c
        s.sb, s.sc, s.sd, s.sh = c * H * W, H * W, H * W, W
    _bn_behind(a, WA)
    a.act, a.post_scale, a.hint = _lib.ACT_GELU, 1.0, hint_a
    pb = kb // 2
    b.nsrc, b.B, b.Cin, b.Cout = 1, B, 16, coutb
    b.Di, b.Hi, b.Wi = 1, a.Ho, a.Wo
    b.Do, b.Ho, b.Wo = 1, a.Ho + 2 * pb - kb + 1, a.Wo + 2 * pb - kb + 1
    b.kd, b.kh, b.kw, b.stride = 1, kb, kb, 1
    b.pd, b.ph, b.pw = 0, pb, pb
    b.cin_pad, b.cout_pad = 16, 32
    b.src[0].ptr, b.src[0].C = SRC, 16
    _bn_behind(b, WB)
    b.out = OUT
    b.ob, b.oc, b.od, b.oh = coutb * b.Ho * b.Wo, b.Ho * b.Wo, b.Ho * b.Wo, b.Wo
    b.act, b.post_scale, b.hint = _lib.ACT_GELU, 1.0, hint_b
    if regress:  # convA's source is the [B, D, H, W] cost volume, and the regressed map is stored to a.out
        a.src[0].C = regress
        a.src[0].sb = regress * H * W
        a.out = OUT + 0x100000
        a.ob, a.oc, a.od, a.oh = H * W, H * W, H * W, W
        a.hint |= HINT_PAIR_REGRESS
    return a, b


def pack(a: EsmConvDesc, b: EsmConvDesc):
    rec = (ctypes.c_uint32 * 20)()
    fields = (ctypes.c_int64 * 24)()
    rc = lib.esm_pair2_record_pack(ctypes.byref(a), ctypes.byref(b), rec, fields)
    assert rc in (0, 1), lib.esm_last_error()
    return rc, list(rec), dict(zip(FIELDS, fields))


def test_record_of_a_one_source_pair():
    a, b = pair()
    rc, rec, f = pack(a, b)
    assert rc == 1
    assert rec[0] | rec[1] << 32 == SRC and rec[2] | rec[3] << 32 == WA and rec[4] | rec[5] << 32 == WB
    assert f == dict(src0=SRC, wa=WA, wb=WB, sb0=16 * 105, sc=105, sh=15, Wi=15, Hi=7, Cin=16, pa=1, pb=1, CoutB=16,
                     nsrc=1, xcd=0, D=0, src1=SRC, src2=SRC, sb1=16 * 105, sb2=16 * 105, C0=16, C01=16, out=SRC,
                     ob=16 * 105, oh=16 * 105)
    assert rec[19] == 0 and rec[10] >> 20 == 0 and rec[18] >> 16 == 0  # the spare bits stay clear


def test_record_of_three_sources():
    a, b = pair(cins=(16, 12, 20), ka=1, pa=0, coutb=5, hint_a=HINT_XCD_SLAB, hint_b=HINT_ROWS(1))
    a.src[1].sb, a.src[2].sb = 777777, 999999
    rc, _, f = pack(a, b)
    assert rc == 1
    assert (f["nsrc"], f["C0"], f["C01"], f["Cin"], f["CoutB"], f["pa"], f["pb"], f["xcd"]) == (3, 16, 28, 48, 5, 0, 1, 1)
    assert (f["src1"], f["src2"], f["sb1"], f["sb2"]) == (SRC + 0x100000, SRC + 0x200000, 777777, 999999)


def test_record_of_the_regression_source():
    a, b = pair(cins=(1,), ka=5, pa=2, regress=12)
    rc, _, f = pack(a, b)
    assert rc == 1
    assert (f["Cin"], f["D"], f["sc"], f["sh"], f["sb0"]) == (1, 12, 105, 15, 12 * 105)
    assert (f["out"], f["ob"], f["oh"]) == (OUT + 0x100000, 105, 15)
    a.ob = 1 << 31
    assert pack(a, b)[0] == 0


def test_fields_at_their_maximum():
    """Extents of 65535 and a batch stride of 2^31 - 1 on a one-row, one-channel source (so its span stays below the
    out-of-range mark), convA's largest pad, 64 channels on a 1x1."""
    a, b = pair(cins=(1,), ka=5, pa=7, H=1, W=65535)
    a.src[0].sb = (1 << 31) - 1
    rc, _, f = pack(a, b)
    assert rc == 1 and (f["Wi"], f["Hi"], f["pa"], f["sb0"]) == (65535, 1, 7, (1 << 31) - 1)
    a, b = pair(cins=(1,), ka=5, pa=2, H=65535, W=1)
    rc, _, f = pack(a, b)
    assert rc == 1 and (f["Wi"], f["Hi"]) == (1, 65535)
    a, b = pair(cins=(64,), ka=1, pa=0)
    rc, _, f = pack(a, b)
    assert rc == 1 and (f["Cin"], f["C0"], f["C01"]) == (64, 64, 64)
    a, b = pair(cins=(1,), ka=5, pa=2, regress=65535)
    rc, _, f = pack(a, b)
    assert rc == 1 and f["D"] == 65535


@pytest.mark.parametrize("what", ["Wi", "Hi", "pa", "D"])
def test_one_past_the_maximum_is_refused(what):
    a, b = pair(cins=(1,), ka=5, pa=2, H=1 if what == "Wi" else 7, W=1 if what == "Hi" else 15,
                regress=5 if what == "D" else 0)
    assert pack(a, b)[0] == 1
    if what == "Wi":
        a.Wi, a.Wo, b.Wi, b.Wo = 65536, 65536, 65536, 65536
    elif what == "Hi":
        a.Hi, a.Ho, b.Hi, b.Ho = 65536, 65536, 65536, 65536
    elif what == "pa":
        a.ph = a.pw = 8
        a.Ho, a.Wo = a.Hi + 16 - 4, a.Wi + 16 - 4
        b.Hi, b.Wi, b.Ho, b.Wo = a.Ho, a.Wo, a.Ho, a.Wo
    else:
        a.src[0].C = 65536
    assert pack(a, b)[0] == 0


@pytest.mark.parametrize("which", ["sb", "sc", "sh"])
def test_stride_of_2_to_the_31_is_refused(which):
    a, b = pair(cins=(1,), ka=5, pa=2, H=1, W=9)  # one channel, one row: sc and sh are in no offset
    setattr(a.src[0], which, (1 << 31) - 1)
    assert pack(a, b)[0] == 1
    setattr(a.src[0], which, 1 << 31)
    assert pack(a, b)[0] == 0
    setattr(a.src[0], which, -1)
    assert pack(a, b)[0] == 0


def test_fourth_source_is_refused():
    a, b = pair(cins=(16, 16, 16), ka=1, pa=0)
    assert pack(a, b)[0] == 1
    a.nsrc = 4
    assert pack(a, b)[0] == 0


def test_sources_with_different_strides_are_refused():
    a, b = pair(cins=(16, 32))
    assert pack(a, b)[0] == 1
    a.src[1].sh += 2
    assert pack(a, b)[0] == 0
    a, b = pair(cins=(16, 32))
    a.src[1].sc += 2
    assert pack(a, b)[0] == 0
    a, b = pair(cins=(16, 32))
    a.src[1].C = 28  # the sources do not add up to Cin
    assert pack(a, b)[0] == 0


def test_source_span_past_the_out_of_range_mark_is_refused():
    a, b = pair(cins=(16,))
    a.src[0].sc = (1 << 28) // 15  # 15 channel strides + the last plane reach 2^30 bytes
    assert pack(a, b)[0] == 0
    a.src[0].sc = (1 << 28) // 15 - 105
    assert pack(a, b)[0] == 1


def test_other_weight_packings_are_refused():
    for which, field, val in (("a", "cin_pad", 32), ("a", "cout_pad", 16), ("a", "cout_pad", 64), ("b", "cin_pad", 32),
                              ("b", "cout_pad", 16), ("b", "cout_pad", 64)):
        a, b = pair()
        d = a if which == "a" else b
        setattr(d, field, val)
        _bn_behind(d, WA if which == "a" else WB)  # the BN constants still behind the weights: not the reason
        assert pack(a, b)[0] == 0, (which, field, val)
    a, b = pair()
    a.w += 4  # not 16-byte aligned
    a.scale += 4
    a.shift += 4
    assert pack(a, b)[0] == 0


def test_bn_constants_elsewhere_are_refused():
    for which in "ab":
        for field, delta in (("shift", 4), ("scale", 128)):
            a, b = pair()
            d = a if which == "a" else b
            setattr(d, field, getattr(d, field) + delta)
            assert pack(a, b)[0] == 0, (which, field)
        for field in ("scale", "shift"):
            a, b = pair()
            setattr(a if which == "a" else b, field, None)
            assert pack(a, b)[0] == 0, (which, field)


def test_no_record_hint_and_the_ksplit_form_report_zero():
    a, b = pair(hint_b=HINT_PAIR_NO_RECORD)
    assert pack(a, b)[0] == 0
    a, b = pair(hint_b=HINT_PAIRK)  # a 3x3 + 3x3 pair the K-split form takes
    assert pack(a, b)[0] == 0
    a, b = pair(cins=(1,), ka=5, pa=2, regress=5, hint_b=HINT_PAIRK)  # not with the regression source: the LDS form
    assert pack(a, b)[0] == 1


def test_header_and_lib_agree_on_the_bit():
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"^#define ESM_HINT_PAIR_NO_RECORD[ \t]+\(1 << (\d+)\)", src, flags=re.M)
    assert m and 1 << int(m.group(1)) == HINT_PAIR_NO_RECORD
    # convB's hint: the bit is none of the fields the pair reads there
    assert HINT_PAIR_NO_RECORD & (_lib.HINT_ROWS_MASK | HINT_PAIRK | HINT_XCD_SLAB) == 0
