"""The host guards of the 32-bit addressed conv forms, on the CPU (nothing launched; DESIGN.md "Addressing limits").

Most conv forms address their operands with 32-bit byte offsets through buffer descriptors, out-of-range lanes
marked ``kOOB = 2^30`` (csrc/conv_direct.h): sound while an operand's span per batch item stays below 1 GiB.  For
every row of esmstereo_amd/tuned_hints.json this builds the contiguous descriptor of tests/test_conv_forms_host.py
(fake addresses) and then moves ONE operand -- source 0, the last source, ``out`` (with ``out2``), ``res``, ``mul`` --
to strides at and beyond the limit:

  near    the channel stride (the plane stride of a one-channel 3-D operand, the row stride of a one-channel 2-D
          one) that puts ``4 * last`` in [kOOB - 4096, kOOB), ``last`` = the item's last element + 1;
  over    the stride that puts it in [kOOB, kOOB + 4096);
  stride  that axis 2^28 + 4 elements apart.

With hint 0 ``esm_conv_form`` must keep the contiguous descriptor's form at ``near`` and must never report a form the
table lists as 32-bit for the moved operand at ``over`` / ``stride``.  The automatic single-output-channel
ConvTranspose path reports GENERAL either way, so its guard is asked directly (``esm_convt_c1_ok``).  Descriptors
no form can address (an offset of 2^31 elements or more within one channel) are refused by ``conv_check``.
"""
import ctypes

import pytest
import torch  # noqa: F401  (before the native library, as in every test module: this file is collected first)

from esmstereo_amd import _lib
from test_conv_forms_host import TABLE, build_desc
from tuned_rows import parse_key

KOOB = 0x40000000
PLACES = ("near", "over", "stride")
OPERANDS = ("src0", "srcN", "out", "res", "mul")
G, STEM, C1IN, SMALL, WIDE, WIDE3, WIDET, TILE3, TILE2, PW = range(10)
assert (G, PW) == (_lib.FORM_GENERAL, _lib.FORM_PW)
# DESIGN.md "Addressing limits": the forms whose kernels address the operand through 32-bit offsets and whose guard
# (direct_ok / pw_ok) therefore hands an over-limit layer to another form.  An output over the limit stays in its
# form (the 64-bit epilogue variant of the same kernel) except in the pointwise form; res and mul are 64-bit everywhere.
BITS32 = {
    "src0": {STEM, SMALL, WIDE, WIDE3, WIDET, TILE3, TILE2, PW},
    "srcN": {STEM, SMALL, WIDE, WIDE3, WIDET, TILE3, TILE2, PW},
    "out": {PW},
    "res": set(),
    "mul": set(),
}


def _rup4(n):
    return (n + 3) // 4 * 4


def far_stride(place, n, inner):
    """The stride of an axis of ``n`` entries of ``inner`` packed elements each for ``place`` (None: the entries
    themselves are too large for it).  Shared with tests/test_gpu_addressing_limits.py."""
    lim = KOOB // 4
    if place == "stride":
        s = (1 << 28) + 4
    elif place == "near":
        s = (lim - 1 - inner) // (n - 1)
        if n <= 256:  # 16-byte aligned where that stays within the window (up to 4 (n - 1) elements short)
            s = s // 4 * 4
    else:
        s = -(-(lim - inner) // (n - 1))
        s = max(_rup4(s) if n <= 256 else s, _rup4(inner))
    if s < inner:
        return None
    last = (n - 1) * s + inner
    if place == "near":
        assert lim - 1024 <= last < lim
    elif place == "over" and s > _rup4(inner):
        assert lim <= last < lim + 1024
    return s


def _move(d, nd, which, place):
    """Set the strides of one operand of the contiguous descriptor ``d``; False if the placement does not exist."""
    def axis(C, ext):  # -> (name, n, inner elements of one entry)
        D, H, W = ext
        if C > 1:
            return "c", C, D * H * W
        if nd == 3 and D > 1:
            return "d", D, H * W
        return "h", H, W

    def strides(C, ext):
        name, n, inner = axis(C, ext)
        if n < 2:
            return None
        s = far_stride(place, n, inner)
        if s is None:
            return None
        D, H, W = ext
        sh, sd, sc = W, H * W, D * H * W
        if name == "h":
            sh, sd, sc = s, s * H, s * H * D
        elif name == "d":
            sd, sc = s, s * D
        else:
            sc = s
        return sc * C, sc, sd, sh

    r = d.shuffle if d.shuffle > 1 else 1
    oext = (d.Do, d.Ho * r, d.Wo * r)
    ocs = d.Cout // (r * r)
    if which in ("src0", "srcN"):
        s = d.src[0 if which == "src0" else d.nsrc - 1]
        st = strides(s.C, (d.Di, d.Hi, d.Wi))
        if st is None:
            return False
        s.sb, s.sc, s.sd, s.sh = st[0], st[1], (st[2] if nd == 3 else 0), st[3]
    elif which == "out":
        st = strides(ocs, oext)
        if st is None:
            return False
        d.ob, d.oc, d.od, d.oh = st[0], st[1], (st[2] if nd == 3 else 0), st[3]
    elif which == "res":
        st = strides(ocs, oext)
        if not d.res or st is None:
            return False
        d.rb, d.rc, d.rd, d.rh = st[0], st[1], (st[2] if nd == 3 else 0), st[3]
    else:
        st = strides(d.Cout, (1, d.Ho, d.Wo))
        if not d.mul or st is None:
            return False
        d.mb, d.mc, d.mh = st[0], st[1], st[3]
    return True


def _plane_reach(d, which):
    """The moved operand's last offset within one channel, + 1."""
    r = d.shuffle if d.shuffle > 1 else 1
    if which.startswith("src"):
        s = d.src[0 if which == "src0" else d.nsrc - 1]
        return (d.Di - 1) * s.sd + (d.Hi - 1) * s.sh + d.Wi
    if which == "mul":
        return (d.Ho - 1) * d.mh + d.Wo
    sd, sh = (d.od, d.oh) if which == "out" else (d.rd, d.rh)
    return (d.Do - 1) * sd + (d.Ho * r - 1) * sh + d.Wo * r


def _form(d):
    rc = _lib.lib.esm_conv_form(ctypes.byref(d))
    assert rc >= 0, _lib.lib.esm_last_error()
    return rc


@pytest.mark.parametrize("key", sorted(TABLE))
def test_automatic_rules_leave_the_32bit_forms_past_the_limit(key):
    spec = parse_key(key)
    plain = _form(build_desc(spec, 0))
    moved = 0
    for which in OPERANDS:
        if which == "srcN" and len(spec.cins) == 1:
            continue
        for place in PLACES:
            d = build_desc(spec, 0)
            if not _move(d, spec.nd, which, place):
                continue
            moved += 1
            if _plane_reach(d, which) >= 1 << 31:
                # (rows or planes 2^28 + 4 apart, more than 8 of them: beyond every form, refused by conv_check)
                assert place == "stride" and _lib.lib.esm_conv_form(ctypes.byref(d)) == -1, (key, which, place)
                assert b"2^31 elements" in _lib.lib.esm_last_error()
                continue
            form = _form(d)
            what = (key, which, place, form)
            if place == "near":
                # (a channel stride that is no multiple of 4 -- rows of more than 256 channels, far_stride -- does
                # not suit the pointwise form: it steps aside for the LDS-tiled 1x1 form as on any such layout)
                assert form == plain or (plain == PW and form in (TILE2, TILE3)), what
                continue
            assert form not in BITS32[which], what
            if form == G and spec.transposed and spec.cout == 1 and which.startswith("src"):
                # reported as GENERAL with either kernel: the VALU ConvTranspose form's own guard
                assert _lib.lib.esm_convt_c1_ok(ctypes.byref(d)) == 0, what
    assert moved, key


def test_convt_c1_guard_query():
    """esm_convt_c1_ok: 1 for every contiguous single-output-channel ConvTranspose row of the table and at ``near``,
    0 past the limit, 0 for layers of another shape, a negative status for a refused descriptor."""
    rows = [k for k in sorted(TABLE) if parse_key(k).transposed and parse_key(k).cout == 1]
    assert rows
    ok = _lib.lib.esm_convt_c1_ok
    for key in rows:
        spec = parse_key(key)
        d = build_desc(spec, 0)
        want = int(len(spec.cins) == 1 and spec.cin <= 32)
        assert ok(ctypes.byref(d)) == want, key
        for place, res in (("near", want), ("over", 0), ("stride", 0)):
            d = build_desc(spec, _lib.HINT_C1T)
            assert _move(d, spec.nd, "src0", place) and _plane_reach(d, "src0") < 1 << 31
            assert ok(ctypes.byref(d)) == res, (key, place)
            assert _form(d) == G  # the forced form is reported as forced; its launcher refuses
    other = next(k for k in sorted(TABLE) if not parse_key(k).transposed)
    d = build_desc(parse_key(other), 0)
    assert ok(ctypes.byref(d)) == 0
    d.cin_pad = 8
    assert ok(ctypes.byref(d)) == -1 and b"cin_pad" in _lib.lib.esm_last_error()
    assert ok(None) == -1


def _small_desc(nd, epi=""):
    from tuned_rows import Spec
    ext = (5, 7, 21) if nd == 3 else (9, 37)
    spec = Spec(nd=nd, transposed=False, k=3, s=1, p=1, cins=(12,), cout=1 if "u" in epi else 12, B=2,
                Di=ext[0] if nd == 3 else 1, Hi=ext[-2], Wi=ext[-1], shuffle=1, u="u" in epi, m="m" in epi,
                r="r" in epi, two=False)
    return build_desc(spec, 0)


PLANE_CASES = [  # (dims, epilogue operands, the stride field pushed to 2^31 elements per plane)
    (2, "", "src.sh"), (3, "", "src.sd"), (3, "", "src.sh"), (2, "", "oh"), (3, "", "od"), (3, "", "oh"),
    (2, "r", "rh"), (3, "r", "rd"), (2, "m", "mh"), (2, "u", "uh"),
]


@pytest.mark.parametrize("nd,epi,name", PLANE_CASES, ids=[f"{n}d-{f}" for n, _, f in PLANE_CASES])
def test_conv_check_refuses_planes_of_2_31_elements(nd, epi, name):
    """An offset of 2^31 elements or more within one channel of any operand: refused with a message, for every hint (the LDS-staged general form narrows a source's offset to int; no form
    remains).  One element less is accepted."""
    def setf(d, v):
        if name.startswith("src."):
            setattr(d.src[0], name[4:], v)
        else:
            setattr(d, name, v)

    def terms(d):  # (entries along the field's axis, the other terms of the channel's last offset + 1)
        return {"src.sh": (d.Hi, (d.Di - 1) * d.src[0].sd + d.Wi), "src.sd": (d.Di, (d.Hi - 1) * d.src[0].sh + d.Wi),
                "oh": (d.Ho, (d.Do - 1) * d.od + d.Wo), "od": (d.Do, (d.Ho - 1) * d.oh + d.Wo),
                "rh": (d.Ho, (d.Do - 1) * d.rd + d.Wo), "rd": (d.Do, (d.Ho - 1) * d.rh + d.Wo),
                "mh": (d.Ho, d.Wo), "uh": (d.up_h, d.up_w)}[name]

    for hint in (0, 0x11, _lib.HINT_SMALL):
        d = _small_desc(nd, epi)
        d.hint = hint
        n, other = terms(d)
        s_ok = ((1 << 31) - 1 - other) // (n - 1)
        setf(d, s_ok)
        assert _lib.lib.esm_conv_form(ctypes.byref(d)) >= 0, (name, hint, _lib.lib.esm_last_error())
        setf(d, s_ok + 1)
        assert (n - 1) * (s_ok + 1) + other >= 1 << 31
        assert _lib.lib.esm_conv_form(ctypes.byref(d)) == -1, (name, hint)
        assert b"2^31 elements" in _lib.lib.esm_last_error()


def test_conv_check_refuses_packed_weights_of_1_gib():
    """The packed weights [taps][cin_pad][cout_pad] are read through 32-bit byte offsets with marks at 1 GiB: a slab
    that large is refused with its own message; the largest one below it is accepted."""
    for nd, taps in ((3, 27), (2, 9)):
        d = _small_desc(nd)
        d.cout_pad = 4096
        d.cin_pad = ((1 << 28) // (taps * 4096) + 15) // 16 * 16          # the first multiple of 16 at or past 1 GiB
        assert taps * d.cin_pad * d.cout_pad * 4 >= 1 << 30
        assert _lib.lib.esm_conv_form(ctypes.byref(d)) == -1 and b"packed weights" in _lib.lib.esm_last_error()
        d.cin_pad -= 16
        assert taps * d.cin_pad * d.cout_pad * 4 < 1 << 30
        assert _lib.lib.esm_conv_form(ctypes.byref(d)) >= 0, _lib.lib.esm_last_error()
