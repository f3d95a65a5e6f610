"""The kernel form of every launch the tuned-hint table names, pinned on the CPU (no GPU).

``esm_conv_form`` applies the validation and the rules of ``esm_conv_f32`` and launches nothing, nor does it read
through the descriptor's pointers.  For every row of esmstereo_amd/tuned_hints.json this builds the ``esm_conv_desc``
the key describes, filled as ``engine._conv_desc`` fills it for a BasicConv (folded BN + GELU) over contiguous
tensors, and asks for the form with the row's hint, with hint 0 (the automatic rules) and with XCD_SLAB alone (the
tile order selects no form).  All three must equal tests/golden/conv_forms.json.

The addresses are fake: back to back and 256-byte aligned from ``ARENA_BASE`` in the engine's order (sources,
weights, scale, shift, output, mul, res, up, out2), the way a plan's arena carves its buffers, so that the rules
that look at addresses (alignment, sources within one buffer window) see what a plan shows them.  The window
starts below 1 GiB; the B = 32 volumes are larger than that and simply run on.

``python tests/test_conv_forms_host.py --record`` rewrites the fixture from the library in use (``ESM_LIB`` names
another build).  The committed fixture was recorded from the build before the hint word's fields were named, so
the test holds every later change of ``select_form`` to "same form for every launch the project ships".
"""
import ctypes
import json
import os
import sys

import pytest

if __name__ == "__main__":  # (under pytest, tests/conftest.py has done this)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from esmstereo_amd import _lib  # noqa: E402
from tuned_rows import Spec, load_table, parse_key  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_forms.json")
TABLE = load_table()
ARENA_BASE = 1 << 28
WAYS = ("tuned", "auto", "xcd_slab")


def _rup(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def build_desc(spec: Spec, hint: int, act: int = _lib.ACT_GELU, scale: bool = True, shift: bool = True,
               post_scale: float = 1.0):
    """The descriptor of ``spec`` over fake addresses.  ``act``, ``scale`` / ``shift`` (False: a NULL pointer) and
    ``post_scale``: the descriptor fields a shape key does not name (tests/conv_domain.py)."""
    d = _lib.EsmConvDesc()
    nd, k = spec.nd, spec.k
    cursor = ARENA_BASE

    def carve(*shape: int) -> int:
        nonlocal cursor
        n = 4
        for v in shape:
            n *= v
        addr, cursor = cursor, cursor + _rup(n, 256)
        return addr

    def strides(*shape: int):
        st = [1]
        for v in reversed(shape[1:]):
            st.insert(0, st[0] * v)
        return st

    Di, Hi, Wi = spec.Di, spec.Hi, spec.Wi
    ext = spec.out_ext
    Do, Ho, Wo = (ext if nd == 3 else (1,) + ext)
    for i, c in enumerate(spec.cins):
        shape = (spec.B, c) + spec.in_ext
        st = strides(*shape)
        d.src[i].ptr, d.src[i].C = carve(*shape), c
        d.src[i].sb, d.src[i].sc = st[0], st[1]
        d.src[i].sd = st[2] if nd == 3 else 0
        d.src[i].sh = st[-2]
    d.nsrc = len(spec.cins)
    d.B, d.Cin = spec.B, spec.cin
    d.Di, d.Hi, d.Wi = Di, Hi, Wi
    d.Do, d.Ho, d.Wo = Do, Ho, Wo
    d.kd = k if nd == 3 else 1
    d.kh = d.kw = k
    d.stride, d.transposed = spec.s, int(spec.transposed)
    d.pd = spec.p if nd == 3 else 0
    d.ph = d.pw = spec.p
    d.Cout, d.cin_pad, d.cout_pad = spec.cout, _rup(spec.cin, 16), _rup(spec.cout, 32)  # engine.pack_weight
    taps = (2 ** nd) ** 2 if spec.transposed else k ** nd  # transposed: parity classes x taps per class
    d.w = carve(taps, d.cin_pad, d.cout_pad)
    d.scale, d.shift = carve(spec.cout), carve(spec.cout)  # (carved whether used or not: the addresses behind stay)
    if not scale:
        d.scale = None
    if not shift:
        d.shift = None
    d.act = act
    r = spec.shuffle
    d.shuffle = r
    oshape = (spec.B, spec.cout // (r * r), Ho * r, Wo * r) if r > 1 else (spec.B, spec.cout) + ext
    ost = strides(*oshape)
    d.out = carve(*oshape)
    d.ob, d.oc = ost[0], ost[1]
    d.od = ost[2] if nd == 3 else 0
    d.oh = ost[-2]
    if spec.m:  # [B, Cout, Ho, Wo], broadcast over D
        st = strides(spec.B, spec.cout, Ho, Wo)
        d.mul = carve(spec.B, spec.cout, Ho, Wo)
        d.mb, d.mc, d.mh = st[0], st[1], st[2]
    if spec.r:
        d.res = carve(*oshape)
        d.rb, d.rc = ost[0], ost[1]
        d.rd = ost[2] if nd == 3 else 0
        d.rh = ost[-2]
    if spec.u:  # the refinement heads' `+ bilinear(previous disparity, 2)`
        d.up = carve(spec.B, 1, Ho // 2, Wo // 2)
        d.up_h, d.up_w, d.up_f = Ho // 2, Wo // 2, 2
        d.ub, d.uh = (Ho // 2) * (Wo // 2), Wo // 2
    d.post_scale = post_scale
    if spec.two:
        d.out2 = carve(*oshape)
        d.post_scale2 = 0.5
    d.hint = hint
    return d


def forms(key: str):
    """[form with the row's hint, with hint 0, with XCD_SLAB alone]; a negative value is the library's refusal."""
    spec = parse_key(key)
    out = []
    for hint in (TABLE[key], 0, _lib.HINT_XCD_SLAB):
        d = build_desc(spec, hint)
        rc = _lib.lib.esm_conv_form(ctypes.byref(d))
        assert rc >= 0, (key, hex(hint), rc, _lib.lib.esm_last_error())  # a refusal: the builder is wrong
        out.append(rc)
    return out


def test_fixture_has_every_row():
    with open(FIXTURE) as f:
        fx = json.load(f)["forms"]
    assert sorted(fx) == sorted(TABLE)
    assert all(sorted(v) == sorted(WAYS) and all(0 <= x <= _lib.FORM_PW for x in v.values()) for v in fx.values())


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)["forms"]


@pytest.mark.parametrize("key", sorted(TABLE))
def test_row_takes_the_recorded_form(key, fixture):
    assert dict(zip(WAYS, forms(key))) == fixture[key]


def record() -> None:
    fx = {key: dict(zip(WAYS, forms(key))) for key in sorted(TABLE)}
    with open(FIXTURE, "w") as f:
        json.dump({"forms": fx}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(fx)} rows from {_lib.LIB_PATH}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_conv_forms_host.py --record")
    record()
