"""The descriptor domain of ``esm_conv_f32`` as test input: a case generator and the acceptance table.

``conv_check`` accepts any padding, any extent down to one pixel, any channel count, six activations and every
combination of epilogue operands; each kernel form decides in its own ``*_ok`` predicate what it runs.  This module
restates, in plain Python and from the documentation (the comment above ``esm_conv_desc``, DESIGN 4 / 5 and the comment
above each predicate), what each form runs (``ACCEPTS``), what a forced hint gets where it does not (``REFUSAL``,
the table of DESIGN 5 "Addressing limits"), and which geometry any form instantiates (``SUPPORTED_GEOMETRY``).  The
generator walks one axis at a time around a small base case per (form, geometry), plus seeded random combinations.

``tests/test_conv_domain_host.py`` holds the library's selection (``esm_conv_form``) and the coverage conditions
to these tables on the CPU; ``tests/test_gpu_conv_domain.py`` launches every case.  Nothing here needs a GPU.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from esmstereo_amd import _lib
from esmstereo_amd._lib import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SIGMOID, ACT_SILU, HINT_C1IN, HINT_C1T,
                                HINT_SMALL, HINT_SMALL_NO_RECORD, HINT_SMALL_NO_ZSPLIT, HINT_SMALL_W8, HINT_STEM, HINT_TILE,
                                HINT_TILE_DMA_FLIP, HINT_TILE_PW, HINT_TILE_WLDS, HINT_WIDE, HINT_WIDE3, HINT_WIDE_KS2,
                                HINT_WIDET)
from esmstereo_amd._lib import HINT_ROWS as ROWS
from tuned_rows import Spec, format_key

ACTS = (ACT_NONE, ACT_GELU, ACT_SILU, ACT_RELU, ACT_SIGMOID, ACT_RELU6)
ACT_GAIN = 15.0  # the activation cases' BN gain: pre-activations (sigma about 0.6, a few thousand values) span about +-30


@dataclass(frozen=True)
class Case:
    """One launch: the shape key's ``Spec`` and the descriptor fields a key does not name."""

    spec: Spec
    form: str                # the form under test (a key of ACCEPTS); its hint is forced
    hint: int
    act: int = ACT_GELU
    bn: str = "bn"           # "bn": scale and shift; "bias": shift alone (scale NULL); "none": both NULL
    post: float = 1.0        # post_scale
    gain: float = 1.0        # the BN gain's factor (the activation axis)
    axis: str = "base"       # the axis this case varies, and its value there (coverage bookkeeping)
    value: str = ""
    base: str = ""           # name of the (form, geometry) base the case belongs to

    @property
    def id(self) -> str:
        return (f"{self.form} {format_key(self.spec)} a{self.act} {self.bn} ps{self.post:g} g{self.gain:g} "
                f"h{self.hint:#x} [{self.axis}={self.value}]")

    @property
    def launch(self) -> Spec:
        """The spec as the library sees it (common.h is3d: a cubic kernel or more than one plane on either side): a
        1x1x1 p0 conv over a one-plane volume IS a 2-D launch, whatever the tensors' rank."""
        s = self.spec
        flat = s.nd == 3 and not s.transposed and (s.k, s.p, s.Di) == (1, 0, 1)
        return replace(s, nd=2) if flat else s

    @property
    def seed(self) -> int:
        return zlib.crc32(self.id.encode()) & 0x7FFFFFFF


# ----------------------------------------------------------------------------- what each form runs


def SUPPORTED_GEOMETRY(c: Case) -> bool:
    """The (kernel, stride) pairs some form instantiates (launch_conv2d / launch_conv3d; the comment above
    esm_conv_desc): every other pair ends in ESM_ERR_UNSUPPORTED."""
    s = c.launch
    if s.transposed:
        return (s.k, s.s, s.p) == (4, 2, 1)
    return (s.k, s.s) in ({(1, 1), (3, 1), (3, 2), (5, 1)} if s.nd == 2 else {(1, 1), (3, 1), (3, 2)})


def _aligned_splits(s: Spec) -> bool:
    """direct_ok at these sizes: every split of a multi-source input on a 4-channel boundary."""
    return len(s.cins) == 1 or all(v % 4 == 0 for v in s.cins)


def _ng(s: Spec) -> int:
    return (s.cin + 3) // 4


def _mt(s: Spec) -> int:
    return 2 if s.cout > 16 else 1


def _general(c: Case) -> bool:  # LDS-staged: the last resort, every epilogue, any split
    return SUPPORTED_GEOMETRY(c)


def _direct(c: Case) -> bool:  # register operands: 4-channel aligned splits (conv_direct.h direct_ok)
    return SUPPORTED_GEOMETRY(c) and _aligned_splits(c.spec)


def _rows(c: Case) -> bool:  # conv_rows.h: one source, stride 1, <= 16 input channels, the weight slab within 64 KiB
    s = c.launch
    taps = s.k ** s.nd
    return (SUPPORTED_GEOMETRY(c) and not s.transposed and s.s == 1 and len(s.cins) == 1 and s.cin <= 16 and
            4 * taps * 16 * (16 if s.cout <= 16 else 48) <= 64 * 1024)


def _c1t(c: Case) -> bool:  # conv_c1.h: ConvTranspose to one output channel, one source, <= 32 input channels
    s = c.launch
    return s.transposed and s.cout == 1 and len(s.cins) == 1 and s.cin <= 32


def _stem(c: Case) -> bool:  # conv_stem.hip: 3x3(x3) s1 "same" padding, one source, 8 / 12 / 16 / 24 / 32 couts, slab in LDS
    s = c.launch
    if s.transposed or (s.k, s.s, s.p) != (3, 1, 1) or len(s.cins) != 1 or s.shuffle > 1:
        return False
    if s.cout not in (8, 12, 16, 24, 32):
        return False
    cgp = 4 if s.cout == 12 else s.cout // 4
    return _ng(s) * 4 * (27 if s.nd == 3 else 9) * 4 * cgp * 4 <= 64 * 1024


def _c1in(c: Case) -> bool:  # conv_stem.hip: one input channel, 2-D, k3 s1 / s2 or k5 s1, <= 32 couts, plain store
    s = c.launch
    return (s.nd == 2 and not s.transposed and s.cins == (1,) and s.cout <= 32 and s.shuffle <= 1 and
            not (s.m or s.r or s.u or s.two) and (s.k, s.s) in {(3, 1), (3, 2), (5, 1)})


def _small(c: Case) -> bool:  # conv_small.hip: no mul / up / shuffle, aligned splits, the kernel shapes it instantiates
    s = c.launch
    if s.m or s.u or s.shuffle > 1 or not _aligned_splits(s):
        return False
    if s.transposed:
        return True
    return (s.k, s.s) in ({(1, 1), (3, 1), (3, 2), (5, 1)} if s.nd == 2 else {(1, 1), (3, 1), (3, 2)})


def _wide(c: Case) -> bool:  # conv_wide.hip: 2-D stride 1, <= 32 couts, weights within the register budget
    s = c.launch
    if s.nd != 2 or s.transposed or s.s != 1 or s.m or s.u or s.shuffle > 1 or s.cout > 32 or not _aligned_splits(s):
        return False
    ng, mt = _ng(s), _mt(s)
    if s.k == 5:
        return ng <= 2 and mt == 1
    if s.k == 3:
        return ng * mt <= 10 and (mt == 1 or ng <= 4)
    return s.k == 1 and ng * mt <= 32


def _wide3(c: Case) -> bool:  # conv_wide3.hip: 3x3x3 s1 p1, one source, <= 16 couts, <= 32 input channels
    s = c.launch
    return (s.nd == 3 and not s.transposed and (s.k, s.s, s.p) == (3, 1, 1) and len(s.cins) == 1 and s.cout <= 16 and
            s.cin <= 32 and not s.u)


def _widet(c: Case) -> bool:  # conv_widet.hip: ConvTranspose2d, one source, <= 32 couts, 16 * groups * tiles <= 64
    s = c.launch
    return (s.nd == 2 and s.transposed and len(s.cins) == 1 and not (s.m or s.u) and s.shuffle <= 1 and s.cout <= 32 and
            _ng(s) * _mt(s) <= 4)


def _tile2(c: Case) -> bool:  # conv_tile3.hip, 2-D: k3 s1 / s2 or k1 s1, any padding, 1..3 sources, <= 96 couts
    s = c.launch
    if s.nd != 2 or s.u or s.shuffle > 1 or s.cout > 96 or not _aligned_splits(s):
        return False
    if s.transposed:
        return len(s.cins) == 1 and not s.m and s.cout > 1
    return (s.k, s.s) in {(3, 1), (3, 2), (1, 1)}


def _tile3(c: Case) -> bool:  # conv_tile3.hip, 3-D: k3 s1 / s2 p1 over one source, k1 p0 over 1..3, <= 96 couts
    s = c.launch
    if s.nd != 3 or s.u or s.cout > 96 or not _aligned_splits(s):
        return False
    if s.transposed:
        return len(s.cins) == 1 and not s.m and s.cout > 1
    if (s.k, s.s, s.p) == (1, 1, 0):
        return True
    return s.k == 3 and s.p == 1 and s.s in (1, 2) and len(s.cins) == 1


def _pw(c: Case) -> bool:  # conv_pw.hip: 1x1 s1 p0, plain BN / bias + activation, <= 48 couts, 4-channel sources, 4 | pixels
    s = c.launch
    if s.transposed or (s.k, s.s, s.p) != (1, 1, 0) or s.m or s.r or s.two or s.u or s.shuffle > 1 or c.post != 1.0:
        return False
    pix = s.Di * s.Hi * s.Wi
    return s.cout <= 48 and s.cin <= 192 and pix % 4 == 0 and all(v % 4 == 0 for v in s.cins)


ACCEPTS: Dict[str, Callable[[Case], bool]] = {
    "general": _general, "direct": _direct, "rows": _rows, "c1t": _c1t, "stem": _stem, "c1in": _c1in, "small": _small,
    "wide": _wide, "wide3": _wide3, "widet": _widet, "tile2": _tile2, "tile3": _tile3, "pw": _pw}

# the ESM_FORM_* value esm_conv_form reports for a forced form (the general form's variants share one)
FORM_ID = {"general": _lib.FORM_GENERAL, "direct": _lib.FORM_GENERAL, "rows": _lib.FORM_GENERAL, "c1t": _lib.FORM_GENERAL,
           "stem": _lib.FORM_STEM, "c1in": _lib.FORM_C1IN, "small": _lib.FORM_SMALL, "wide": _lib.FORM_WIDE,
           "wide3": _lib.FORM_WIDE3, "widet": _lib.FORM_WIDET, "tile2": _lib.FORM_TILE2, "tile3": _lib.FORM_TILE3,
           "pw": _lib.FORM_PW}
# an automatic choice by its ESM_FORM_* value: the ACCEPTS entry it must satisfy (GENERAL: whichever variant runs)
FORM_NAME = {_lib.FORM_GENERAL: "general", _lib.FORM_STEM: "stem", _lib.FORM_C1IN: "c1in", _lib.FORM_SMALL: "small",
             _lib.FORM_WIDE: "wide", _lib.FORM_WIDE3: "wide3", _lib.FORM_WIDET: "widet", _lib.FORM_TILE2: "tile2",
             _lib.FORM_TILE3: "tile3", _lib.FORM_PW: "pw"}

AUTO, TILE = "auto", "tile"  # stepping aside: for the automatic rules / for the LDS-tiled 1x1 its TILE bit names
# what a forced hint gets for a case the form does not run ("Addressing limits", column "past the guard"):
# the message of ESM_ERR_ARG, or the form it steps aside for (which is then held to its own entry)
REFUSAL: Dict[str, str] = {
    "direct": "conv: direct hint not applicable",
    "rows": "conv: row-streaming hint not applicable",
    "c1t": "conv: c1-transposed hint not applicable",
    "stem": "conv: stem form not applicable",
    "c1in": "conv: 1-channel-input form not applicable",
    "small": "conv: small-form hint not applicable",
    "wide": AUTO,
    "wide3": "conv: wide3-form hint not applicable",
    "widet": "conv: wide-T hint not applicable",
    "tile2": "conv: tile2-form hint not applicable",
    "tile3": "conv: tile3-form hint not applicable",
    "pw": TILE,
}


def forced_form(c: Case) -> str:
    """The form a case's hint selects (select_form): its own, but the TILE bit names the 2-D or the 3-D tiled form by
    the launch's dimension, and a pointwise hint the form cannot take leaves the TILE bit."""
    form = c.form
    if form == "pw" and not ACCEPTS["pw"](c):
        form = "tile2"
    if form in ("tile2", "tile3"):
        form = "tile3" if c.launch.nd == 3 else "tile2"
    return form


def expected(c: Case) -> Tuple[str, Optional[str]]:
    """The documented outcome of the forced launch of ``c``: ("runs", form that must be reported), ("auto", None) or
    ("refused", message)."""
    form = forced_form(c)
    if ACCEPTS[form](c):
        return "runs", form
    return ("auto", None) if REFUSAL[form] == AUTO else ("refused", REFUSAL[form])


# ----------------------------------------------------------------------------- bases


@dataclass(frozen=True)
class Base:
    name: str
    form: str
    spec: Spec
    hints: Tuple[int, ...]   # every value of the form's hint fields at this geometry; the first is the base case's


def _spec(nd, cins, cout, k, s, shape, tr=False, p=None, B=2) -> Spec:
    ext = (1,) + tuple(shape) if nd == 2 else tuple(shape)
    return Spec(nd, tr, k, s, (1 if tr else k // 2) if p is None else p, tuple(cins), cout, B, *ext, 1, False, False, False,
                False)


def _each(form, *fields):
    return tuple(form | v for v in fields)


_GEN, _DIR = (0x11, 0x44, 0x12, 0x41), (0x211, 0x241, 0x212)
_SMALL_H = _each(HINT_SMALL, 0, HINT_SMALL_W8, HINT_SMALL_NO_RECORD)
_TILE_ROWS = _each(HINT_TILE, 0, ROWS(1), ROWS(2), ROWS(3))
_GEOS2 = (("k1", 1, 1, False), ("k3s1", 3, 1, False), ("k3s2", 3, 2, False), ("k5", 5, 1, False), ("convT", 4, 2, True))
_GEOS3 = (("k1", 1, 1, False), ("k3s1", 3, 1, False), ("k3s2", 3, 2, False), ("convT", 4, 2, True))
S2, S3, S3T = (9, 21), (3, 6, 20), (2, 3, 10)  # shapes of the layouts cases (tests/test_gpu_layouts.py)


def _bases() -> List[Base]:
    out = []
    for form, hints, cin in (("general", _GEN, 12), ("direct", _DIR, 12)):
        for g, k, s, tr in _GEOS2:
            out.append(Base(f"{form}-2d-{g}", form, _spec(2, (cin,), 12 if tr else 24, k, s, S2, tr), hints))
        for g, k, s, tr in _GEOS3:
            out.append(Base(f"{form}-3d-{g}", form, _spec(3, (cin,), 12, k, s, S3T if tr else S3, tr), hints))
    for g, k in (("k1", 1), ("k3", 3), ("k5", 5)):
        out.append(Base(f"rows-2d-{g}", "rows", _spec(2, (16,), 16, k, 1, S2), (0x411,)))
    for g, k in (("k1", 1), ("k3", 3)):
        out.append(Base(f"rows-3d-{g}", "rows", _spec(3, (8,), 8, k, 1, S3), (0x411,)))
    c1t = _each(HINT_C1T, 0, ROWS(1))
    out.append(Base("c1t-2d", "c1t", _spec(2, (16,), 1, 4, 2, (7, 19), True), c1t))
    out.append(Base("c1t-3d", "c1t", _spec(3, (12,), 1, 4, 2, S3T, True), c1t))
    out.append(Base("stem-2d", "stem", _spec(2, (16,), 8, 3, 1, S2), (HINT_STEM,)))
    out.append(Base("stem-3d", "stem", _spec(3, (12,), 12, 3, 1, S3), (HINT_STEM,)))
    for g, k, s in (("k3s1", 3, 1), ("k3s2", 3, 2), ("k5", 5, 1)):
        out.append(Base(f"c1in-{g}", "c1in", _spec(2, (1,), 16, k, s, (13, 37)), (HINT_C1IN,)))
    for g, k, s, tr in _GEOS2:
        out.append(Base(f"small-2d-{g}", "small", _spec(2, (16,), 16, k, s, S2, tr), _SMALL_H))
    for g, k, s, tr in _GEOS3:
        h = _SMALL_H + ((HINT_SMALL | HINT_SMALL_NO_ZSPLIT,) if (k, s) == (3, 1) else ())
        out.append(Base(f"small-3d-{g}", "small", _spec(3, (16,), 16, k, s, S3T if tr else S3, tr), h))
    wide = _each(HINT_WIDE, 0, ROWS(1), ROWS(2), ROWS(3), ROWS(2) | HINT_WIDE_KS2, ROWS(3) | HINT_WIDE_KS2)
    for g, k, cin in (("k1", 1, 16), ("k3", 3, 16), ("k5", 5, 4)):
        out.append(Base(f"wide-{g}", "wide", _spec(2, (cin,), 16, k, 1, S2), wide))
    out.append(Base("wide3", "wide3", _spec(3, (12,), 12, 3, 1, S3), (HINT_WIDE3,)))
    out.append(Base("widet", "widet", _spec(2, (8,), 16, 4, 2, (7, 21), True), _each(HINT_WIDET, 0, ROWS(1), ROWS(2))))
    t3 = _TILE_ROWS + _each(HINT_TILE, ROWS(1) | HINT_TILE_DMA_FLIP, HINT_TILE_DMA_FLIP, HINT_TILE_WLDS, ROWS(2) | HINT_TILE_WLDS)
    out.append(Base("tile3-k3s1", "tile3", _spec(3, (8,), 8, 3, 1, S3), t3))
    out.append(Base("tile3-k3s2", "tile3", _spec(3, (8,), 24, 3, 2, S3), t3))
    out.append(Base("tile3-k1", "tile3", _spec(3, (16,), 24, 1, 1, S3), _TILE_ROWS))  # (bit 29 on a 1x1: the pointwise form)
    out.append(Base("tile3-convT", "tile3", _spec(3, (24,), 16, 4, 2, S3T, True), _TILE_ROWS))
    for g, k, s, tr in (("k3s1", 3, 1, False), ("k3s2", 3, 2, False), ("k1", 1, 1, False), ("convT", 4, 2, True)):
        out.append(Base(f"tile2-{g}", "tile2", _spec(2, (16,), 16 if tr else 32, k, s, S2, tr), _TILE_ROWS))
    out.append(Base("pw-2d", "pw", _spec(2, (16,), 16, 1, 1, (4, 20)), (HINT_TILE | HINT_TILE_PW,)))
    out.append(Base("pw-3d", "pw", _spec(3, (16,), 16, 1, 1, (2, 6, 10)), (HINT_TILE | HINT_TILE_PW,)))
    return out


BASES: List[Base] = _bases()
FORMS: Tuple[str, ...] = tuple(ACCEPTS)

# ----------------------------------------------------------------------------- axes

_EXT = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33)
AXES: Dict[str, Tuple] = {
    "p": (0, 1, 2, 3, 4, 5),
    "D": _EXT, "H": _EXT, "W": _EXT + (47, 48, 49, 63, 64, 65),
    "cin": (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 17, 20, 32, 33, 48, 49),
    "split": ((4, 4), (16, 8), (8, 8, 4), (6, 10), (1, 1, 1), (5, 4, 3)),
    "cout": (1, 2, 3, 4, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32, 33, 40, 48, 96, 97),
    "act": ACTS,
    "bn": ("bn", "bias", "none"),
    "epi": ("mul", "res", "up", "out2", "post4", "shuffle2", "shuffle4", "mul+res", "res+out2", "mul+res+out2"),
    "B": (1, 2, 3),
}


def _even_out(s: Spec) -> Spec:
    """The bilinear operand is the output at half size: the input extent grown until the output extent is even."""
    while s.out_ext[-2] % 2:
        s = replace(s, Hi=s.Hi + 1)
    while s.out_ext[-1] % 2:
        s = replace(s, Wi=s.Wi + 1)
    return s


def _with_epi(s: Spec, post: float, what: str) -> Optional[Tuple[Spec, float]]:
    """``s`` with the epilogue operands ``what`` names, or None where conv_check refuses the combination by
    definition (pixel shuffle and the bilinear add are 2-D; a shuffle is not transposed)."""
    for tok in what.split("+"):
        if tok == "mul":
            s = replace(s, m=True)
        elif tok == "res":
            s = replace(s, r=True)
        elif tok == "out2":
            s = replace(s, two=True)
        elif tok == "post4":
            post = 4.0
        elif tok == "up":
            if s.nd != 2:
                return None
            s = _even_out(replace(s, u=True, cout=1))
        elif tok.startswith("shuffle"):
            if s.nd != 2 or s.transposed:
                return None
            s = replace(s, shuffle=int(tok[7:]), cout=16)
    return s, post


def _alive(s: Spec) -> bool:
    return min(s.out_ext) > 0


def axis_cases(b: Base) -> List[Case]:
    """The base case and one case per value of every axis, the other fields at the base's."""
    s0 = b.spec
    mk = lambda spec, axis, value, **kw: Case(spec, b.form, kw.pop("hint", b.hints[0]), axis=axis, value=str(value),  # noqa: E731
                                              base=b.name, **kw)
    out = [mk(s0, "base", "")]
    for p in AXES["p"]:
        if p <= s0.k and (not s0.transposed or p == 1):
            out.append(mk(replace(s0, p=p), "p", p))
    for ax, field in (("D", "Di"), ("H", "Hi"), ("W", "Wi")):
        if ax == "D" and s0.nd == 2:
            continue
        out += [mk(replace(s0, **{field: v}), ax, v) for v in AXES[ax]]
    out += [mk(replace(s0, cins=(v,)), "cin", v) for v in AXES["cin"]]
    out += [mk(replace(s0, cins=v), "split", "+".join(map(str, v))) for v in AXES["split"]]
    out += [mk(replace(s0, cout=v), "cout", v) for v in AXES["cout"]]
    out += [mk(s0, "act", a, act=a, gain=ACT_GAIN) for a in AXES["act"]]
    out += [mk(s0, "bn", v, bn=v) for v in AXES["bn"]]
    for e in AXES["epi"]:
        se = _with_epi(s0, 1.0, e)
        if se is not None:
            out.append(mk(se[0], "epi", e, post=se[1]))
    out += [mk(replace(s0, B=v), "B", v) for v in AXES["B"]]
    out += [mk(s0, "hint", hex(h), hint=h) for h in b.hints]
    return [c for c in out if _alive(c.spec)]


RANDOM_PER_FORM = 96
_KEEP = 0.6  # a random combination leaves each axis at the base's value with this probability


@functools.lru_cache(maxsize=None)
def random_cases(form: str) -> Tuple[Case, ...]:
    """Seeded combinations around the form's bases: interactions single axes cannot show (p = 3 at W = 17 with two
    sources and a residual)."""
    rng = np.random.default_rng(zlib.crc32(form.encode()))
    bases = [b for b in BASES if b.form == form]
    out: List[Case] = []
    n = 0
    while len(out) < RANDOM_PER_FORM:
        n += 1
        b = bases[int(rng.integers(len(bases)))]
        s = b.spec
        pick = lambda vals: vals[int(rng.integers(len(vals)))]  # noqa: E731
        vary = lambda: rng.random() >= _KEEP  # noqa: E731
        if vary() and not s.transposed:
            s = replace(s, p=int(rng.integers(0, s.k + 1)))
        for ax, field in (("D", "Di"), ("H", "Hi"), ("W", "Wi")):
            if (ax != "D" or s.nd == 3) and vary():
                s = replace(s, **{field: pick(AXES[ax])})
        if vary():
            s = replace(s, cins=(pick(AXES["cin"]),) if rng.random() < 0.6 else pick(AXES["split"]))
        if vary():
            s = replace(s, cout=pick(AXES["cout"]))
        act = pick(ACTS) if vary() else ACT_GELU
        bn = pick(AXES["bn"]) if vary() else "bn"
        post = 1.0
        if vary():
            se = _with_epi(s, post, pick(AXES["epi"]))
            if se is not None:
                s, post = se
        if vary():
            s = replace(s, B=pick(AXES["B"]))
        hint = pick(b.hints) if vary() else b.hints[0]
        if _alive(s):
            out.append(Case(s, form, hint, act=act, bn=bn, post=post, axis="random", value=str(n), base=b.name))
    return tuple(out)


# (kernel, stride) pairs conv_check lets through and no form instantiates, small and beyond the lean form's 2^17
# (pixel x cout tile) automatic bound: ESM_ERR_UNSUPPORTED at every size
OUTSIDE: List[Case] = [
    Case(_spec(nd, (4,), 16, k, s, shape, p=k // 2, B=1), "general", 0, axis="outside", value=f"{nd}d k{k}s{s} {shape}", base="outside")
    for nd, k, s, shapes in ((2, 1, 2, ((9, 21), (600, 900))), (2, 5, 2, ((9, 21), (600, 900))), (2, 2, 1, ((9, 21),)),
                             (2, 7, 1, ((9, 21),)), (3, 1, 2, ((3, 6, 20), (24, 240, 200))), (3, 5, 1, ((5, 6, 20),)),
                             (3, 5, 2, ((5, 6, 20),)))
    for shape in shapes]


def cases_of(b: Base) -> List[Case]:
    """Every case a base's GPU test walks: its axis cases and its share of the form's random combinations."""
    return axis_cases(b) + [c for c in random_cases(b.form) if c.base == b.name]


def all_cases() -> List[Case]:
    return [c for b in BASES for c in axis_cases(b)] + [c for f in FORMS for c in random_cases(f)]


# ----------------------------------------------------------------------------- values no case of a form can run

# NEVER[form]: (axis, values or None for the whole axis, reason).  The coverage condition of
# tests/test_conv_domain_host.py asks for one accepted case per (form, axis value) outside this table, and for none
# inside it.
_ODD_SPLITS = ("6+10", "1+1+1", "5+4+3")
_NOT_P1 = (0, 2, 3, 4, 5)
_MUL = ("mul", "mul+res", "mul+res+out2")
_SHUFFLE = ("shuffle2", "shuffle4")
_T = "transposed convs are k4 s2 p1 (conv_check)"
_ONE_SRC = "one source only"
_ALIGNED = "direct_ok: the splits of a multi-source input lie on 4-channel boundaries"
_2D = "a 2-D form"
_NO_K5 = "the padding axis ends at k, and the form has no 5x5"


def _couts(ok) -> Tuple[int, ...]:
    return tuple(v for v in AXES["cout"] if not ok(v))


def _cins(ok) -> Tuple[int, ...]:
    return tuple(v for v in AXES["cin"] if not ok(v))


NEVER: Dict[str, List[Tuple[str, Optional[Sequence], str]]] = {
    "general": [],
    "direct": [("split", _ODD_SPLITS, _ALIGNED)],
    "rows": [("cin", _cins(lambda v: v <= 16), "one 16-channel chunk: the row pipeline keeps one row's operands live"),
             ("split", None, _ONE_SRC)],
    "c1t": [("cin", _cins(lambda v: v <= 32), "<= 32 input channels"), ("cout", _couts(lambda v: v == 1), "one output channel"),
            ("epi", _SHUFFLE, "conv_check: no pixel shuffle on a transposed conv"), ("p", _NOT_P1, _T), ("split", None, _ONE_SRC)],
    "stem": [("cout", _couts(lambda v: v in (8, 12, 16, 24, 32)), "8, 12, 16, 24 or 32 output channels"),
             ("epi", _SHUFFLE, "no pixel shuffle"), ("epi", ("up",), "the bilinear add needs one output channel"),
             ("p", _NOT_P1, '"same" padding only'), ("split", None, _ONE_SRC)],
    "c1in": [("D", None, _2D), ("cin", _cins(lambda v: v == 1), "one input channel"),
             ("cout", _couts(lambda v: v <= 32), "<= 32 output channels"),
             ("epi", tuple(e for e in AXES["epi"] if e != "post4"), "plain store: no operand but post_scale"),
             ("split", None, _ONE_SRC)],
    "small": [("epi", _MUL + _SHUFFLE + ("up",), "plain epilogue: no mul, bilinear add or shuffle"), ("split", _ODD_SPLITS, _ALIGNED)],
    "wide": [("D", None, _2D), ("cout", _couts(lambda v: v <= 32), "<= 32 output channels"),
             ("epi", _MUL + _SHUFFLE + ("up",), "no mul, bilinear add or shuffle"), ("split", _ODD_SPLITS, _ALIGNED)],
    "wide3": [("cin", _cins(lambda v: v <= 32), "<= 32 input channels"), ("cout", _couts(lambda v: v <= 16), "<= 16 output channels"),
              ("epi", _SHUFFLE + ("up",), "3-D: conv_check refuses both"), ("p", _NOT_P1, "3x3x3 p1 only"),
              ("split", None, _ONE_SRC)],
    "widet": [("D", None, _2D), ("cin", _cins(lambda v: v <= 16), "16 * channel groups * cout tiles <= 64 weight registers"),
              ("cout", _couts(lambda v: v <= 32), "<= 32 output channels"),
              ("epi", _MUL + ("up",), "no mul or bilinear add"), ("epi", _SHUFFLE, "conv_check: no pixel shuffle on a transposed conv"),
              ("p", _NOT_P1, _T), ("split", None, _ONE_SRC)],
    "tile2": [("D", None, _2D), ("cout", (97,), "<= 96 output channels"), ("epi", _SHUFFLE + ("up",), "no shuffle or bilinear add"),
              ("p", (4, 5), _NO_K5), ("split", _ODD_SPLITS, _ALIGNED)],
    "tile3": [("cout", (97,), "<= 96 output channels"), ("epi", _SHUFFLE + ("up",), "3-D: conv_check refuses both"),
              ("p", (2, 3, 4, 5), "3x3x3 p1 and 1x1x1 p0 only"), ("split", _ODD_SPLITS, _ALIGNED)],
    "pw": [("cin", _cins(lambda v: v % 4 == 0), "16-byte loads: 4-channel sources"), ("cout", (96, 97), "<= 48 output channels"),
           ("epi", None, "BN / bias and activation only"), ("p", (1, 2, 3, 4, 5), "1x1 p0 only"), ("split", _ODD_SPLITS, _ALIGNED)],
}
