"""The fused conv launches' descriptor domain (companion of tests/conv_domain.py): ``esm_conv_pair2_f32`` (LDS-staged and
K-split) and ``esm_convt_1x1_f32`` (lean and LDS-tiled), with reduced axes: the padding of both convs, extents, the
channel counts of both, batch.  ``engine.py``'s predicates, which decide what the hot path fuses, ask the library's form
queries (esm_conv_pair2_form, esm_convt_1x1_form) about the descriptors a launch would get; ``pair_query`` /
``up1_query`` evaluate them on shape-only tensors, and tests/test_gpu_conv_domain.py holds the launchers to the answers.
Nothing here needs a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import List, Tuple

import torch

from esmstereo_amd import engine as EN
from esmstereo_amd._lib import ACT_GELU, HINT_SMALL, HINT_SMALL_W8, HINT_TILE
from esmstereo_amd._lib import HINT_ROWS as ROWS


def _packed(nd, cin, cout, k, s, p, transposed=False):
    """What the predicates read of a PackedConv (BN + GELU): its geometry, and shape-only weights / BN constants."""
    cin_pad, cout_pad = (cin + 15) // 16 * 16, (cout + 31) // 32 * 32
    taps = (2 ** nd) ** 2 if transposed else k ** nd
    w = torch.empty(taps * cin_pad * cout_pad, device="meta")
    bn = torch.empty(cout, device="meta")
    return EN.PackedConv(w, bn, bn, ACT_GELU, nd, k, s, p, transposed, cin, cout, cin_pad, cout_pad)


@dataclass(frozen=True)
class PairCase:
    """convB(convA(cat(sources))): two BasicConvs in one launch."""

    name: str
    nd: int
    cins: Tuple[int, ...]
    ka: int
    sa: int
    pa: int
    couta: int
    kb: int
    pb: int
    coutb: int
    shape: Tuple[int, ...]
    B: int = 2
    ksplit: bool = False     # PAIRK in convB's hint
    regress: bool = False    # PAIR_REGRESS: convA's input is the disparity regression of a cost volume
    axis: str = "base"
    value: str = ""

    @property
    def id(self) -> str:
        return (f"pair {self.name} {self.nd}d {'+'.join(map(str, self.cins))}->k{self.ka}s{self.sa}p{self.pa}->{self.couta}"
                f"->k{self.kb}p{self.pb}->{self.coutb} B{self.B} {'x'.join(map(str, self.shape))} ks{int(self.ksplit)} "
                f"rg{int(self.regress)} [{self.axis}={self.value}]")

    @property
    def mid_ext(self) -> Tuple[int, ...]:
        return tuple((v + 2 * self.pa - self.ka) // self.sa + 1 for v in self.shape)

    @property
    def out_ext(self) -> Tuple[int, ...]:
        return tuple(v + 2 * self.pb - self.kb + 1 for v in self.mid_ext)


def pair_query(c: PairCase, tensor) -> Tuple[bool, bool]:
    """(engine._pair2_lds_supported, engine.pairk_supported) of the pair; ``tensor(*shape)`` makes a source."""
    pa = _packed(c.nd, sum(c.cins), c.couta, c.ka, c.sa, c.pa)
    pb = _packed(c.nd, c.couta, c.coutb, c.kb, 1, c.pb)
    srcs = [tensor(c.B, ci, *c.shape) for ci in c.cins]
    return bool(EN._pair2_lds_supported(pa, pb, srcs)), bool(EN.pairk_supported(pa, pb, srcs))


_PAIR_BASES = [
    PairCase("lds-k3s1", 2, (16,), 3, 1, 1, 16, 3, 1, 16, (9, 21)),
    PairCase("lds-k3s2", 2, (16,), 3, 2, 1, 16, 3, 1, 16, (9, 21)),
    PairCase("lds-k5", 2, (1,), 5, 1, 2, 16, 3, 1, 16, (9, 21)),
    PairCase("lds-k1-kb1", 2, (16, 16), 1, 1, 0, 16, 1, 0, 12, (9, 21)),
    PairCase("lds-regress", 2, (1,), 5, 1, 2, 16, 3, 1, 16, (7, 19), regress=True),
    PairCase("ksplit-2d-s1", 2, (16,), 3, 1, 1, 16, 3, 1, 16, (9, 21), ksplit=True),
    PairCase("ksplit-2d-s2", 2, (12,), 3, 2, 1, 12, 3, 1, 12, (9, 21), ksplit=True),
    PairCase("ksplit-3d-s1", 3, (16,), 3, 1, 1, 16, 3, 1, 16, (3, 6, 20), ksplit=True),
    PairCase("ksplit-3d-s2", 3, (16,), 3, 2, 1, 16, 3, 1, 16, (3, 6, 20), ksplit=True),
]
_PAIR_EXT = (1, 2, 3, 7, 13, 14, 15, 16, 17, 31, 33)


def _pair_cases() -> List[PairCase]:
    out = []
    for b in _PAIR_BASES:
        v = lambda axis, value, **kw: replace(b, axis=axis, value=str(value), **kw)  # noqa: E731
        out.append(b)
        out += [v("pa", p, pa=p) for p in range(b.ka + 1)]
        out += [v("pb", p, pb=p) for p in range(b.kb + 1)]
        for i, ax in enumerate("DHW"[-b.nd:]):
            out += [v(ax, n, shape=b.shape[:i] + (n,) + b.shape[i + 1:]) for n in _PAIR_EXT]
        if not b.regress:
            out += [v("cin", n, cins=(n,)) for n in (1, 3, 4, 9, 16, 33, 48, 49, 64, 65)]
            out += [v("split", "+".join(map(str, s)), cins=s) for s in ((16, 8), (8, 8, 4), (6, 10))]
            out += [v("couta", n, couta=n) for n in (8, 12, 16, 17, 32, 33)]
        out += [v("coutb", n, coutb=n) for n in (1, 3, 8, 15, 16, 17, 32, 33)]
        out += [v("B", n, B=n) for n in (1, 2, 3)]
    return [c for c in out if min(c.mid_ext) > 0 and min(c.out_ext) > 0]


PAIR_CASES: List[PairCase] = _pair_cases()


@dataclass(frozen=True)
class Up1Case:
    """conv1x1(cat(crop(convT(x)), extras)): the transposed conv and the 1x1 after it in one launch."""

    name: str
    nd: int
    cin: int
    cy: int                  # the transposed conv's output channels
    cxs: Tuple[int, ...]     # extra sources' channels
    coutb: int
    grid: Tuple[int, ...]    # the transposed conv's input extent
    crop: bool               # the extras one short of 2 x grid in every dim, or the full extent
    hint: int                # the transposed conv's hint: the lean or the LDS-tiled form
    B: int = 2
    axis: str = "base"
    value: str = ""

    @property
    def id(self) -> str:
        return (f"up1 {self.name} {self.nd}d {self.cin}->{self.cy}+{'+'.join(map(str, self.cxs))}->{self.coutb} B{self.B} "
                f"{'x'.join(map(str, self.grid))} crop{int(self.crop)} h{self.hint:#x} [{self.axis}={self.value}]")

    @property
    def out_ext(self) -> Tuple[int, ...]:
        return tuple(2 * v - int(self.crop) for v in self.grid)


def up1_query(c: Up1Case, tensor) -> bool:
    """engine.convt_1x1_supported of the launch; ``tensor(*shape)`` makes an extra source."""
    pa = _packed(c.nd, c.cin, c.cy, 4, 2, 1, transposed=True)
    pb = _packed(c.nd, c.cy + sum(c.cxs), c.coutb, 1, 1, 0)
    return bool(EN.convt_1x1_supported(pa, pb, [tensor(c.B, cx, *c.out_ext) for cx in c.cxs]))


_UP1_BASES = [
    Up1Case("2d-lean", 2, 12, 12, (16,), 16, (6, 10), True, HINT_SMALL),
    Up1Case("2d-lean-w8", 2, 24, 12, (16, 8), 16, (6, 10), False, HINT_SMALL | HINT_SMALL_W8),
    Up1Case("2d-tiled", 2, 12, 12, (16,), 16, (6, 10), True, HINT_TILE | ROWS(2)),
    Up1Case("2d-tiled-rows1", 2, 12, 12, (16, 8), 16, (6, 10), False, HINT_TILE | ROWS(1)),
    Up1Case("3d-lean", 3, 24, 8, (4,), 12, (2, 4, 5), True, HINT_SMALL),
    Up1Case("3d-tiled", 3, 24, 8, (4,), 12, (2, 4, 5), False, HINT_TILE | ROWS(1)),
    Up1Case("3d-tiled-two-tiles", 3, 24, 20, (8, 4), 28, (2, 3, 5), True, HINT_TILE | ROWS(2)),
]
_UP1_EXT = (1, 2, 3, 7, 8, 9, 16, 17)


def _up1_cases() -> List[Up1Case]:
    out = []
    for b in _UP1_BASES:
        v = lambda axis, value, **kw: replace(b, axis=axis, value=str(value), **kw)  # noqa: E731
        out.append(b)
        out.append(v("crop", int(not b.crop), crop=not b.crop))
        for i, ax in enumerate("DHW"[-b.nd:]):
            out += [v(ax, n, grid=b.grid[:i] + (n,) + b.grid[i + 1:]) for n in _UP1_EXT]
        out += [v("cin", n, cin=n) for n in (1, 4, 7, 16, 33, 48)]
        out += [v("cy", n, cy=n) for n in (4, 6, 8, 16, 20, 32, 36)]
        out += [v("cxs", "+".join(map(str, s)), cxs=s) for s in ((4,), (6,), (16,), (32,), (48,), (4, 4), (24, 24), (28, 24))]
        out += [v("coutb", n, coutb=n) for n in (1, 4, 15, 16, 17, 32, 33)]
        out += [v("B", n, B=n) for n in (1, 2, 3)]
    return [c for c in out if min(c.out_ext) > 0]


UP1_CASES: List[Up1Case] = _up1_cases()
