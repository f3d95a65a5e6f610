"""The tuned-hint table (esmstereo_amd/tuned_hints.json) as test input.

Every row of the table is a shape key (``engine.conv_key``) and the hint the engine puts into
``esm_conv_desc.hint`` for a conv launch of exactly that shape.  This module turns a key back into the
layer and the tensors it names (``parse_key`` / ``format_key``), and gives the tests a bounded fp64
reference for tensors of the rows' own size: ``windows`` picks a few output windows (corners, one
interior, three batch items) and ``window_ref`` computes one of them from the input crop it depends on
alone, so nothing of the size of the whole tensor is ever convolved on the CPU.

Nothing here needs a GPU; tensors handed to ``window_ref`` may live on any device (only the crop is moved).
"""
from __future__ import annotations

import json
import os
import random
import re
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

TABLE_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "esmstereo_amd",
                          "tuned_hints.json")

# engine.conv_key: "<nd>d[T] k<k>s<s>p<p> <c0>[+<c1>[+<c2>]]-><cout> B<B> <Di>x<Hi>x<Wi> sh<r>[u][m][r][2]".
# The shuffle factor is one digit (1, 2, 4: nn.PixelShuffle of the reference's heads), so the out2 flag "2"
# behind it reads unambiguously.  Anything else does not match: an unknown flag or layout must raise.
_KEY = re.compile(r"^(?P<nd>[23])d(?P<T>T?) k(?P<k>\d+)s(?P<s>\d+)p(?P<p>\d+) (?P<cins>\d+(?:\+\d+){0,2})->(?P<cout>\d+) "
                  r"B(?P<B>\d+) (?P<Di>\d+)x(?P<Hi>\d+)x(?P<Wi>\d+) sh(?P<sh>\d)(?P<u>u?)(?P<m>m?)(?P<r>r?)(?P<two>2?)$")


@dataclass(frozen=True)
class Spec:
    """One conv launch as its shape key names it."""

    nd: int
    transposed: bool
    k: int
    s: int
    p: int
    cins: Tuple[int, ...]   # the source channel split (the sources are concatenated along channels)
    cout: int
    B: int
    Di: int
    Hi: int
    Wi: int
    shuffle: int
    u: bool                 # + bilinear(up) in the epilogue
    m: bool                 # * mul
    r: bool                 # + res
    two: bool               # a second, separately scaled output (out2)

    @property
    def cin(self) -> int:
        return sum(self.cins)

    @property
    def in_ext(self) -> Tuple[int, ...]:
        """Input spatial extent: (Di, Hi, Wi) in 3-D, (Hi, Wi) in 2-D."""
        return (self.Di, self.Hi, self.Wi) if self.nd == 3 else (self.Hi, self.Wi)

    @property
    def out_ext(self) -> Tuple[int, ...]:
        """Conv output extent before any PixelShuffle (engine._conv_desc's Do / Ho / Wo)."""
        if self.transposed:
            return tuple(2 * v for v in self.in_ext)
        return tuple((v + 2 * self.p - self.k) // self.s + 1 for v in self.in_ext)


def parse_key(key: str) -> Spec:
    """Invert ``engine.conv_key``.  Raises ValueError for anything the format does not produce."""
    g = _KEY.match(key)
    if g is None:
        raise ValueError(f"tuned row {key!r}: not a conv_key (unknown flag or layout)")
    nd = int(g["nd"])
    spec = Spec(nd, g["T"] == "T", int(g["k"]), int(g["s"]), int(g["p"]), tuple(int(c) for c in g["cins"].split("+")),
                int(g["cout"]), int(g["B"]), int(g["Di"]), int(g["Hi"]), int(g["Wi"]), int(g["sh"]),
                bool(g["u"]), bool(g["m"]), bool(g["r"]), bool(g["two"]))
    if nd == 2 and spec.Di != 1:
        raise ValueError(f"tuned row {key!r}: a 2-D launch has depth 1")
    if spec.transposed and (spec.k, spec.s, spec.p) != (4, 2, 1):
        raise ValueError(f"tuned row {key!r}: transposed convs are k4 s2 p1")
    if min(spec.cins) < 1 or min(spec.cout, spec.B, spec.s, spec.k, spec.shuffle) < 1 or min(spec.out_ext) < 1:
        raise ValueError(f"tuned row {key!r}: empty layer or extent")
    if format_key(spec) != key:  # leading zeros and the like: two spellings of one launch never share a row
        raise ValueError(f"tuned row {key!r}: not in conv_key's own spelling")
    return spec


def format_key(spec: Spec) -> str:
    """The string ``engine.conv_key`` gives a launch of this spec."""
    return (f"{spec.nd}d{'T' if spec.transposed else ''} k{spec.k}s{spec.s}p{spec.p} "
            f"{'+'.join(str(c) for c in spec.cins)}->{spec.cout} B{spec.B} {spec.Di}x{spec.Hi}x{spec.Wi} "
            f"sh{spec.shuffle}{'u' if spec.u else ''}{'m' if spec.m else ''}{'r' if spec.r else ''}{'2' if spec.two else ''}")


def load_table(path: str = TABLE_PATH) -> Dict[str, int]:
    with open(path) as f:
        return {k: int(v) for k, v in json.load(f)["hints"].items()}


# ----------------------------------------------------------------------------- windowed fp64 reference


def crop_range(spec: Spec, lo: Sequence[int], hi: Sequence[int]) -> List[Tuple[int, int, int, int]]:
    """Per spatial dim: (start, stop, pad_before, pad_after) of the input the output window [lo, hi) reads,
    start / stop clamped to the tensor, the pads the zero border the clamp cut off (0 for transposed)."""
    out = []
    for n, a, b in zip(spec.in_ext, lo, hi):
        if spec.transposed:  # output o reads inputs ceil((o - 2) / 2) .. floor((o + 1) / 2)
            s0, s1 = (a - 2) // 2, b // 2 + 1
        else:
            s0, s1 = a * spec.s - spec.p, (b - 1) * spec.s - spec.p + spec.k
        c0, c1 = max(s0, 0), min(s1, n)
        out.append((c0, c1, 0, 0) if spec.transposed else (c0, c1, c0 - s0, s1 - c1))
    return out


def window_ref(x_b: Union[torch.Tensor, Sequence[torch.Tensor]], weight: torch.Tensor, spec: Spec, lo: Sequence[int],
               hi: Sequence[int]) -> torch.Tensor:
    """fp64 conv output [Cout, *(hi - lo)] of ONE batch item over the output window [lo, hi) (conv output
    coordinates, nd of them), bias-free, before BN and activation.  ``x_b``: the item's input [Cin, *in_ext], or
    its sources (concatenated along channels); only the crop the window reads is sliced out and moved to the
    CPU.  ``weight``: the torch layer's weight."""
    srcs = [x_b] if isinstance(x_b, torch.Tensor) else list(x_b)
    rng = crop_range(spec, lo, hi)
    sl = (slice(None),) + tuple(slice(c0, c1) for c0, c1, _, _ in rng)
    x = torch.cat([t[sl].detach().to("cpu", torch.float64) for t in srcs], 0).unsqueeze(0)
    w = weight.detach().to("cpu", torch.float64)
    if spec.transposed:
        y = (F.conv_transpose3d if spec.nd == 3 else F.conv_transpose2d)(x, w, None, spec.s, spec.p)
        off = tuple(a - 2 * c0 for a, (c0, _, _, _) in zip(lo, rng))
    else:
        pads = [v for _, _, pb, pa in reversed(rng) for v in (pb, pa)]  # F.pad: last dim first
        y = (F.conv3d if spec.nd == 3 else F.conv2d)(F.pad(x, pads), w, None, spec.s, 0)
        off = (0,) * spec.nd
    y = y[(0, slice(None)) + tuple(slice(o, o + b - a) for o, a, b in zip(off, lo, hi))]
    if tuple(y.shape[1:]) != tuple(b - a for a, b in zip(lo, hi)):
        raise AssertionError(f"window_ref: window {tuple(lo)}..{tuple(hi)} came out as {tuple(y.shape[1:])}")
    return y


WINDOW_2D = (24, 80)      # >= three 8-row blocks and five 16-column strips: a ragged last strip at the high corner
WINDOW_3D = (6, 12, 40)


def windows(spec: Spec, extent: Optional[Sequence[int]] = None) -> List[Tuple[int, Tuple[int, ...], Tuple[int, ...]]]:
    """(batch item, lo, hi) of the output windows to check: items 0, B // 2 and B - 1; the all-low corner, the
    all-high corner, one mixed corner (low / high alternating, the innermost dim high) and one interior window
    whose origin is seeded by the key.  A dim the map does not exceed is taken whole.  ``extent``: another
    window extent than WINDOW_2D / WINDOW_3D (the host test of this function, on small maps)."""
    ext = spec.out_ext
    win = tuple(min(e, w) for e, w in zip(ext, extent or (WINDOW_3D if spec.nd == 3 else WINDOW_2D)))
    top = tuple(e - w for e, w in zip(ext, win))
    rnd = random.Random(zlib.crc32(format_key(spec).encode()))
    origins = [tuple(0 for _ in ext), top,
               tuple(t if (spec.nd - 1 - i) % 2 == 0 else 0 for i, t in enumerate(top)),
               tuple(rnd.randint(min(1, t), max(t - 1, min(1, t))) if t else 0 for t in top)]
    out, seen = [], set()
    for b in (0, spec.B // 2, spec.B - 1):
        for o in origins:
            if (b, o) not in seen:
                seen.add((b, o))
                out.append((b, o, tuple(a + w for a, w in zip(o, win))))
    return out


def window_expect(x_b, weight: torch.Tensor, spec: Spec, lo: Sequence[int], hi: Sequence[int], scale: torch.Tensor,
                  shift: torch.Tensor, act, mul_b: Optional[torch.Tensor] = None, res_b: Optional[torch.Tensor] = None,
                  up_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``window_ref`` pushed through the launch's epilogue in fp64, in the kernels' order (conv_epilogue.h): folded
    BN ``* scale + shift`` per cout, ``act`` (a callable), ``* mul``, ``+ res``, ``+ up``.  The operands are ONE batch
    item's, on any device (only the window is moved): ``mul_b`` [Cout, Ho, Wo] (broadcast over D), ``res_b``
    [Cout, *out_ext], ``up_b`` [1, Ho, Wo]: the bilinear map already interpolated to the output extent in fp64."""
    bc = (slice(None),) + (None,) * spec.nd
    win = (slice(None),) + tuple(slice(a, b) for a, b in zip(lo, hi))
    cpu64 = lambda t: t.detach().to("cpu", torch.float64)  # noqa: E731
    y = act(window_ref(x_b, weight, spec, lo, hi) * cpu64(scale)[bc] + cpu64(shift)[bc])
    if mul_b is not None:
        m = cpu64(mul_b[(slice(None),) + win[-2:]])
        y = y * (m.unsqueeze(1) if spec.nd == 3 else m)
    if res_b is not None:
        y = y + cpu64(res_b[win])
    if up_b is not None:
        y = y + cpu64(up_b[win])
    return y
