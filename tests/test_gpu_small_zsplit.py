"""The lean form's tap-plane split of 3x3x3 convs (conv_small.hip lconv_body ZS).

Layers of at most six 4-channel groups whose grid is resident at once (workgroups x waves <= 8192) split the K
reduction by (group, tap plane dz) into units of 9 taps over 8, 12 or 16 waves; HINT_SMALL_NO_ZSPLIT selects the loop
the split replaced (one wave per group, 27 taps in series).  The two differ by fp32 reassociation only: every case is
checked against fp64 torch and against the plain loop at relative 1e-5, and twice against itself bitwise (the sum
order is fixed).  Outside the split's range the hint bit changes nothing, bitwise.
"""
from __future__ import annotations

import pytest
import torch

from layouts import assert_guards_intact, embed, guard_snapshot
from test_gpu_parity import _mk, _ref_conv, pk, rel

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

from esmstereo_amd._lib import HINT_SMALL, HINT_SMALL_NO_ZSPLIT  # noqa: E402
from esmstereo_amd.engine import ACT_GELU, Ctx, run_conv  # noqa: E402

DEV = torch.device("cuda")

CASES = [  # (source channels, cout, stride, volume, B, the split runs; None: it does, in the plain loop's sum order)
    ((8,), 8, 1, (4, 6, 20), 1, True),      # G = 2
    ((8,), 12, 2, (4, 6, 20), 1, True),     # G = 2, stride 2
    ((12,), 16, 2, (6, 12, 39), 1, True),   # G = 3, stride 2 (-> 3x6x20)
    ((16,), 16, 1, (3, 6, 20), 1, True),    # G = 4
    ((16,), 24, 2, (3, 6, 20), 1, True),    # two cout tiles (-> 2x3x10)
    ((24,), 24, 1, (2, 3, 10), 1, True),    # G = 6, two cout tiles
    # one plane (two tap planes skipped), channel tail, ragged width, batch 2; one unit per group: the plain loop's order
    ((10,), 12, 1, (1, 5, 19), 2, None),
    ((8, 4), 12, 1, (2, 7, 17), 1, True),   # concat of two sources
    ((28,), 16, 1, (2, 3, 10), 1, False),   # G = 7: the plain loop either way
    ((8,), 8, 1, (32, 32, 16), 1, True),    # 1024 workgroups x 8 waves: the last grid the split takes
    ((8,), 8, 1, (32, 33, 16), 1, False),   # 1056 workgroups: past it, the plain loop either way
    ((8,), 8, 1, (12, 24, 78), 1, False),   # the S-K `agg` volume (1440 workgroups): the plain loop
]


@pytest.mark.parametrize("cins,cout,s,shape,B,split", CASES)
def test_small_zsplit(cins, cout, s, shape, B, split):
    conv, bn = _mk(3, sum(cins), cout, 3, s, 1, seed=7 + sum(cins))
    xs = [torch.randn(B, c, *shape) for c in cins]
    ref = _ref_conv(xs, conv, bn, ACT_GELU)
    p = pk(conv, bn, ACT_GELU)
    xd = [x.to(DEV) for x in xs]
    y = run_conv(Ctx(DEV), p, xd, hint=HINT_SMALL)
    assert y.shape == ref.shape
    assert rel(y, ref) < 1e-5
    plain = run_conv(Ctx(DEV), p, xd, hint=HINT_SMALL | HINT_SMALL_NO_ZSPLIT)
    assert rel(plain, ref) < 1e-5
    assert rel(y, plain) < 1e-5
    again = run_conv(Ctx(DEV), p, xd, hint=HINT_SMALL)
    assert torch.equal(y, again)
    # another sum order shows in the last bits of some of the volume's elements; the same loop in none
    if split is not None:
        assert torch.equal(y, plain) != split


def test_small_zsplit_layout_odd():
    """Sources and output as 4-byte-aligned, odd-stride views inside poisoned allocations (layouts.py)."""
    conv, bn = _mk(3, 12, 16, 3, 1, 1, seed=19)
    x = torch.randn(2, 12, 3, 5, 19)
    ref = _ref_conv([x], conv, bn, ACT_GELU)
    p = pk(conv, bn, ACT_GELU)
    out = embed(torch.zeros(ref.shape), "odd", DEV)
    snap = guard_snapshot(out)
    y = run_conv(Ctx(DEV), p, [embed(x, "odd", DEV)], out, hint=HINT_SMALL)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()), "a value from outside the logical extent reached the output"
    assert rel(y, ref) < 1e-5
    assert_guards_intact(out, snap, "odd")
    assert torch.equal(y.contiguous(), run_conv(Ctx(DEV), p, [x.to(DEV)], hint=HINT_SMALL))
