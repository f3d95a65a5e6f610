"""The K-split conv pair (conv_pairk.hip: two 3x3 / 3x3x3 BasicConvs in one launch, convA recomputed on
convB's halo, the K reduction of both phases split over the workgroup's waves) against fp64 torch of the two
layers and against the two separate launches, relative 1e-5 like every conv form of test_gpu_parity.py.
Batch 2 and random BN with nonzero shifts everywhere, so a wrong padding value (GELU(shift) instead of 0)
shows; every case forces the K-split form."""
import pytest
import torch

from test_gpu_parity import _mk, _ref_conv, pk, rel

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

from esmstereo_amd import engine as EN  # noqa: E402
from esmstereo_amd.engine import ACT_GELU, Ctx, pairk_supported, run_conv, run_pair2  # noqa: E402

DEV = torch.device("cuda")

CASES = [  # (nd, cins, stride A, cout A, cout B, input extent): the smallest extents that cross every seam
    (2, (16,), 2, 16, 16, (25, 79)),        # odd extents, ragged stride-2 edge, several 14-column tiles, partial last
    (2, (16,), 2, 16, 12, (9, 40)),         # convB Cout < 16
    (2, (16, 32), 1, 16, 16, (7, 13)),      # three-way source selection (two sources), map narrower than one tile
    (3, (8,), 2, 12, 12, (5, 7, 19)),       # -> 3x4x10
    (3, (12,), 2, 16, 16, (6, 12, 39)),     # -> 3x6x20
    (3, (16,), 2, 24, 24, (3, 6, 20)),      # -> 2x3x10: two cout tiles, the workload's own shape
    (3, (16,), 2, 24, 24, (3, 5, 17)),      # two cout tiles, ragged
]
_CACHE = {}


def _case(i):
    """(packed convA, packed convB, device inputs, fp64 reference, two-launch result) of CASES[i], computed once."""
    if i not in _CACHE:
        nd, cins, sa, ca_, cb_, ext = CASES[i]
        ca, ba = _mk(nd, sum(cins), ca_, 3, sa, 1, seed=71 + i)
        cb, bb = _mk(nd, ca_, cb_, 3, 1, 1, seed=81 + i)
        torch.manual_seed(91 + i)
        xs = [torch.randn(2, c, *ext) for c in cins]
        ref = _ref_conv([_ref_conv(xs, ca, ba, ACT_GELU)], cb, bb, ACT_GELU)
        pa, pb = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
        xd = [x.to(DEV) for x in xs]
        ctx = Ctx(DEV)
        two = run_conv(ctx, pb, [run_conv(ctx, pa, xd)]).clone()
        _CACHE[i] = (pa, pb, xd, ref, two)
    return _CACHE[i]


def _check(y, ref, two):
    assert y.shape == ref.shape
    e_ref, e_two = rel(y, ref), rel(y, two)
    print(f"rel vs fp64 {e_ref:.3g}, vs two launches {e_two:.3g}")
    assert e_ref < 1e-5
    assert e_two < 1e-5


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{c[0]}d-{'x'.join(map(str, c[5]))}-{c[4]}" for c in CASES])
def test_pair_ksplit(i):
    pa, pb, xd, ref, two = _case(i)
    assert pairk_supported(pa, pb, xd)
    n0 = len((ctx := Ctx(DEV)).meta)
    y = run_pair2(ctx, pa, xd, pb, force=True, ksplit=True)
    assert [m["kind"] for m in ctx.meta[n0:]] == ["conv_pair"]
    _check(y, ref, two)


@pytest.mark.parametrize("i,sel", [(0, 2), (0, 3), (3, 2), (6, 3)])
def test_pair_ksplit_tile_rows(i, sel):
    """2- and 4-row tiles (convB's hint bits 26-27; the launcher's choice on maps of more than 256 one-row tiles)."""
    pa, pb, xd, ref, two = _case(i)
    th0 = EN.PAIR2_TH
    EN.PAIR2_TH = {sel: ("convA",)}
    try:
        y = run_pair2(Ctx(DEV), pa, xd, pb, force=True, ksplit=True)
    finally:
        EN.PAIR2_TH = th0
    _check(y, ref, two)


def test_pair_ksplit_auto_rows_large_map():
    """A map of more than 256 one-row tiles (2 x 50x150 outputs): the launcher's own choice of taller tiles."""
    ca, ba = _mk(2, 16, 16, 3, 2, 1, seed=101)
    cb, bb = _mk(2, 16, 16, 3, 1, 1, seed=102)
    torch.manual_seed(103)
    x = torch.randn(2, 16, 99, 299)
    ref = _ref_conv([_ref_conv([x], ca, ba, ACT_GELU)], cb, bb, ACT_GELU)
    pa, pb = pk(ca, ba, ACT_GELU), pk(cb, bb, ACT_GELU)
    ctx = Ctx(DEV)
    xd = [x.to(DEV)]
    two = run_conv(ctx, pb, [run_conv(ctx, pa, xd)])
    _check(run_pair2(ctx, pa, xd, pb, force=True, ksplit=True), ref, two)


def test_pair_ksplit_deterministic():
    """The partial tiles are summed in a fixed order: two runs on the same inputs are bitwise equal."""
    pa, pb, xd, _, _ = _case(4)
    ctx = Ctx(DEV)
    y0 = run_pair2(ctx, pa, xd, pb, force=True, ksplit=True).clone()
    y1 = run_pair2(ctx, pa, xd, pb, force=True, ksplit=True)
    assert torch.equal(y0, y1)


def test_pair_ksplit_in_plan():
    """Through a plan: the graph replayed twice with the inputs changed in between, against eager."""
    pa, pb, xd, _, _ = _case(3)
    x = xd[0].clone()
    plan = Ctx(DEV, plan=True)
    y = run_pair2(plan, pa, [x], pb, force=True, ksplit=True)
    eager = Ctx(DEV)
    for k in range(2):
        plan.launch(graph=True)
        torch.cuda.synchronize()
        assert torch.equal(y, run_pair2(eager, pa, [x.clone()], pb, force=True, ksplit=True)), k
        x.mul_(-0.5).add_(0.25)
    plan.close()
