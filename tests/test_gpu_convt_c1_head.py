"""GPU tests of the single-output-channel ConvTranspose2d heads (csrc/conv_c1.h ``convt_c1_batch_kernel`` behind its
first-load record, csrc/conv_c1_rec.h) and of the two 3-D kernels that share ``C1Stage``.

Reference: fp64 ``conv_transpose2d`` / ``conv_transpose3d`` of the logical data, plus
``F.interpolate(bilinear, align_corners=False)`` of ``up`` (``test_gpu_parity._ref_conv``); tolerance 1e-5 relative,
the one ``test_gpu_parity.test_convt_c1_form`` holds these kernels to.

What selects a kernel: ``Cin`` <= 16 the ``<16>`` instantiation, else ``<32>``; 64-column tiles (``QW`` = 4, one
16-byte store per thread, the taps of ``up`` loaded once per thread) from 256 workgroups of 16 x 64 outputs on,
32-column tiles (``QW`` = 2) below; the compiled epilogue for no BN scale / activation / ``mul`` / ``res`` with ``up``
at factor 2 or 4, the general one for everything else.
"""
import pytest
import torch

from layouts import assert_guards_intact, embed, guard_snapshot
from lds_poison import assert_leftover_free
from test_gpu_parity import _mk, _ref_conv, pk, rel

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

from esmstereo_amd._lib import HINT_C1T  # noqa: E402
from esmstereo_amd._lib import HINT_ROWS as ROWS  # noqa: E402
from esmstereo_amd.engine import ACT_GELU, ACT_NONE, Ctx, run_conv  # noqa: E402

DEV = torch.device("cuda")
TOL = 1e-5

SMALL_MAPS = [(3, 5), (8, 32), (9, 33), (17, 47)]    # QW = 2: odd extents, one tile, rows / columns ending inside a tile
BIG_MAPS = [(2, 64, 512), (3, 60, 350)]              # QW = 4: 8 x 16 tiles; Ho 120 / Wo 700 end inside tiles


def _workgroups64(B, Hi, Wi):
    return -(-2 * Wi // 64) * -(-2 * Hi // 16) * B


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _close(y, ref, what):
    assert bool(torch.isfinite(y).all()), what
    assert rel(y, ref) < TOL, what


@pytest.mark.parametrize("cin", [1, 5, 16, 17, 32])
def test_channels_on_small_maps(cin):
    """Both channel instantiations on the 32-column tiles, plain epilogue (bias only)."""
    conv, _ = _mk(2, cin, 1, 4, 2, 1, transposed=True, bias=True, bn=False, seed=cin)
    p = pk(conv, None, ACT_NONE)
    for Hi, Wi in SMALL_MAPS:
        assert _workgroups64(1, Hi, Wi) < 256
        x = _randn(1, cin, Hi, Wi, seed=Hi * Wi)
        _close(run_conv(Ctx(DEV), p, [x.to(DEV)]), _ref_conv([x], conv, None, ACT_NONE), f"Cin {cin} {Hi}x{Wi}")


@pytest.mark.parametrize("cin", [5, 17])
@pytest.mark.parametrize("B,Hi,Wi", BIG_MAPS)
def test_epilogues_on_wide_tiles(B, Hi, Wi, cin):
    """The 64-column tiles: plain; ``up`` at factor 2 and 4 with ``post_scale`` 4 (the compiled epilogue), the same
    with ``out2``; ``res``, ``mul`` and BN + GELU (the general epilogue)."""
    assert _workgroups64(B, Hi, Wi) >= 256
    conv, _ = _mk(2, cin, 1, 4, 2, 1, transposed=True, bias=True, bn=False, seed=3)
    p = pk(conv, None, ACT_NONE)
    x = _randn(B, cin, Hi, Wi, seed=1)
    xd = x.to(DEV)
    Ho, Wo = 2 * Hi, 2 * Wi
    _close(run_conv(Ctx(DEV), p, [xd]), _ref_conv([x], conv, None, ACT_NONE), "plain")
    for f in (2, 4):
        up = _randn(B, 1, Ho // f, Wo // f, seed=f)
        ref = _ref_conv([x], conv, None, ACT_NONE, up=up, up_f=f)
        _close(run_conv(Ctx(DEV), p, [xd], up=up.to(DEV), up_f=f, post_scale=4.0), ref * 4, f"up x{f}")
        cp = torch.zeros(B, 1, Ho, Wo, device=DEV)
        y = run_conv(Ctx(DEV), p, [xd], up=up.to(DEV), up_f=f, post_scale=4.0, out2=cp, post_scale2=0.5)
        _close(y, ref * 4, f"up x{f} out2: out")
        _close(cp, ref * 0.5, f"up x{f} out2: out2")
    res, mul = _randn(B, 1, Ho, Wo, seed=7), torch.rand(B, 1, Ho, Wo, generator=torch.Generator().manual_seed(8)) + 0.5
    _close(run_conv(Ctx(DEV), p, [xd], res=res.to(DEV)), _ref_conv([x], conv, None, ACT_NONE, res=res), "res")
    _close(run_conv(Ctx(DEV), p, [xd], mul=mul.to(DEV)), _ref_conv([x], conv, None, ACT_NONE, mul=mul), "mul")
    up = _randn(B, 1, Hi, Wi, seed=9)  # the general epilogue with every operand at once
    _close(run_conv(Ctx(DEV), p, [xd], mul=mul.to(DEV), res=res.to(DEV), up=up.to(DEV), up_f=2),
           _ref_conv([x], conv, None, ACT_NONE, mul=mul, res=res, up=up, up_f=2), "mul res up")
    cbn, bn = _mk(2, cin, 1, 4, 2, 1, transposed=True, bn=True, seed=4)
    _close(run_conv(Ctx(DEV), pk(cbn, bn, ACT_GELU), [xd]), _ref_conv([x], cbn, bn, ACT_GELU), "BN + GELU")
    _close(run_conv(Ctx(DEV), pk(cbn, bn, ACT_GELU), [xd], up=up.to(DEV), up_f=2),
           _ref_conv([x], cbn, bn, ACT_GELU, up=up, up_f=2), "BN + GELU + up")


@pytest.mark.parametrize("f", [2, 4])
@pytest.mark.parametrize("uh,uw", [(1, 1), (2, 3)])
def test_tap_border_clamps(uh, uw, f):
    """An ``up`` of 1 x 1 and of 2 x 3: every tap is clamped at a border.  B 1 runs the 32-column tiles (taps per
    column), B 256 the 64-column tiles (taps loaded once per thread)."""
    Ho, Wo = uh * f, uw * f
    conv, _ = _mk(2, 3, 1, 4, 2, 1, transposed=True, bias=True, bn=False, seed=5)
    p = pk(conv, None, ACT_NONE)
    for B in (1, 256):
        assert (_workgroups64(B, Ho // 2, Wo // 2) >= 256) == (B == 256)
        x, up = _randn(B, 3, Ho // 2, Wo // 2, seed=B), _randn(B, 1, uh, uw, seed=B + 1)
        y = run_conv(Ctx(DEV), p, [x.to(DEV)], up=up.to(DEV), up_f=f, post_scale=4.0)
        _close(y, _ref_conv([x], conv, None, ACT_NONE, up=up, up_f=f) * 4, f"up {uh}x{uw} x{f} B {B}")


@pytest.mark.parametrize("B,cin,Hi,Wi", [(1, 5, 9, 33), (1, 17, 17, 47), (3, 5, 60, 350)])
def test_odd_strided_views(B, cin, Hi, Wi):
    """Source, output, ``out2`` and ``up`` as odd-strided views (4-byte aligned base, odd row stride) inside
    allocations full of a NaN sentinel: finite and within tolerance, and every cell around ``out`` / ``out2`` intact."""
    conv, _ = _mk(2, cin, 1, 4, 2, 1, transposed=True, bias=True, bn=False, seed=6)
    p = pk(conv, None, ACT_NONE)
    x, up = _randn(B, cin, Hi, Wi, seed=2), _randn(B, 1, Hi, Wi, seed=3)
    ref = _ref_conv([x], conv, None, ACT_NONE, up=up, up_f=2)
    zero = torch.zeros(B, 1, 2 * Hi, 2 * Wi)
    out, out2 = embed(zero, "odd", DEV), embed(zero, "odd", DEV)
    assert out.stride() == out2.stride()
    snaps = [guard_snapshot(out), guard_snapshot(out2)]
    run_conv(Ctx(DEV), p, [embed(x, "odd", DEV)], out, up=embed(up, "odd", DEV), up_f=2, post_scale=4.0, out2=out2,
             post_scale2=1.0)
    torch.cuda.synchronize()
    _close(out, ref * 4, "out")
    _close(out2, ref, "out2")
    assert_guards_intact(out, snaps[0], "out")
    assert_guards_intact(out2, snaps[1], "out2")
    # without out2 and on a 16-byte aligned placement: the vector store's surroundings
    out = embed(zero, "gapped16", DEV)
    snap = guard_snapshot(out)
    run_conv(Ctx(DEV), p, [embed(x, "gapped16", DEV)], out, up=embed(up, "gapped16", DEV), up_f=2, post_scale=4.0)
    torch.cuda.synchronize()
    _close(out, ref * 4, "out (gapped16)")
    assert_guards_intact(out, snap, "out (gapped16)")


@pytest.mark.parametrize("cin", [5, 17])
def test_lds_leftovers(cin):
    """Each instantiation on poisoned LDS (tests/lds_poison.py): channels past Cin, the pad columns and the slots past
    a channel plane must not reach a result.  Both tile widths."""
    conv, _ = _mk(2, cin, 1, 4, 2, 1, transposed=True, bias=True, bn=False, seed=7)
    p = pk(conv, None, ACT_NONE)
    for B, Hi, Wi in [(1, 9, 33), (3, 60, 350)]:
        x, up = _randn(B, cin, Hi, Wi, seed=4).to(DEV), _randn(B, 1, Hi, Wi, seed=5).to(DEV)
        out = torch.zeros(B, 1, 2 * Hi, 2 * Wi, device=DEV)
        ctx = Ctx(DEV)
        assert_leftover_free(lambda: run_conv(ctx, p, [x], out, up=up, up_f=2, post_scale=4.0), [out],
                             f"Cin {cin} {Hi}x{Wi}")


def test_3d_siblings():
    """The 3-D kernels on the shared staging plan: the register-blocked form at 6 x 12 x 39 -> 12 x 24 x 78 with Cin 12
    (S-K's aggregation head) and the per-class form (ROWS(1)), both against fp64."""
    conv, _ = _mk(3, 12, 1, 4, 2, 1, transposed=True, bias=True, bn=False, seed=8)
    p = pk(conv, None, ACT_NONE)
    x = _randn(1, 12, 6, 12, 39, seed=6)
    ref = _ref_conv([x], conv, None, ACT_NONE)
    _close(run_conv(Ctx(DEV), p, [x.to(DEV)]), ref, "blocked")
    _close(run_conv(Ctx(DEV), p, [x.to(DEV)], hint=HINT_C1T | ROWS(1)), ref, "per class")
