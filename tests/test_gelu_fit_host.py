"""The one-branch GELU of the conv epilogues (csrc/common.h gelu_erf), checked on the CPU from the constants in the
header itself (no GPU, no build).

    g(x) = x * (x < 0 ? e : 1 - e),   e = exp2(s(t)),   t = |x| / sqrt 2,   s = t q(t) - 1 ~ log2(1/2 erfc(t))

The Horner chain is read out of common.h and evaluated in fp32 the way the kernel does: every fused multiply-add as
an fp64 product-sum rounded once to fp32 (the product of two fp32 values is exact in fp64), v_exp_f32 as the fp64
exp2 rounded to fp32, results below the normal range flushed to zero.  The instruction is accurate to 1 ulp, so every
check runs three times, with the exponential exact and multiplied by (1 +- 2^-23).

Bound: |g(x) - GELU(x)| <= 0.8 * (2.5e-7 |x| + 1e-37) against the fp64 x/2 erfc(-x / sqrt 2): the bound of
tests/test_gpu_parity.py::test_gelu_epilogue_branch_free_erf with a fifth kept back for what the emulation does not
model of the hardware's rounding.
"""
import math
import os
import re

import numpy as np
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "esmstereo_amd", "csrc", "common.h")
F32 = np.float32
T_FIT = 4.2  # end of the fit range in t (scripts/fit_gelu.py --top)
_LIT = r"-?(?:0x[0-9a-f.]+p[+-]?\d+|\d+\.\d*)f"


def _constants():
    """(1 / sqrt 2 as the kernel has it, [c_N, ..., c_1, -1]: the chain's constants in evaluation order)."""
    with open(HEADER) as f:
        src = f.read()
    body = src[src.index("#ifndef ESM_GELU_TWO_BRANCH"):]
    body = body[:body.index("#else")]
    val = lambda s: F32(float.fromhex(s[:-1]) if "0x" in s else float(s[:-1]))  # noqa: E731
    m = re.search(rf"const float t = fabsf\(x\) \* ({_LIT});", body)
    assert m, "the scale of t"
    first = re.search(rf"float s = fmaf\(t, ({_LIT}), ({_LIT})\);", body)
    assert first, "the head of the Horner chain"
    rest = re.findall(rf"\n\s*s = fmaf\(t, s, ({_LIT})\);", body)
    chain = [val(first.group(1)), val(first.group(2))] + [val(c) for c in rest]
    assert "__builtin_amdgcn_exp2f(s)" in body and "x * (x < 0.0f ? e : 1.0f - e)" in body
    return val(m.group(1)), chain


RSQRT2, CHAIN = _constants()


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(F32)


def exponent(t):
    p = np.full(t.shape, CHAIN[0], dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in CHAIN[1:]:
            p = fma(t, p, c)
    return p


def gelu32(x, ulp):
    """The kernel's g(x) in emulated fp32; `ulp` in (0, 1, -1) moves the exponential by that many units."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        e = np.exp2(exponent(np.abs(x) * RSQRT2).astype(np.float64)).astype(F32)
        e = np.where(e < np.finfo(F32).tiny, F32(0), e)
        e = (e.astype(np.float64) * (1.0 + ulp * 2.0 ** -23)).astype(F32)
        return (x * np.where(x < 0, e, F32(1) - e)).astype(F32)


def gelu64(x):
    x = torch.from_numpy(np.asarray(x, dtype=np.float64))
    return (x * 0.5 * torch.erfc(-x / math.sqrt(2.0))).numpy()  # no cancellation on either side


def parity_grid():
    """The inputs of test_gelu_epilogue_branch_free_erf."""
    return torch.cat([torch.linspace(-12, 12, 200001), torch.linspace(1.40, 1.43, 20001),
                      torch.linspace(-1.43, -1.40, 20001), torch.tensor([0.0, -0.0, 1e-30, -1e-30])]).numpy()


def dense_grid():
    """Every 16th fp32 value of +-[2^-4, 16)."""
    pos = np.arange(np.array(2.0 ** -4, F32).view(np.uint32), np.array(16.0, F32).view(np.uint32), 16,
                    dtype=np.uint32).view(F32)
    return np.concatenate([pos, -pos])


def log_sweep():
    """Log-spaced from the smallest denormal to FLT_MAX, both signs."""
    fi = np.finfo(F32)
    pos = np.concatenate([np.logspace(math.log10(1.5e-45), math.log10(float(fi.max)), 8000).astype(F32),
                          np.array([fi.smallest_subnormal, fi.tiny, fi.max], dtype=F32)])
    assert pos[0] > 0 and np.isfinite(pos).all() and (pos < fi.tiny).sum() > 100
    return np.concatenate([pos, -pos])


def worst_ratio(x):
    ref = gelu64(x)
    lim = 2.5e-7 * np.abs(x.astype(np.float64)) + 1e-37
    out = {}
    for ulp in (0, 1, -1):
        q = np.abs(gelu32(x, ulp).astype(np.float64) - ref) / lim
        i = int(np.argmax(q))
        out[ulp] = (float(q[i]), float(x[i]))
    return out


def test_constants_are_the_fit():
    """Degree 8 (8 fused multiply-adds), s(0) = -1 exactly, 1 / sqrt 2 rounded to fp32."""
    assert len(CHAIN) == 9 and CHAIN[-1] == F32(-1.0)
    assert RSQRT2 == F32(math.sqrt(0.5))
    assert exponent(np.zeros(1, F32))[0] == F32(-1.0)


def test_error_bound_dense():
    for name, x in (("dense", dense_grid()), ("sweep", log_sweep()), ("parity grid", parity_grid())):
        w = worst_ratio(x)
        print(f"{name}: worst |error| / (2.5e-7 |x| + 1e-37) = " +
              ", ".join(f"{w[u][0]:.3f} at {w[u][1]!r} (exp {u:+d} ulp)" for u in (0, 1, -1)))
        for u in (0, 1, -1):
            assert w[u][0] <= 0.8, (name, u, w[u])


def test_special_values():
    inf, nan = F32(np.inf), F32(np.nan)
    for ulp in (0, 1, -1):
        z = gelu32(np.array([0.0, -0.0], F32), ulp)
        assert z[0] == 0 and z[1] == 0 and not np.signbit(z[0]) and np.signbit(z[1])
        assert gelu32(np.array([inf], F32), ulp)[0] == inf
        assert np.isnan(gelu32(np.array([nan], F32), ulp)[0])
        # -inf: -inf * 0 = NaN, as x * 0.5 * (1 + erf(-inf)) = -inf * 0 of the two-branch form
        assert np.isnan(gelu32(np.array([-inf], F32), ulp)[0])
        # x <= -6, however large: -0 or a value no larger than |GELU(-6)| = 5.92e-9 (|x| Phi(x) falls from there on):
        # no clamp of the exponent may leave a visible value behind
        big = -np.concatenate([np.logspace(math.log10(6.0), math.log10(float(np.finfo(F32).max)), 4000).astype(F32),
                               np.array([6.0, 1e6, np.finfo(F32).max], F32)])
        g = gelu32(big, ulp)
        assert np.isfinite(g).all() and (g <= 0).all() and float(np.abs(g).max()) <= 6.0e-9
        assert (np.abs(g.astype(np.float64) - gelu64(big)) <= 2.5e-7 * np.abs(big.astype(np.float64))).all()
        assert gelu32(np.array([-1e6], F32), ulp)[0] == 0 and np.signbit(gelu32(np.array([-1e6], F32), ulp)[0])


def test_exponent_tail_needs_no_clamp():
    """s(t) <= -29 (exp2 < 2e-9) and not NaN from the end of the fit range to +inf: every 251st fp32 value of
    [4.2, +inf), every value of the first binade's start, FLT_MAX and +inf."""
    lo = int(np.array(T_FIT, F32).view(np.uint32))
    hi = int(np.array(np.inf, F32).view(np.uint32))
    t = np.concatenate([np.arange(lo, hi, 251, dtype=np.uint32).view(F32),
                        np.arange(lo, lo + 100000, dtype=np.uint32).view(F32),
                        np.array([np.finfo(F32).max, np.inf], F32)])
    s = exponent(t)
    assert not np.isnan(s).any()
    assert float(s.max()) <= -29.0, float(s.max())
    assert s[-1] == -np.inf
