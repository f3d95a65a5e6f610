#!/usr/bin/env python3
"""Derive the constants of the one-branch GELU in esmstereo_amd/csrc/common.h (gelu_erf).

GELU(x) = x Phi(x).  With t = |x| / sqrt 2:  Phi(x) = 1/2 erfc(t) for x < 0 and 1 - 1/2 erfc(t) for x >= 0, and
1/2 erfc(t) = exp2(s(t)) with s(t) = log2 erfc(t) - 1 = t q(t) - 1 (s(0) = -1 exactly: the constant is not fitted).
This script fits q (degree N - 1, so s has degree N) on [0, T]:

  * the error that counts is the one of Phi, d Phi = ln 2 * exp2(s) * d s, so the fit is a weighted minimax of d s
    with the weight ln 2 * 1/2 erfc(t), by Lawson's iteratively reweighted least squares on a Chebyshev grid;
  * the fp64 coefficients are rounded to fp32 and the whole GELU is then evaluated the way the kernel does, in fp32
    with fused multiply-adds (an fp64 product-sum rounded once), over a dense grid, against the fp64 x/2 erfc(-x/sqrt 2);
  * the exponent of the tail (t > T up to +inf) is checked to stay below -29 (exp2 < 2e-9: Phi = 0 or 1 within
    2^-28) and never NaN, so the kernel needs no clamp.

It prints the fp32 constants as hex floats (the lines of common.h) and the worst |error| / (2.5e-7 |x|), the bound of
tests/test_gpu_parity.py::test_gelu_epilogue_branch_free_erf.  numpy and the standard library only.

    python scripts/fit_gelu.py [--degree 8] [--top 4.2]
"""
from __future__ import annotations

import argparse
import math

import numpy as np

F32 = np.float32
RSQRT2 = F32(0.70710678118654752440)
BOUND = 2.5e-7   # |g(x) - GELU(x)| <= BOUND |x| + FLOOR
FLOOR = 1e-37
_erfc = np.frompyfunc(math.erfc, 1, 1)


def erfc64(t):
    return _erfc(np.asarray(t, dtype=np.float64)).astype(np.float64)


def gelu64(x):
    """x Phi(x) in fp64 without cancellation on either side."""
    x = np.asarray(x, dtype=np.float64)
    return x * 0.5 * erfc64(-x / math.sqrt(2.0))


def fit(degree: int, top: float, n: int = 6000, iters: int = 400):
    """fp64 coefficients c[0..degree-1] of q(t) = c0 + c1 t + ... with log2 erfc(t) ~ t q(t) on [0, top]."""
    k = np.arange(n)
    t = 0.5 * top * (1.0 - np.cos(math.pi * (k + 0.5) / n))  # Chebyshev nodes of [0, top]
    erfc = erfc64(t)
    y = np.log2(erfc)
    w = math.log(2.0) * 0.5 * erfc                           # d Phi / d s
    A = np.stack([t ** (j + 1) for j in range(degree)], axis=1)
    u = np.ones(n)
    best, best_c = np.inf, None
    for _ in range(iters):
        sw = np.sqrt(u) * w
        c, *_ = np.linalg.lstsq(A * sw[:, None], y * sw, rcond=None)
        r = np.abs(w * (A @ c - y))
        if r.max() < best:
            best, best_c = r.max(), c
        u = u * r
        u /= u.sum()
    return best_c, best


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def exponent32(t, c32):
    """s(t) as the kernel's Horner chain: `degree` fused multiply-adds, the last one with the constant -1."""
    p = np.full(t.shape, c32[-1], dtype=F32)
    for c in c32[-2::-1]:
        p = fma(t, p, c)
    return fma(t, p, F32(-1.0))


def exp2_32(s, ulp=0):
    """v_exp_f32: exp2 rounded to fp32, results below the normal range flushed to 0; `ulp` = +-1 perturbs the
    result by one unit in the last place, the instruction's stated accuracy."""
    with np.errstate(under="ignore"):
        e = np.exp2(s.astype(np.float64)).astype(F32)
    e = np.where(e < np.finfo(F32).tiny, F32(0), e)
    if ulp:
        e = (e.astype(np.float64) * (1.0 + ulp * 2.0 ** -23)).astype(F32)
    return e


def gelu32(x, c32, ulp=0):
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.abs(x) * RSQRT2
        e = exp2_32(exponent32(t, c32), ulp)
        phi = np.where(x < 0, e, F32(1) - e)
        return (x * phi).astype(F32)


def grid():
    """2 M points of [-12, 12] and the windows and specials of test_gelu_epilogue_branch_free_erf."""
    return np.concatenate([
        np.linspace(-12, 12, 2000001), np.linspace(-12, 12, 200001), np.linspace(1.40, 1.43, 20001),
        np.linspace(-1.43, -1.40, 20001), [0.0, -0.0, 1e-30, -1e-30]]).astype(F32)


def worst(c32, x=None):
    x = grid() if x is None else x
    ref = gelu64(x)
    lim = BOUND * np.abs(x.astype(np.float64)) + FLOOR
    out = []
    for ulp in (0, 1, -1):
        q = np.abs(gelu32(x, c32, ulp).astype(np.float64) - ref) / lim
        i = int(np.argmax(q))
        out.append((float(q[i]), float(x[i])))
    return out


def tail_max(c32, top):
    """max of s over the fp32 values from `top` to +inf (every 64th value, and +inf)."""
    lo = int(np.array(top, dtype=F32).view(np.uint32))
    hi = int(np.array(np.inf, dtype=F32).view(np.uint32))
    t = np.arange(lo, hi + 1, 64, dtype=np.uint32).view(F32)
    t = np.concatenate([t, np.array([np.inf], dtype=F32)])
    with np.errstate(over="ignore", invalid="ignore"):
        s = exponent32(t, c32)
    return float(np.max(s)), bool(np.isnan(s).any())


def hexf(c) -> str:
    """fp32 value as a C++17 hex-float literal, e.g. -0x1.a0be9ep+0f"""
    m, e = float(c).hex().split("p")
    return f"{m.rstrip('0')}p{e}f"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--degree", type=int, default=8, help="degree of s(t) = t q(t) - 1")
    ap.add_argument("--top", type=float, default=4.2, help="end of the fit range in t = |x| / sqrt 2")
    a = ap.parse_args()
    c64, fit_err = fit(a.degree, a.top)
    c32 = c64.astype(F32)
    print(f"degree {a.degree}, fit on [0, {a.top}]: weighted minimax error of Phi {fit_err:.3e} (fp64 coefficients)")
    print("constants (s = t (c1 + t (c2 + ...)) - 1, base 2):")
    for j, c in enumerate(c32):
        print(f"    c{j + 1} = {hexf(c):>16}   // {float(c): .9e}")
    for name, (q, at) in zip(("v_exp_f32 exact", "v_exp_f32 +1 ulp", "v_exp_f32 -1 ulp"), worst(c32)):
        print(f"worst |error| / (2.5e-7 |x| + 1e-37), {name:>16}: {q:.3f} at x = {at!r}")
    smax, nan = tail_max(c32, a.top)
    print(f"tail: max s(t) for t in [{a.top}, +inf] = {smax:.2f}, NaN: {nan}")


if __name__ == "__main__":
    main()
