"""LDS poisoning: what global memory has in tests/layouts.py, for the memory no host call can reach.

The hardware does not clear LDS between workgroups or launches, so a kernel that reads a cell it never wrote (a pad
column, the tail of a staged chunk, a channel past Cin, a halo row past a ragged edge) reads what the previous kernel
on that CU left there.  In a test that is almost always the same kernel on the same input: finite, plausible, and
invisible once it meets a zero weight.  ``fill`` makes every CU's whole LDS one chosen word first
(esm_lds_fill_u32, csrc/lds_debug.hip), and ``assert_leftover_free`` asserts a launch gives the same bits whatever
that word is.

PATTERNS: a quiet NaN (anything it touches, whatever weight or mask it meets, is NaN) and 1e30 (finite, for paths
where a max / min / select drops a NaN).  No kernel here keeps indices or addresses in LDS (the one integer array is
render.hip's colour table), so neither can become a wild address.
"""
import ctypes

import torch

from esmstereo_amd import _lib

PATTERNS = (0x7FC00000, 0x7149F2CA)
LDS_WORDS = 163840 // 4


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def fill(pattern: int) -> None:
    """Every word of every CU's LDS becomes ``pattern``, ordered on the current torch stream."""
    _lib.check(_lib.lib.esm_lds_fill_u32(pattern, _stream()), "lds_fill")


def probe(pattern: int) -> torch.Tensor:
    """[workgroups, 2] int64 on the host: per workgroup of the probe launch, the number of its 40,960 LDS words that
    differ from ``pattern`` and the identity of the CU it ran on."""
    n = _lib.check(_lib.lib.esm_lds_probe_workgroups(), "lds_probe_workgroups")
    out = torch.empty(n, 2, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.esm_lds_probe_u32(pattern, out.data_ptr(), n, _stream()), "lds_probe")
    torch.cuda.synchronize()
    return out.cpu().long() & 0xFFFFFFFF


def _tensors(outputs):
    outs = outputs() if callable(outputs) else outputs
    return [outs] if isinstance(outs, torch.Tensor) else list(outs)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def assert_leftover_free(launch, outputs, what: str = "") -> None:
    """``launch()`` enqueues only the kernel(s) under test (inputs, packed weights and output buffers are prepared
    before the first call, so nothing runs between a fill and the launch); ``outputs`` is the tensor(s) it writes, or
    a callable giving them after a launch.  One plain run, then one run per pattern behind ``fill(pattern)``: every
    output bitwise the plain run's, and finite wherever the plain run is finite."""
    launch()
    torch.cuda.synchronize()
    plain = [t.clone() for t in _tensors(outputs)]
    for pattern in PATTERNS:
        if not callable(outputs):
            for t in _tensors(outputs):
                t.zero_()  # (a launch that stored nothing would otherwise leave "the same bits")
        torch.cuda.synchronize()
        fill(pattern)
        launch()
        torch.cuda.synchronize()
        got = _tensors(outputs)
        assert len(got) == len(plain), what
        for i, (g, p) in enumerate(zip(got, plain)):
            where = f"{what} output {i} after LDS pattern {pattern:#010x}"
            if p.is_floating_point():
                bad = torch.isfinite(p) & ~torch.isfinite(g)
                assert not bool(bad.any()), f"{where}: {int(bad.sum())} values lost to LDS leftovers (not finite)"
            if not _same_bits(g, p):
                n = int((g.contiguous().view(torch.uint8) != p.contiguous().view(torch.uint8)).sum())
                raise AssertionError(f"{where}: {n} bytes differ from the plain run: the result depends on LDS leftovers")
