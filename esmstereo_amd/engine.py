"""Host side of the HIP hot path: weight packing, launch descriptors, eager/plan contexts.

Every op here goes to ``libesmstereo_amd.so`` through ``_lib`` (ctypes over the C ABI of
``include/esmstereo_amd.h``).  Nothing computes on the CPU and there is no PyTorch
fallback: CPU tensors, non-fp32 tensors or a missing library raise.

A :class:`Ctx` either launches each op immediately on the current torch stream (``eager``)
or appends it to a native ``esm_plan`` (``plan``) whose launch list is later replayed —
eagerly or as one hipGraph.  The module classes (blocks.py, mixer.py, model.py) describe the
reference's forward passes once, against a Ctx, so the eager nn.Module forward and the
compiled whole-hot-path plan run the very same kernels with the very same fusions.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
import threading
import dataclasses
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SIGMOID, ACT_SILU, EsmConfDesc, EsmConvDesc, EsmShuffleConvDesc,
                   EsmShuffleTailDesc, EsmSmixDesc, HINT_GWC_STEM_WLDS, HINT_PAIR_NO_RECORD, HINT_PAIR_REGRESS, HINT_PAIRK,
                   HINT_ROWS, HINT_ROWS_MASK, HINT_SMALL, HINT_SMALL_NO_RECORD, HINT_SMALL_NO_ZSPLIT, HINT_TILE, HINT_XCD_SLAB, check, lib)

__all__ = ["Ctx", "PackedConv", "pack_conv", "run_conv", "run_smix", "run_fmnet", "run_shuffle_tail", "pack_shuffle_tail",
           "ACT_NONE", "ACT_GELU", "ACT_SILU", "ACT_RELU", "ACT_SIGMOID", "ACT_RELU6", "run_dwconv", "cached_pack", "run_convt_1x1",
           "convt_1x1_supported"]


def _rup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# Dry emission (Ctx(dry=True)): the launch list is walked with shape-only ``meta`` tensors, nothing is
# submitted and no device memory is touched.  It sizes a plan's arena before the real emission and
# lets CPU tests read every op's algorithmic cost (ctx.meta).  While one is active IN THIS THREAD, meta
# tensors pass the device checks below; they can never reach a kernel, because a dry Ctx submits nothing.
# The depth is thread-local: a dry emission in one thread never relaxes another thread's eager checks
# (ADVICE r4).
_DRY = threading.local()


def _dry_depth() -> int:
    return getattr(_DRY, "depth", 0)


def require_device(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor")
    if t.device.type == "meta" and _dry_depth():
        return
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: esmstereo_amd runs on ROCm devices only (got a {t.device.type} tensor); "
                           "there is no CPU path")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32, got {t.dtype}")
    if t.dim() > 0 and t.stride(-1) != 1:
        raise ValueError(f"{what}: innermost dimension must be contiguous")


def require_on(dev: torch.device, what: str, *ts: Optional[torch.Tensor]) -> None:
    """Every pointer a kernel dereferences must live on the launch device (a host or
    other-device pointer would fault the GPU, so this is checked on the host first)."""
    dry = _dry_depth()
    for t in ts:
        if t is None:
            continue
        if dry and (t.device.type == "meta" or torch.device(dev).type == "meta"):
            continue  # a dry emission submits nothing (its buffers are shape-only)
        if t.device != dev or t.dtype != torch.float32:
            raise RuntimeError(f"{what}: tensor on {t.device} ({t.dtype}); expected float32 on {dev} "
                               "(move the module to the input's device)")


# ----------------------------------------------------------------------------- packing


@dataclass
class PackedConv:
    """A conv layer ready for ``esm_conv_f32``: packed weights + folded BN/bias epilogue."""

    w: torch.Tensor
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    act: int
    nd: int
    k: int
    stride: int
    pad: int
    transposed: bool
    cin: int
    cout: int
    cin_pad: int
    cout_pad: int


def _bits(v: int, n: int) -> Tuple[int, ...]:
    return tuple((v >> (n - 1 - i)) & 1 for i in range(n))


def pack_weight(W: torch.Tensor, transposed: bool) -> Tuple[torch.Tensor, int, int]:
    """Pack a Conv/ConvTranspose weight for the implicit-GEMM kernel.

    normal      W[cout][cin][k..]  -> P[tap][cin_pad][cout_pad]
    transposed  W[cin][cout][4..]  -> P[cls][tap][cin_pad][cout_pad]; for output parity q and
                tap t of a dim the kernel index is 1 - q + 2t (input index m + q - t).
    """
    W = W.detach().to(torch.float32)
    nd = W.dim() - 2
    if not transposed:
        cout, cin = W.shape[:2]
        taps = int(W[0, 0].numel())
        cin_pad, cout_pad = _rup(cin, 16), _rup(cout, 32)
        P = W.new_zeros(taps, cin_pad, cout_pad)
        P[:, :cin, :cout] = W.reshape(cout, cin, taps).permute(2, 1, 0)
        return P.contiguous(), cin_pad, cout_pad
    cin, cout = W.shape[:2]
    if any(s != 4 for s in W.shape[2:]):
        raise ValueError("transposed conv: only kernel 4 is supported")
    cin_pad, cout_pad = _rup(cin, 16), _rup(cout, 32)
    n = 2 ** nd
    P = W.new_zeros(n, n, cin_pad, cout_pad)
    for cls in range(n):
        q = _bits(cls, nd)
        for tap in range(n):
            t = _bits(tap, nd)
            k = tuple(1 - qi + 2 * ti for qi, ti in zip(q, t))
            P[cls, tap, :cin, :cout] = W[(slice(None), slice(None)) + k]
    return P.contiguous(), cin_pad, cout_pad


def bn_affine(bn: torch.nn.Module) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval BatchNorm as y = x*alpha + beta with alpha = w/sqrt(var+eps), beta = b - mean*alpha."""
    invstd = 1.0 / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    alpha = invstd * bn.weight.detach().float()
    beta = bn.bias.detach().float() - bn.running_mean.detach().float() * alpha
    return alpha.contiguous(), beta.contiguous()


def pack_conv(conv: torch.nn.Module, bn: Optional[torch.nn.Module] = None, act: int = ACT_NONE) -> PackedConv:
    transposed = isinstance(conv, (torch.nn.ConvTranspose2d, torch.nn.ConvTranspose3d))
    W = conv.weight
    nd = W.dim() - 2
    ks = set(conv.kernel_size)
    ss = set(conv.stride)
    ps = set(conv.padding) if not isinstance(conv.padding, str) else {-1}
    if len(ks) != 1 or len(ss) != 1 or len(ps) != 1 or set(conv.dilation) != {1} or conv.groups != 1:
        raise ValueError(f"unsupported conv geometry {conv}")
    P, cin_pad, cout_pad = pack_weight(W, transposed)
    scale = shift = None
    if bn is not None:
        scale, shift = bn_affine(bn)
        if conv.bias is not None:  # conv bias feeds BN: (x + cb)*a + b = x*a + (cb*a + b)
            shift = (conv.bias.detach().float() * scale + shift).contiguous()
    elif conv.bias is not None:
        shift = conv.bias.detach().float().contiguous()
    cin, cout = (W.shape[0], W.shape[1]) if transposed else (W.shape[1], W.shape[0])
    if shift is not None:
        # one buffer [packed weights | scale | shift], cout_pad floats each: the lean form's record kernels read the BN
        # constants through the weight pointer (csrc/conv_lean_rec.h); every other reader takes the three pointers
        n = P.numel()
        buf = P.new_zeros(n + 2 * cout_pad)
        buf[:n] = P.reshape(-1)
        buf[n + cout_pad:n + cout_pad + cout] = shift
        P, shift = buf[:n].view(P.shape), buf[n + cout_pad:n + cout_pad + cout]
        if scale is not None:
            buf[n:n + cout] = scale
            scale = buf[n:n + cout]
    return PackedConv(P, scale, shift, act, nd, ks.pop(), ss.pop(), ps.pop(), transposed, int(cin), int(cout),
                      cin_pad, cout_pad)


def cached_pack(owner: torch.nn.Module, name: str, mods: Sequence[Optional[torch.nn.Module]], build, *extra):
    """``build()`` (packed weights of ``mods``) cached on ``owner`` under ``name`` until a tensor of ``mods`` is
    replaced, moved or edited in place (param_token)."""
    tok = param_token(*mods) + tuple(extra)
    packs = owner.__dict__.setdefault("_esm_packs", {})
    c = packs.get(name)
    if c is None or c[0] != tok:
        c = packs[name] = (tok, build())
    return c[1]


def param_token(*mods: torch.nn.Module) -> Tuple:
    """Cheap identity of a module's own tensors (storage + in-place version)."""
    tok = []
    for m in mods:
        if m is None:
            continue
        for t in list(m.parameters(recurse=False)) + list(m.buffers(recurse=False)):
            tok.append((t.data_ptr(), t._version, t.device.index))
    return tuple(tok)


# ----------------------------------------------------------------------------- context


def _spans(*ts) -> List[Tuple[int, int]]:
    """(base address, bytes) of the allocations behind tensors: the unit the plan's
    dependency analysis works in (a view depends on its whole allocation)."""
    out = []
    for t in ts:
        if t is not None:
            st = t.untyped_storage()
            out.append((st.data_ptr(), st.nbytes()))
    return out


class Ctx:
    """Where ops go: launched now (``plan=False``), appended to a native plan (``plan=True``), or
    only recorded (``dry=True``: shape-only ``meta`` buffers, nothing submitted; use as a context
    manager, ``with Ctx(dev, dry=True) as ctx: ...``)."""

    def __init__(self, device: torch.device, plan: bool = False, dry: bool = False):
        self.device = torch.device(device)
        self.dry = bool(dry)
        self.plan = lib.esm_plan_create() if plan and not dry else None
        if plan and not dry and not self.plan:
            raise RuntimeError("esm_plan_create failed")
        self.keep: List[object] = []  # tensors (and ctypes descs) that must outlive the plan
        # one entry per launch-list op: name, kernel family, algorithmic flops / HBM bytes
        self.meta: List[dict] = []
        self.stream = None if (plan or dry) else ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._arena: Optional[torch.Tensor] = None
        self._arena_off = 0
        self.arena_bytes = 0   # bytes carved out of the arena (256-B granules)
        self.arena_chunks = 0
        self.num_ops = 0       # ops submitted (or, dry, recorded)

    def __enter__(self) -> "Ctx":
        if self.dry:
            _DRY.depth = _dry_depth() + 1
        return self

    def __exit__(self, *exc) -> None:
        if self.dry:
            _DRY.depth = _dry_depth() - 1

    def _submit(self) -> bool:
        """Count one op; True when it is to be handed to the library (not a dry emission)."""
        self.num_ops += 1
        if self.dry and not _dry_depth():
            raise RuntimeError("a dry Ctx must be used as a context manager")
        return not self.dry

    def launch(self, graph: bool = True, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Run a plan context's launch list (as a hipGraph by default) on the current stream."""
        if not self.plan:
            raise RuntimeError("launch() needs a plan context")
        s = ctypes.c_void_p((stream or torch.cuda.current_stream(self.device)).cuda_stream)
        if graph:
            if not getattr(self, "_graph_ready", False):
                check(lib.esm_plan_graph_build(self.plan, s), "graph_build")
                self._graph_ready = True
            check(lib.esm_plan_graph_launch(self.plan, s), "graph_launch")
        else:
            check(lib.esm_plan_run(self.plan, s), "plan_run")

    def close(self) -> None:
        if self.plan:
            lib.esm_plan_destroy(self.plan)
            self.plan = None
        self.keep.clear()

    def __del__(self):  # pragma: no cover - interpreter teardown order
        try:
            self.close()
        except Exception:
            pass

    ARENA_CHUNK = 256 << 20  # bytes: the largest arena chunk (every buffer of an S / M plan at KITTI size)
    ARENA_FIRST = 16 << 20   # the first chunk; each further chunk doubles, up to ARENA_CHUNK

    def empty(self, *shape: int) -> torch.Tensor:
        """A float32 buffer.  A plan's buffers are carved (256-B aligned) out of arena chunks (one
        chunk sized by a dry emission for a compiled plan; 16 MiB doubling chunks otherwise), so a
        launch list's buffers sit together and come from one allocation."""
        if self.dry:  # the plan's arena accounting, with shape-only buffers
            n = math.prod(shape)
            self.arena_bytes += (4 * n + 255) // 256 * 256
            return torch.empty(shape, device="meta", dtype=torch.float32)
        if not self.plan:
            return torch.empty(shape, device=self.device, dtype=torch.float32)
        n = math.prod(shape)
        nb = (4 * n + 255) // 256 * 256
        if self._arena is None or self._arena_off + nb > self._tail_lo():
            size = self.ARENA_FIRST if self._arena is None else min(self.ARENA_CHUNK, 2 * self._arena.numel())
            self._arena = torch.empty(max(size, nb), device=self.device, dtype=torch.uint8)
            self._arena_off = 0
            self._tail = None
            self.arena_chunks += 1
            self.keep.append(self._arena)
        t = self._arena[self._arena_off:self._arena_off + 4 * n].view(torch.float32).view(shape)
        self._arena_off += nb
        self.arena_bytes += nb
        return t

    def empty_tail(self, *shape: int) -> torch.Tensor:
        """A float32 buffer carved from the END of the current arena chunk (which must have room):
        the hot path's backbone-feature inputs go there, next to the upsampler's buffers (the last
        ones the plan allocates from the front) that they are concatenated with."""
        n = math.prod(shape)
        nb = (4 * n + 255) // 256 * 256
        if self.dry or not self.plan or self._arena is None or self._arena_off + nb > self._tail_lo():
            return self.empty(*shape)
        self._tail = self._tail_lo() - nb
        self.arena_bytes += nb
        return self._arena[self._tail:self._tail + 4 * n].view(torch.float32).view(shape)

    def _tail_lo(self) -> int:
        t = getattr(self, "_tail", None)
        return self._arena.numel() if t is None or t > self._arena.numel() else t

    def hold(self, *objs) -> None:
        if self.plan:
            self.keep.extend(o for o in objs if o is not None)

    # --- op submission
    def conv(self, d: EsmConvDesc) -> None:
        if not self._submit():
            return
        if self.plan:
            check(lib.esm_plan_add_conv(self.plan, ctypes.byref(d)), "plan_add_conv")
        else:
            check(lib.esm_conv_f32(ctypes.byref(d), self.stream), "conv")

    def smix(self, d: EsmSmixDesc) -> None:
        if not self._submit():
            return
        if self.plan:
            check(lib.esm_plan_add_smix(self.plan, ctypes.byref(d)), "plan_add_smix")
        else:
            check(lib.esm_smix_f32(ctypes.byref(d), self.stream), "smix")

    def fmnet(self, d) -> None:
        if not self._submit():
            return
        if self.plan:
            check(lib.esm_plan_add_fmnet(self.plan, ctypes.byref(d)), "plan_add_fmnet")
        else:
            check(lib.esm_fmnet_f32(ctypes.byref(d), self.stream), "fmnet")

    def shuffle_tail(self, d: EsmShuffleTailDesc) -> None:
        if not self._submit():
            return
        if self.plan:
            check(lib.esm_plan_add_shuffle_tail(self.plan, ctypes.byref(d)), "plan_add_shuffle_tail")
        else:
            check(lib.esm_shuffle_tail_f32(ctypes.byref(d), self.stream), "shuffle_tail")

    def pair2(self, a: EsmConvDesc, b: EsmConvDesc) -> None:
        if not self._submit():
            return
        if self.plan:
            check(lib.esm_plan_add_conv_pair2(self.plan, ctypes.byref(a), ctypes.byref(b)), "plan_add_conv_pair2")
        else:
            check(lib.esm_conv_pair2_f32(ctypes.byref(a), ctypes.byref(b), self.stream), "conv_pair2")

    def shuffle_conv(self, d: EsmShuffleConvDesc) -> None:
        if not self._submit():
            return
        if self.plan:
            check(lib.esm_plan_add_shuffle_conv(self.plan, ctypes.byref(d)), "plan_add_shuffle_conv")
        else:
            check(lib.esm_shuffle_conv_f32(ctypes.byref(d), self.stream), "shuffle_conv")

    def dwconv(self, d) -> None:
        if not self._submit():
            return
        if self.plan:
            raise RuntimeError("dwconv: the backbone's depthwise convs run eagerly (no plan op)")
        check(lib.esm_dwconv_f32(ctypes.byref(d), self.stream), "dwconv")

    def gwc(self, L, R, att, V, B, C, H, W, D, G) -> None:
        self.meta.append(dict(name="gwc_volume", kind="gwc", flops=2 * B * C * D * H * W,
                              bytes=4 * B * (2 * C * H * W + G * D * H * W + (G * H * W if att is not None else 0)),
                              reads=_spans(L, R, att), writes=_spans(V)))
        a = att.data_ptr() if att is not None else None
        if not self._submit():
            return
        if self.plan:
            self.hold(L, R, att, V)
            check(lib.esm_plan_add_gwc(self.plan, L.data_ptr(), R.data_ptr(), a, V.data_ptr(), B, C, H, W, D, G), "gwc")
        else:
            check(lib.esm_gwc_volume_f32(L.data_ptr(), R.data_ptr(), a, V.data_ptr(), B, C, H, W, D, G, self.stream),
                  "gwc")

    def gwc_stem(self, d: EsmConvDesc, L, R, C: int, G: int) -> None:
        if not self._submit():
            return
        if self.plan:
            self.hold(L, R)
            check(lib.esm_plan_add_gwc_stem(self.plan, ctypes.byref(d), L.data_ptr(), R.data_ptr(), C, G), "gwc_stem")
        else:
            check(lib.esm_gwc_stem_f32(ctypes.byref(d), L.data_ptr(), R.data_ptr(), C, G, self.stream), "gwc_stem")

    def concat(self, L, R, V, B, C, H, W, D) -> None:
        self.meta.append(dict(name="concat_volume", kind="concat", flops=0,
                              bytes=4 * B * (2 * C * H * W + 2 * C * D * H * W), reads=_spans(L, R), writes=_spans(V)))
        if not self._submit():
            return
        if self.plan:
            self.hold(L, R, V)
            check(lib.esm_plan_add_concat(self.plan, L.data_ptr(), R.data_ptr(), V.data_ptr(), B, C, H, W, D), "concat")
        else:
            check(lib.esm_concat_volume_f32(L.data_ptr(), R.data_ptr(), V.data_ptr(), B, C, H, W, D, self.stream),
                  "concat")

    def normcorr(self, L, R, V, work, B, C, H, W, D) -> None:
        self.meta.append(dict(name="normcorr_volume", kind="normcorr", flops=2 * B * C * D * H * W,
                              bytes=4 * B * (2 * C * H * W + D * H * W), reads=_spans(L, R), writes=_spans(V, work)))
        if not self._submit():
            return
        if self.plan:
            self.hold(L, R, V, work)
            check(lib.esm_plan_add_normcorr(self.plan, L.data_ptr(), R.data_ptr(), V.data_ptr(), work.data_ptr(), B, C,
                                            H, W, D), "normcorr")
        else:
            check(lib.esm_normcorr_volume_f32(L.data_ptr(), R.data_ptr(), V.data_ptr(), work.data_ptr(), B, C, H, W, D,
                                              self.stream), "normcorr")

    def conf(self, op: int, xs: Sequence[Optional[torch.Tensor]], out: torch.Tensor, B: int, C: int, D: int, H: int,
             W: int, name: str = "conf") -> None:
        """One per-pixel stage of the confidence head (esm_conf_f32; contiguous NCHW operands)."""
        for t in list(xs) + [out]:
            if t is not None and not t.is_contiguous():
                raise ValueError(f"{name}: confidence-head operands must be contiguous")
        d = EsmConfDesc()
        d.op, d.B, d.C, d.D, d.H, d.W = op, B, C, D, H, W
        for i, t in enumerate(xs):
            d.x[i] = t.data_ptr() if t is not None else None
        d.out = out.data_ptr()
        nbytes = 4 * (sum(t.numel() for t in xs if t is not None) + out.numel())
        self.meta.append(dict(name=name, kind="conf", flops=0, bytes=nbytes, reads=_spans(*xs), writes=_spans(out)))
        if not self._submit():
            return
        if self.plan:
            self.hold(*xs, out)
            check(lib.esm_plan_add_conf(self.plan, ctypes.byref(d)), name)
        else:
            check(lib.esm_conf_f32(ctypes.byref(d), self.stream), name)

    def regression(self, kind, cost, out, B, D, H, W, samples=None, k: int = 2) -> None:
        """kind 0: disparity_regression; kind 1: regression_topk with ``k`` (2 in the hot path)."""
        name = "disparity_regression" if kind == 0 else f"regression_topk{k}"
        self.meta.append(dict(name=name, kind="regression", flops=2 * B * D * H * W, bytes=4 * B * (D + 1) * H * W,
                              reads=_spans(cost, samples), writes=_spans(out)))
        if not self._submit():
            return
        if self.plan:
            if samples is not None or (kind and k != 2):
                raise ValueError("plan regression: disparity_regression or regression_topk(k=2) over arange(D)")
            self.hold(cost, out)
            check(lib.esm_plan_add_regression(self.plan, kind, cost.data_ptr(), out.data_ptr(), B, D, H, W),
                  "regression")
        elif kind == 0:
            check(lib.esm_disp_regression_f32(cost.data_ptr(), out.data_ptr(), B, D, H, W, self.stream), "regression")
        else:
            s = samples.data_ptr() if samples is not None else None
            check(lib.esm_topk_regression_f32(cost.data_ptr(), s, out.data_ptr(), B, D, H, W, int(k), self.stream),
                  "regression_topk")


def eager_emit(device: torch.device, fn, *args, **kw):
    """Run ``fn(ctx, *args, **kw)`` (a module's ``emit``) eagerly: every launch is submitted on the
    current stream as it is emitted, its buffers from PyTorch's allocator."""
    return fn(Ctx(device), *args, **kw)


# ----------------------------------------------------------------------------- ops


# A/B switches.  The kernel-selection knobs below are read from the environment only when ESM_AB=1 (the
# measurement scripts set it); otherwise every knob takes its measured default, so a caller's environment
# can never select a combination of forms the GPU suite did not run.
AB = os.environ.get("ESM_AB") == "1"


def _ab(name: str, default: str) -> str:
    return os.environ.get(name, default) if AB else default


# Measured tile choices (scripts/autotune.py on MI355X, in the hot path's own launch sequence):
# XCD-slab tile order (HINT_XCD_SLAB, esm_shuffle_tail_desc.flags bit 0; common.h xcd_block)
# for launches whose input or output map (B x D x H x W) has at least this many pixels: there it takes
# the memory-side bytes of the full-resolution convs from 2.1-2.9x the algorithmic to 1.05-1.13x at no
# cost in step time, while on the hourglasses' small maps it measured 0.1-1 us slower per launch
# (round 3, S-K, rocprofv3 op maps; every launch remapped: +10 us on the S-K step).
XCD_SLAB_MIN_PIX = int(_ab("ESM_XCD_SLAB_MIN_PIX", "65536"))
# the same order on 3-D volumes (B x D x H x W output or input voxels over the threshold); ESM_XCD_SLAB_3D=0
# leaves every 3-D launch in the default order (A/B measurements)
XCD_SLAB_3D = _ab("ESM_XCD_SLAB_3D", "1") != "0"
# 3-D launches with >= 32 input channels from this many output voxels: the S / M `group_stem` (12x24x78),
# whose 32-channel input each workgroup re-reads with its halo: 15.8 -> 7.8 MB per launch, step time
# unchanged (round 4, two alternations, profiles/r04_xcd_group_stem_SK.txt)
XCD_SLAB_MIN_VOX_WIDE = int(_ab("ESM_XCD_SLAB_MIN_VOX_WIDE", "16384"))
# per-launch hints by op name, "name=0x...,name=0x..." (A/B measurements; replaces the tuned / automatic choice)
HINT_SET: Dict[str, int] = {k: int(v, 0) for k, v in (t.split("=") for t in _ab("ESM_HINT_SET", "").split(",") if t)}
# launches (by name, comma-separated) given the slab order whatever their size (A/B measurements)
XCD_SLAB_OPS = tuple(t for t in _ab("ESM_XCD_SLAB_OPS", "").split(",") if t)

# the lean 3x3x3 form's tap-plane split (conv_small.hip; HINT_SMALL_NO_ZSPLIT): ESM_SMALL_ZSPLIT=0 keeps the group
# loop on every layer the lean form runs (A/B measurements)
SMALL_ZSPLIT = _ab("ESM_SMALL_ZSPLIT", "1") != "0"
# the lean form's first-load record (conv_lean_rec.h; HINT_SMALL_NO_RECORD): ESM_SMALL_RECORD=0 keeps the
# struct-argument kernels (A/B)
SMALL_RECORD = _ab("ESM_SMALL_RECORD", "1") != "0"

# shape key -> esm_conv_desc.hint.  Layers not in the table take the library's automatic rules.
_TUNED_PATH = _ab("ESM_TUNED", "") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_hints.json")
TUNED_HINTS: Dict[str, int] = {}
if os.path.exists(_TUNED_PATH) and not _ab("ESM_NO_TUNED", ""):
    with open(_TUNED_PATH) as _f:
        TUNED_HINTS = {k: int(v) for k, v in json.load(_f).get("hints", {}).items()}


def conv_key(d: EsmConvDesc, nd: int) -> str:
    """Shape key of a conv launch: geometry, source channel split, batch, input extent and the
    epilogue features that change the store path (an operand without an address has a fake one, ``_addr``, so a dry
    emission's keys are the real emission's)."""
    cins = "+".join(str(d.src[i].C) for i in range(d.nsrc))
    return (f"{nd}d{'T' if d.transposed else ''} k{d.kh}s{d.stride}p{d.ph} {cins}->{d.Cout} B{d.B} "
            f"{d.Di}x{d.Hi}x{d.Wi} sh{d.shuffle}{'u' if d.up else ''}{'m' if d.mul else ''}"
            f"{'r' if d.res else ''}{'2' if d.out2 else ''}")


def _spatial(t: torch.Tensor, nd: int) -> Tuple[int, int, int]:
    if nd == 3:
        return int(t.shape[2]), int(t.shape[3]), int(t.shape[4])
    return 1, int(t.shape[2]), int(t.shape[3])


def run_conv(ctx: Ctx, pc: PackedConv, srcs: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None, *,
             mul: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
             up: Optional[torch.Tensor] = None, up_f: int = 0, post_scale: float = 1.0, shuffle: int = 1,
             out2: Optional[torch.Tensor] = None, post_scale2: float = 1.0, tag: str = "conv",
             hint: int = 0) -> torch.Tensor:
    """One implicit-GEMM conv launch; ``srcs`` are concatenated along channels (each may be a
    cropped view), the epilogue applies BN/bias, activation, ``*mul``, ``+res``,
    ``+bilinear(up)``, ``*post_scale`` and an optional PixelShuffle(``shuffle``)."""
    d, out, meta = _conv_desc(ctx, pc, srcs, out, mul=mul, res=res, up=up, up_f=up_f, post_scale=post_scale,
                              shuffle=shuffle, out2=out2, post_scale2=post_scale2, tag=tag, hint=hint)
    ctx.meta.append(meta)
    ctx.conv(d)
    return out


# A descriptor's operand that is present but has no address (a dry emission's shape-only ``meta`` buffers, the
# stand-ins of a form query) gets a fake one: non-null, 256-aligned, one per operand slot, so that the library's
# queries (esm_conv_form and the fused launches' *_form) answer for it as for the real operand.  It can never reach a
# kernel: only a dry Ctx accepts such a tensor (require_device), and a dry Ctx submits nothing (Ctx._submit).
_FAKE_ADDR = 1 << 20


def _addr(t: torch.Tensor, slot: int = 0) -> int:
    if not isinstance(t, torch.Tensor):  # (a missing operand must never become an address)
        raise TypeError(f"expected a torch.Tensor operand, got {type(t).__name__}")
    return t.data_ptr() or _FAKE_ADDR + 256 * slot


def _query_pack(pc: PackedConv) -> PackedConv:
    """``pc`` as a predicate reads it.  A predicate needs a layer's geometry and which BN constants it has, not its
    tensors, so one that carries no tensors (weights None, constants a bare True) gets shape-only ones here.  Only the
    predicates do this: a launch builds its descriptors from ``pc`` itself, where a non-tensor operand raises."""
    if isinstance(pc.w, torch.Tensor):
        return pc
    so = lambda t: None if t is None else torch.empty(pc.cout, device="meta")  # noqa: E731
    return dataclasses.replace(pc, w=torch.empty(0, device="meta"), scale=so(pc.scale), shift=so(pc.shift))


def _out_shape(pc: PackedConv, x0: torch.Tensor, shuffle: int = 1) -> Tuple[int, ...]:
    """Shape of the conv's output tensor over an input shaped like ``x0`` (after the PixelShuffle, if any)."""
    nd = pc.nd
    if x0.dim() != nd + 2:
        raise ValueError(f"conv: expected a {nd + 2}-D input, got shape {tuple(x0.shape)}")
    B = int(x0.shape[0])
    Di, Hi, Wi = _spatial(x0, nd)
    k, s, p = pc.k, pc.stride, pc.pad
    if pc.transposed:
        if (k, s, p) != (4, 2, 1):
            raise ValueError("transposed conv: only k=4 s=2 p=1")
        Do, Ho, Wo = (2 * Di if nd == 3 else 1), 2 * Hi, 2 * Wi
    else:
        Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
        Do = (Di + 2 * p - k) // s + 1 if nd == 3 else 1
    if min(Do, Ho, Wo) <= 0:
        raise RuntimeError(f"conv: empty output for input extent {(B, pc.cin, Di, Hi, Wi)}")
    r = int(shuffle)
    if r > 1:
        if pc.cout % (r * r):
            raise ValueError("pixel shuffle: Cout not divisible by r^2")
        return (B, pc.cout // (r * r), Ho * r, Wo * r)
    return (B, pc.cout, Do, Ho, Wo) if nd == 3 else (B, pc.cout, Ho, Wo)


def _set_out(d: EsmConvDesc, out: torch.Tensor, nd: int) -> None:
    ost = out.stride()
    d.out = _addr(out, 1)
    d.ob, d.oc = ost[0], ost[1]
    d.od = ost[2] if nd == 3 else 0
    d.oh = ost[-2]


def _build_desc(pc: PackedConv, srcs: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None, *,
                mul: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
                up: Optional[torch.Tensor] = None, up_f: int = 0, post_scale: float = 1.0, shuffle: int = 1,
                out2: Optional[torch.Tensor] = None, post_scale2: float = 1.0) -> EsmConvDesc:
    """One conv's ``esm_conv_desc`` without its hint: geometry, strides, operand addresses, epilogue.  Reads shapes,
    strides and addresses only (shape-only tensors do: ``_addr``) and has no side effect; the form queries build their
    descriptors with it, ``_conv_desc`` the launches'.  ``out=None`` leaves the output pointer NULL."""
    nd = pc.nd
    d = EsmConvDesc()
    if not srcs or len(srcs) > _lib.MAX_SRC:
        raise ValueError("conv: 1..3 sources")
    x0 = srcs[0]
    oshape = _out_shape(pc, x0, shuffle)
    B = int(x0.shape[0])
    Di, Hi, Wi = _spatial(x0, nd)
    cin = 0
    for i, s in enumerate(srcs):
        if s.dim() != nd + 2 or int(s.shape[0]) != B or _spatial(s, nd) != (Di, Hi, Wi):
            # torch.cat of mismatching tensors raises RuntimeError in the reference
            raise RuntimeError(f"Sizes of tensors must match except in dimension 1 (conv sources "
                               f"{[tuple(t.shape) for t in srcs]})")
        st = s.stride()
        d.src[i].ptr = _addr(s)
        d.src[i].C = int(s.shape[1])
        d.src[i].sb, d.src[i].sc = st[0], st[1]
        d.src[i].sd = st[2] if nd == 3 else 0
        d.src[i].sh = st[-2]
        cin += int(s.shape[1])
    if cin != pc.cin:
        raise RuntimeError(f"conv: input has {cin} channels, layer expects {pc.cin}")
    d.nsrc = max(1, len(srcs))
    d.B, d.Cin = B, cin
    d.Di, d.Hi, d.Wi = Di, Hi, Wi
    r = int(shuffle)
    Ho, Wo = oshape[-2] // max(r, 1), oshape[-1] // max(r, 1)
    d.Do, d.Ho, d.Wo = (oshape[2] if nd == 3 else 1), Ho, Wo
    d.kd = pc.k if nd == 3 else 1
    d.kh = d.kw = pc.k
    d.stride, d.transposed = pc.stride, int(pc.transposed)
    d.pd = pc.pad if nd == 3 else 0
    d.ph = d.pw = pc.pad
    d.Cout, d.cin_pad, d.cout_pad = pc.cout, pc.cin_pad, pc.cout_pad
    d.w = _addr(pc.w)
    d.scale = _addr(pc.scale) if pc.scale is not None else None
    d.shift = _addr(pc.shift) if pc.shift is not None else None
    d.act = pc.act
    d.shuffle = r
    if out is not None:
        _set_out(d, out, nd)
    if mul is not None:
        d.mul = _addr(mul)
        d.mb, d.mc, d.mh = mul.stride(0), mul.stride(1), mul.stride(-2)
    if res is not None:
        if out is None or tuple(res.shape) != tuple(out.shape):
            raise ValueError("conv: residual shape must match the output")
        rs = res.stride()
        d.res = _addr(res)
        d.rb, d.rc = rs[0], rs[1]
        d.rd = rs[2] if nd == 3 else 0
        d.rh = rs[-2]
    if up is not None:
        d.up = _addr(up)
        d.up_h, d.up_w, d.up_f = int(up.shape[-2]), int(up.shape[-1]), int(up_f)
        d.ub, d.uh = up.stride(0), up.stride(-2)
        if d.up_h * up_f != Ho or d.up_w * up_f != Wo:
            raise ValueError("conv: bilinear source extent x factor must equal the output extent")
    d.post_scale = float(post_scale)
    if out2 is not None:
        if out2.stride() != out.stride() or out2.shape != out.shape:
            raise ValueError("conv: out2 must have the output's shape and strides")
        d.out2 = _addr(out2, 2)
        d.post_scale2 = float(post_scale2)
    return d


def _conv_desc(ctx: Optional[Ctx], pc: PackedConv, srcs: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None, *,
               mul: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
               up: Optional[torch.Tensor] = None, up_f: int = 0, post_scale: float = 1.0, shuffle: int = 1,
               out2: Optional[torch.Tensor] = None, post_scale2: float = 1.0, tag: str = "conv",
               hint: int = 0, alloc_out: bool = True):
    """One conv's descriptor as a launch through ``ctx`` gets it: the operands' device checks, the output's allocation,
    ``_build_desc``, the hint, the plan's holds and the op's meta; returns (desc, output tensor, meta).
    ``alloc_out=False`` (the first conv of a fused launch) leaves the output pointer NULL.  ``ctx=None``: the same
    descriptor for a form query, with no side effect: nothing is checked against a device or held, and the output is a
    shape-only stand-in for the contiguous buffer the launch would allocate."""
    if not srcs or len(srcs) > _lib.MAX_SRC:
        raise ValueError("conv: 1..3 sources")
    if ctx is not None:
        for t, what in [(s, "conv input") for s in srcs] + [(out, "conv output"), (mul, "conv mul"), (res, "conv residual"),
                                                             (up, "conv bilinear source"), (out2, "conv out2")]:
            if t is not None:
                require_device(t, what)
        require_on(srcs[0].device, "conv", *srcs, pc.w, pc.scale, pc.shift, out, mul, res, up, out2)
    if out is None and alloc_out:
        shape = _out_shape(pc, srcs[0], shuffle)
        out = ctx.empty(*shape) if ctx is not None else torch.empty(shape, device="meta", dtype=torch.float32)
    d = _build_desc(pc, srcs, out, mul=mul, res=res, up=up, up_f=up_f, post_scale=post_scale, shuffle=shuffle,
                    out2=out2, post_scale2=post_scale2)
    nd, B, cin = pc.nd, d.B, d.Cin
    Di, Hi, Wi, Do, Ho, Wo = d.Di, d.Hi, d.Wi, d.Do, d.Ho, d.Wo
    key = conv_key(d, nd)
    d.hint = int(hint) if hint else HINT_SET.get(tag, TUNED_HINTS.get(key, 0))
    if (B * max(Di * Hi * Wi, Do * Ho * Wo) >= XCD_SLAB_MIN_PIX and (nd == 2 or XCD_SLAB_3D)) or \
            (nd == 3 and XCD_SLAB_3D and pc.cin >= 32 and B * Do * Ho * Wo >= XCD_SLAB_MIN_VOX_WIDE) or \
            tag in XCD_SLAB_OPS:
        d.hint |= HINT_XCD_SLAB
    if not SMALL_ZSPLIT and nd == 3 and pc.k == 3 and not pc.transposed and \
            (d.hint & HINT_SMALL or lib.esm_conv_form(ctypes.byref(d)) == _lib.FORM_SMALL):
        d.hint |= HINT_SMALL | HINT_SMALL_NO_ZSPLIT
    if not SMALL_RECORD and (d.hint & HINT_SMALL or lib.esm_conv_form(ctypes.byref(d)) == _lib.FORM_SMALL):
        d.hint |= HINT_SMALL | HINT_SMALL_NO_RECORD
    if ctx is not None:
        ctx.hold(pc.w, pc.scale, pc.shift, *srcs, out, out2, mul, res, up)
    taps = pc.k ** nd
    if pc.transposed:  # algorithmic ConvT count: every input voxel meets every kernel tap
        macs = B * Di * Hi * Wi * pc.cin * pc.cout * taps
    else:
        macs = B * Do * Ho * Wo * pc.cin * pc.cout * taps
    in_bytes = 4 * B * cin * Di * Hi * Wi
    out_bytes = 4 * B * pc.cout * Do * Ho * Wo * (2 if out2 is not None else 1)
    extra = 4 * sum(t.numel() for t in (res, mul, up) if t is not None)
    w_bytes = 4 * pc.cin * pc.cout * taps  # the layer's weights (the packed slab's padding is not algorithmic)
    meta = dict(name=tag, kind="conv", flops=2 * macs, bytes=in_bytes + out_bytes + extra + w_bytes,
                shape=f"{'T' if pc.transposed else ''}{nd}d k{pc.k}s{pc.stride} {cin}->{pc.cout} "
                      f"in {Di}x{Hi}x{Wi} out {Do}x{Ho}x{Wo}",
                reads=_spans(*srcs, mul, res, up), writes=_spans(out, out2), key=key, hint=d.hint)
    return d, out, meta


# The gwc volume and group_stem as one launch (esm_gwc_stem_f32, gwc_stem.hip) on the volumes the LDS-tiled
# stem takes (ESMStereo-L / -M); ESM_GWC_STEM=0 keeps the two launches (A/B measurements)
GWC_STEM_ENABLED = _ab("ESM_GWC_STEM", "1") != "0"
# its composite weights staged in LDS per k-step (round 5; HINT_GWC_STEM_WLDS) instead of loaded into
# registers (round 6): A/B knob
GWC_STEM_WLDS = _ab("ESM_GWC_STEM_WLDS", "0") == "1"


def _gwc_virt(L: torch.Tensor, G: int, D: int) -> torch.Tensor:
    """The [B, G, D, H, W] volume's geometry only, never read."""
    B, _, H, W = (int(v) for v in L.shape)
    return L.as_strided((B, G, D, H, W), (0, 0, 0, 0, 1))


def gwc_stem_supported(pc: PackedConv, L: torch.Tensor, G: int, D: int, att) -> bool:
    """Whether the fused launch takes the stem over contiguous [B, C, H, W] features (esm_gwc_stem_check on the
    descriptor the launch would get), restricted to where the fused form replaces the tiled stem (tile3_auto:
    >= 2^16 output voxels; the S volumes keep their row-streaming stem)."""
    if att is not None or L.dim() != 4 or not L.is_contiguous():
        return False
    B, C, H, W = (int(v) for v in L.shape)
    if B * D * H * W < (1 << 16):
        return False
    try:
        d = _conv_desc(None, _query_pack(pc), [_gwc_virt(L, G, D)])[0]
    except (ValueError, RuntimeError):
        return False
    return lib.esm_gwc_stem_check(ctypes.byref(d), _addr(L), _addr(L), C, G) == 0


def run_gwc_stem(ctx: Ctx, pc: PackedConv, L: torch.Tensor, R: torch.Tensor, G: int, D: int,
                 tag: str = "gwc_volume+group_stem", hint: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``group_stem(build_gwc_volume(L, R, D, G))`` (models/submodule.py:151-161, models/ESMStereo.py:703-704)
    as one launch: the volume is formed in LDS per k-step and never written (bit-identical to the two
    launches with the tiled stem)."""
    B, C, H, W = (int(v) for v in L.shape)
    if tuple(R.shape) != (B, C, H, W) or not R.is_contiguous() or not L.is_contiguous():
        raise ValueError("gwc_stem: L and R must be contiguous tensors of one shape")
    virt = _gwc_virt(L, G, D)
    d, out, meta = _conv_desc(ctx, pc, [virt], out, tag=tag, hint=hint)
    # tile order and rows per wave (+ the weight form when the caller passes a hint); a standalone stem's
    # tuned form bits do not apply
    d.hint &= HINT_XCD_SLAB | HINT_ROWS_MASK | (HINT_GWC_STEM_WLDS if hint else 0)
    if GWC_STEM_WLDS:
        d.hint |= HINT_GWC_STEM_WLDS
    vol_flops = 2 * B * C * D * H * W
    meta.update(kind="gwc_stem", hint=d.hint, form="wlds" if d.hint & HINT_GWC_STEM_WLDS else "wreg",
                flops=meta["flops"] + vol_flops,
                bytes=4 * B * 2 * C * H * W + 4 * B * pc.cout * D * H * W + 4 * pc.cin * pc.cout * 27,
                reads=_spans(L, R), shape=f"gwc G{G} D{D} + " + meta["shape"])
    ctx.meta.append(meta)
    ctx.gwc_stem(d, L, R, C, G)
    return out


# Two consecutive BasicConvs as one launch (esm_conv_pair2_f32: conv_pair2.hip, and the K-split form of
# conv_pairk.hip); ESM_PAIR2=0 runs every pair as two launches, ESM_PAIRK=0 keeps the K-split form off the
# hot path (A/B measurements)
PAIR2_ENABLED = _ab("ESM_PAIR2", "1") != "0"
PAIRK_ENABLED = _ab("ESM_PAIRK", "1") != "0"
# the K-split form's automatic range: output pixels (B x Ho x Wo) of a 2-D pair (see pairk_auto)
PAIRK_MAX_VOX = int(_ab("ESM_PAIRK_MAX_VOX", "4096"))


def _virt(like: torch.Tensor, shape: Sequence[int]) -> torch.Tensor:
    """The geometry of a fused launch's intermediate map (the first conv's output), never read."""
    return like.as_strided(tuple(shape), (0,) * (len(shape) - 1) + (1,))


def _pair_form(da: EsmConvDesc, db: EsmConvDesc, ksplit: bool = False) -> int:
    """esm_conv_pair2_form of the pair with PAIRK in convB's hint set as ``ksplit`` says (negative: refused)."""
    hint = db.hint
    db.hint = (hint | HINT_PAIRK) if ksplit else (hint & ~HINT_PAIRK)
    form = lib.esm_conv_pair2_form(ctypes.byref(da), ctypes.byref(db))
    db.hint = hint
    return form


class _Pair(NamedTuple):
    """The two descriptors of ``pb(pa(cat(srcs)))`` as one launch with their metas, the intermediate map's geometry,
    and what the library says of them: whether the LDS-staged / the K-split form runs the pair."""
    da: Optional[EsmConvDesc] = None  # None: the pair is no two convs (they raise when they are built on their own)
    ma: Optional[dict] = None
    db: Optional[EsmConvDesc] = None
    mb: Optional[dict] = None
    virt: Optional[torch.Tensor] = None
    lds: bool = False
    ks: bool = False


def _pair_descs(pa: PackedConv, srcs: Sequence[torch.Tensor], pb: PackedConv, out: Optional[torch.Tensor] = None,
                tags: Tuple[str, str] = ("convA", "convB")) -> _Pair:
    """Built without side effect; convB's output is a shape-only stand-in where ``out`` is None."""
    try:
        da, _, ma = _conv_desc(None, pa, srcs, tag=tags[0], alloc_out=False)
        virt = _virt(srcs[0], _out_shape(pa, srcs[0]))
        db, _, mb = _conv_desc(None, pb, [virt], out, tag=tags[1])
    except (ValueError, RuntimeError):
        return _Pair()
    da.hint &= ~HINT_PAIR_REGRESS
    # convB's ROWS field picks the pair's tile rows, PAIRK its form (a standalone conv's tuned hint does not)
    db.hint &= ~(HINT_ROWS_MASK | HINT_PAIRK | HINT_PAIR_NO_RECORD)
    for sel, subs in PAIR2_TH.items():
        if any(x in tags[0] for x in subs):
            db.hint |= HINT_ROWS(sel)
    return _Pair(da, ma, db, mb, virt, _pair_form(da, db) == _lib.PAIR_FORM_LDS,
                 PAIR2_ENABLED and _pair_form(da, db, True) == _lib.PAIR_FORM_KSPLIT)


def _pair_query(pa: PackedConv, pb: PackedConv, srcs: Sequence[torch.Tensor]) -> _Pair:
    return _pair_descs(_query_pack(pa), srcs, _query_pack(pb))


def _pair2_lds_supported(pa: PackedConv, pb: PackedConv, srcs: Sequence[torch.Tensor]) -> bool:
    """Whether the LDS-staged form (conv_pair2.hip) runs the pair: the library's answer for its descriptors."""
    return _pair_query(pa, pb, srcs).lds


def pairk_supported(pa: PackedConv, pb: PackedConv, srcs: Sequence[torch.Tensor]) -> bool:
    """Whether the K-split form (conv_pairk.hip) runs the pair: the library's answer for its descriptors with PAIRK in
    convB's hint (plus the on/off switch)."""
    return _pair_query(pa, pb, srcs).ks


def pair2_supported(pa: PackedConv, pb: PackedConv, srcs: Sequence[torch.Tensor]) -> bool:
    """Whether either form runs the pair (plus the on/off switch)."""
    q = _pair_query(pa, pb, srcs)
    return PAIR2_ENABLED and (q.lds or q.ks)


def _pairk_auto(pa: PackedConv, da: EsmConvDesc, ks: bool) -> bool:
    return PAIRK_ENABLED and pa.nd == 2 and ks and da.B * da.Do * da.Ho * da.Wo <= PAIRK_MAX_VOX


def pairk_auto(pa: PackedConv, pb: PackedConv, srcs: Sequence[torch.Tensor]) -> bool:
    """Where the hot path takes the K-split pair (conv_pairk.hip): the 2-D 3x3 pairs of at most 4096 output
    pixels (B x Ho x Wo).  Fitted in the replayed S-K graph (rocprofv3 per-op tables, profiles/r07_ops_SK_*.txt,
    DESIGN 4.9; pair vs the sum of its two launches in the parent's table, us):
      taken     ref2x.conv2.0+1 (s2 16->16->16, 24x78)   6.1-6.4 vs 9.1-9.3
                ref2x.conv3.0+1 (s2 16->16->16, 12x39)   5.9-6.1 vs 9.3-9.5
                spx_2x.0+1 (s1 48->16->16, 24x78)        8.6-8.8 vs 9.1-9.6
      excluded  ref4x.conv3.0+1 (48x156, 4-row tiles)    8.4-8.8 vs 9.3: the gain is about the spread of two
                                                         recordings (11.3 at 2-row tiles, 13.3 at 1-row)
                ref4x.conv2.0+1 (96x312)                 22.4 vs 14.0
                spx_4x.0+1 (s1 40->16->8, 96x312)        35.2 vs 9.2 + its share of the fused head
                aggregation conv1 / conv2 / conv3 (3-D)  11.0 vs 9.9, 13.1 vs 9.6, 16.9 vs 12.7: a workgroup
                    recomputes 9 row segments of convA per output row (3 planes x 3 rows) and one CU's four
                    matrix pipes pace them (conv3: 1296 MFMAs = 4.3 us per workgroup)."""
    q = _pair_query(pa, pb, srcs)
    return _pairk_auto(pa, q.da, q.ks)


def _pair2_auto(pa: PackedConv, pb: PackedConv, da: EsmConvDesc, lds: bool, ks: bool) -> bool:
    if _pairk_auto(pa, da, ks):
        return True
    if not PAIR2_ENABLED or not lds:
        return False
    light = pa.cin * pa.k * pa.k
    return pb.k == 1 or (light <= 25 and pa.stride == 1) or (pa.k == 1 and da.B * da.Ho * da.Wo <= 8192)


def pair2_auto(pa: PackedConv, pb: PackedConv, srcs: Sequence[torch.Tensor]) -> bool:
    """Where the hot path takes the fused pair.  Measured in the S-K chain (rocprofv3, round 3): the pair
    wins where convA is light -- the dm stacks' 5x5 single-channel head (dm.0 + dm.1: 6.1 vs 9.1 us at
    24x78, 10.6 vs 11.5 at 96x312), a 1x1 convB (dm.2 + dm.3: 6.5 vs 9.2, 7.6 vs 10.4), the 1x1 agg.0 of
    the small refinement levels (7.6 vs 9.0, 8.7 vs 9.3) -- and loses where convA's recomputed halo is
    heavy work for one workgroup (spx 48 / 40 -> 16 3x3: 13.7 vs 9.1, 32.9 vs 14.8; the 192x624 agg_1:
    48.4 vs 20.5; the stride-2 conv pairs at 96x312 and up: 24.2 vs 13.7; the refinement's 1 -> 16
    stride-2 head + conv1.1 at 192x624: 23.6 vs 19.0).  Round 7: the small 3x3 pairs the K-split form takes
    (pairk_auto), which those numbers' LDS-staged form lost."""
    q = _pair_query(pa, pb, srcs)
    return _pair2_auto(pa, pb, q.da, q.lds, q.ks)


# A ConvTranspose BasicConv + crop + cat + the 1x1 BasicConv after it as one launch (esm_convt_1x1_f32,
# conv_up1.hip): the hourglasses' conv3_up -> agg_0[0] and conv2_up -> agg_1[0].  ESM_CONVT_1X1=0 keeps two
# launches; ESM_CONVT_1X1_PAIRED=0 keeps agg_N[0] + agg_N[1] as one pair2 launch where pair2_auto takes it
# (A/B measurements).  S-K, three alternations on one box (round 6): 0.3202-0.3214 ms with two launches,
# 0.3127-0.3140 fused where agg_N[0] is not paired, 0.3077-0.3080 fused everywhere (the default)
CONVT1X1_ENABLED = _ab("ESM_CONVT_1X1", "1") != "0"
CONVT1X1_PAIRED = _ab("ESM_CONVT_1X1_PAIRED", "1") == "1"


def _up1_descs(pa: PackedConv, srcs: Sequence[torch.Tensor], pb: PackedConv, extra: Sequence[torch.Tensor],
               out: Optional[torch.Tensor] = None, tags: Tuple[str, str] = ("convT", "conv1x1")):
    """The two descriptors of ``pb(cat(crop(pa(srcs)), *extra))`` as one launch, built without side effect:
    ``_conv_desc``'s triples of both; the 1x1's output is a shape-only stand-in where ``out`` is None."""
    a = _conv_desc(None, pa, srcs, tag=tags[0], alloc_out=False)
    e0 = extra[0]
    virt = _virt(srcs[0], (int(e0.shape[0]), pa.cout) + tuple(int(v) for v in e0.shape[2:]))  # the crop
    b = _conv_desc(None, pb, [virt, *extra], out, tag=tags[1])
    b[0].hint = 0
    return a, b


def convt_1x1_supported(pa: PackedConv, pb: PackedConv, extra: Sequence[torch.Tensor],
                        srcs: Optional[Sequence[torch.Tensor]] = None) -> bool:
    """Whether ``pb(cat(crop(pa(srcs)), *extra))`` runs as one launch: the library's answer (esm_convt_1x1_form) for the
    descriptors the launch would get (plus the on/off switch).  ``srcs``: the transposed conv's input; default: the
    smallest extent whose doubled extent covers the extra sources, ceil(extent / 2) per dimension."""
    if not CONVT1X1_ENABLED or not extra:
        return False
    if srcs is None:
        e0 = extra[0]
        srcs = [_virt(e0, (int(e0.shape[0]), pa.cin) + tuple((int(v) + 1) // 2 for v in e0.shape[2:]))]
    try:
        (da, _, _), (db, _, _) = _up1_descs(_query_pack(pa), srcs, _query_pack(pb), extra)
    except (ValueError, RuntimeError):
        return False
    return lib.esm_convt_1x1_form(ctypes.byref(da), ctypes.byref(db)) > 0


def run_convt_1x1(ctx: Ctx, pa: PackedConv, srcs: Sequence[torch.Tensor], pb: PackedConv, extra: Sequence[torch.Tensor],
                  tags: Tuple[str, str] = ("convT", "conv1x1"), out: Optional[torch.Tensor] = None,
                  optional: bool = False) -> Optional[torch.Tensor]:
    """``pb(cat(crop(pa(srcs)), *extra))`` (models/ESMStereo.py:163-175, 221-234) as one launch: the transposed
    conv's output is cropped to the extra sources' extent and never written.  ``optional``: where
    ``convt_1x1_supported`` would say no, return None instead of raising; nothing has then been emitted, held or
    allocated (the decision and the launch share one pair of descriptors)."""
    if optional and not CONVT1X1_ENABLED:
        return None
    try:
        (da, _, ma), (db, like, mb) = _up1_descs(pa, srcs, pb, extra, out, tags)
    except (ValueError, RuntimeError):
        if optional:
            return None
        raise
    # the transposed conv's form, as the library names it for these descriptors (conv_up1.hip up1_form)
    form = lib.esm_convt_1x1_form(ctypes.byref(da), ctypes.byref(db))
    if form < 0 and optional:
        return None
    form = {_lib.UP1_FORM_LEAN: "lean", _lib.UP1_FORM_TILED: "tiled"}[check(form, "convt_1x1")]
    for t in (*srcs, *extra, out):
        if t is not None:
            require_device(t, "convt_1x1")
    require_on(srcs[0].device, "convt_1x1", *srcs, *extra, pa.w, pa.scale, pa.shift, pb.w, pb.scale, pb.shift, out)
    if out is None:
        out = ctx.empty(*like.shape)
        _set_out(db, out, pb.nd)
        mb["writes"] = _spans(out)
    ctx.hold(pa.w, pa.scale, pa.shift, pb.w, pb.scale, pb.shift, *srcs, *extra, out)
    B, vox = int(extra[0].shape[0]), math.prod(int(v) for v in extra[0].shape[2:])
    full = 4 * B * pa.cout * int(da.Ho) * int(da.Wo) * (int(da.Do) if pa.nd == 3 else 1)
    name = f"{tags[0]}+{'.'.join(tags[1].split('.')[-2:])}"
    ctx.meta.append(dict(name=name, kind="conv_up1", form=form, flops=ma["flops"] + mb["flops"],
                         bytes=ma["bytes"] - full + mb["bytes"] - 4 * B * pa.cout * vox,
                         shape=f"{ma['shape']} + {mb['shape']}", reads=ma["reads"] + _spans(*extra), writes=mb["writes"],
                         key=ma["key"] + " | " + mb["key"], hint=da.hint))
    if ctx._submit():
        if ctx.plan:
            check(lib.esm_plan_add_convt_1x1(ctx.plan, ctypes.byref(da), ctypes.byref(db)), "plan_add_convt_1x1")
        else:
            check(lib.esm_convt_1x1_f32(ctypes.byref(da), ctypes.byref(db), ctx.stream), "convt_1x1")
    return out


# the hot path's disparity_regression folded into the upsampler's first pair (HINT_PAIR_REGRESS):
# one launch less on the S / M chains; ESM_PAIR_REGRESS=0 keeps the separate launch (A/B)
PAIR_REGRESS_ENABLED = _ab("ESM_PAIR_REGRESS", "1") != "0"
# tile rows of the pairs whose first conv's name contains one of the comma-separated substrings (A/B knobs;
# conv_pair2.hip: 2 / 4 / 8 rows, 8 only up to 16 input channels; default: the launcher's choice)
PAIR2_TH = {sel: tuple(x for x in _ab(f"ESM_PAIR2_TH{n}", "").split(",") if x)
            for sel, n in ((1, 2), (2, 4), (3, 8))}
# the LDS form's staging record (conv_pair2_rec.h; HINT_PAIR_NO_RECORD): ESM_PAIR2_RECORD=0 keeps the
# struct-argument kernels (A/B)
PAIR2_RECORD = _ab("ESM_PAIR2_RECORD", "1") != "0"


def run_pair2(ctx: Ctx, pa: PackedConv, srcs: Sequence[torch.Tensor], pb: PackedConv,
              tags: Tuple[str, str] = ("convA", "convB"), force: bool = False,
              regress: Optional[torch.Tensor] = None, ksplit: Optional[bool] = None,
              out: Optional[torch.Tensor] = None, optional: bool = False) -> Optional[torch.Tensor]:
    """``pb(pa(cat(srcs)))`` (two BasicConvs, BN + GELU each) as one launch where ``pair2_auto`` takes it
    (``force``: wherever supported), else two launches.  ``ksplit``: the K-split form (conv_pairk.hip) or the
    LDS-staged one (conv_pair2.hip); default: K-split where ``pairk_auto`` takes the pair or only it runs it.

    ``regress``: a [B, D, H, W] cost volume whose disparity_regression (models/submodule.py:211-216) is
    ``srcs[0]``, still to be computed: the pair computes it per staged pixel and stores it to ``srcs[0]``
    where the kernel has the shape (5x5 1 -> 16 head, 3x3 convB), else the regression runs first as its
    own launch.  ``optional`` (without ``regress``): where the pair is not taken, return None with nothing emitted
    instead of running the two convs."""
    # the pair's two descriptors, built once: the decisions below are the library's answers for them (hint bits
    # toggled), and the launch gets the same two
    da, ma, db, mb, virt, lds, ks = _pair_descs(pa, srcs, pb, out, tags)
    take = (PAIR2_ENABLED and (lds or ks)) if force else (da is not None and _pair2_auto(pa, pb, da, lds, ks))
    if ksplit is None:
        ksplit = take and regress is None and ((not force and _pairk_auto(pa, da, ks)) or not lds)
    elif take and not (ks if ksplit else lds):
        # the requested form does not run these operands.  By their shapes alone (contiguous stand-ins)?  Then the
        # request is wrong; else it is their addressing, and the pair runs as two launches
        q = _pair_descs(pa, [torch.empty(t.shape, device="meta") for t in srcs], pb, None, tags)
        if not (q.ks if ksplit else q.lds):
            raise ValueError("conv pair: the requested form does not run this pair")
        take = False
    if optional and not take:  # (the caller has another plan for the two convs; nothing is emitted)
        return None
    if regress is not None:
        B_, D_, H_, W_ = (int(v) for v in regress.shape)
        init = srcs[0]
        fuse = (take and PAIR_REGRESS_ENABLED and len(srcs) == 1 and regress.stride(3) == 1 and
                tuple(init.shape) == (B_, 1, H_, W_) and init.stride(3) == 1)
        if fuse:  # convA reads the D cost planes instead of the map, which is stored once: where the library has that form
            dr, st = EsmConvDesc.from_buffer_copy(da), regress.stride()
            dr.src[0].ptr, dr.src[0].C = _addr(regress), D_
            dr.src[0].sb, dr.src[0].sc, dr.src[0].sh = st[0], st[1], st[2]
            dr.out = _addr(init, 2)
            dr.ob, dr.oc, dr.oh = init.stride(0), init.stride(1), init.stride(2)
            dr.hint |= HINT_PAIR_REGRESS
            fuse = _pair_form(dr, db) == _lib.PAIR_FORM_LDS
        if fuse:
            da = dr
        else:
            ctx.regression(0, regress, init, B_, D_, H_, W_)
            regress = None
    if not take:
        return run_conv(ctx, pb, [run_conv(ctx, pa, srcs, tag=tags[0])], out, tag=tags[1])
    for t in (*srcs, out):
        if t is not None:
            require_device(t, "conv pair")
    require_on(srcs[0].device, "conv pair", *srcs, pa.w, pa.scale, pa.shift, pb.w, pb.scale, pb.shift, out, regress)
    if out is None:
        out = ctx.empty(*_out_shape(pb, virt))
        _set_out(db, out, pb.nd)
    if ksplit:
        db.hint |= HINT_PAIRK
    elif not PAIR2_RECORD:
        db.hint |= HINT_PAIR_NO_RECORD
    ctx.hold(pa.w, pa.scale, pa.shift, pb.w, pb.scale, pb.shift, *srcs, out, regress)
    B = int(srcs[0].shape[0])
    mid = 4 * B * pa.cout * int(da.Ho) * int(da.Wo) * (int(da.Do) if pa.nd == 3 else 1)
    name = f"{tags[0]}+{tags[1].rsplit('.', 1)[-1]}"
    flops, byts, reads, writes = ma["flops"] + mb["flops"], ma["bytes"] - mid + mb["bytes"] - mid, ma["reads"], _spans(out)
    if regress is not None:
        name = "disparity_regression+" + name
        flops += 2 * B_ * D_ * H_ * W_
        byts += 4 * B_ * D_ * H_ * W_
        reads, writes = _spans(regress), writes + _spans(init)
    # the pair's kernel as the library names it: K-split (conv_pairk.hip) or LDS-staged (conv_pair2.hip), with the
    # regression in convA or not
    form = {_lib.PAIR_FORM_KSPLIT: "ksplit", _lib.PAIR_FORM_LDS: "lds"}[
        check(lib.esm_conv_pair2_form(ctypes.byref(da), ctypes.byref(db)), "conv_pair2")]
    ctx.meta.append(dict(name=name, kind="conv_pair", form=form + ("+regress" if regress is not None else ""), flops=flops,
                         bytes=byts, shape=f"pair {ma['shape']} + {mb['shape']}",
                         reads=reads, writes=writes, key=ma["key"] + " | " + mb["key"], hint=0))
    ctx.pair2(da, db)
    return out


def run_dwconv(ctx: Ctx, x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
               k: int, stride: int, pad: int, act: int, tag: str = "dwconv",
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise KxK conv (groups = C) + folded BN + activation (``esm_dwconv_f32``): timm's ``conv_dw -> bn``
    (+ act) of the backbone blocks.  ``w``: [C, K*K] contiguous."""
    if stride <= 0 or k <= 0 or not 0 <= pad < k:
        raise ValueError("dwconv: stride and K must be positive, 0 <= pad < K")
    if x.dim() != 4 or x.stride(3) != 1:
        raise ValueError("dwconv: a [B, C, H, W] input with unit W stride")
    require_device(x, "dwconv input")
    B, C, H, W = (int(v) for v in x.shape)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if out is None:
        out = ctx.empty(B, C, Ho, Wo)
    elif tuple(out.shape) != (B, C, Ho, Wo) or out.stride(3) != 1:
        raise ValueError("dwconv: output must be [B, C, Ho, Wo] with unit W stride")
    require_on(x.device, "dwconv", x, w, scale, shift, out)
    d = _lib.EsmDwconvDesc()
    d.x, d.xb, d.xc, d.xh = x.data_ptr(), x.stride(0), x.stride(1), x.stride(2)
    d.w = w.data_ptr()
    d.scale = scale.data_ptr() if scale is not None else None
    d.shift = shift.data_ptr() if shift is not None else None
    d.out, d.ob, d.oc, d.oh = out.data_ptr(), out.stride(0), out.stride(1), out.stride(2)
    d.B, d.C, d.H, d.W, d.K, d.stride, d.pad, d.act, d.Ho, d.Wo = B, C, H, W, k, stride, pad, act, Ho, Wo
    ctx.meta.append(dict(name=tag, kind="dwconv", flops=2 * B * C * Ho * Wo * k * k,
                         bytes=4 * (x.numel() + out.numel() + C * k * k), reads=_spans(x), writes=_spans(out)))
    ctx.dwconv(d)
    return out


@dataclass
class SmixStage:
    ln_w: torch.Tensor
    fc0_w: torch.Tensor
    fc0_b: torch.Tensor
    fc2_w: torch.Tensor
    fc2_b: torch.Tensor


def run_smix(ctx: Ctx, x: torch.Tensor, stages: Sequence[SmixStage], *, dw: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
             res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, tag: str = "smix") -> torch.Tensor:
    require_device(x, "smix input")
    if not x.is_contiguous():
        raise ValueError("smix: input must be contiguous")
    B, C, H, W = (int(v) for v in x.shape)
    if out is None:
        out = ctx.empty(B, C, H, W)
    d = EsmSmixDesc()
    d.x, d.out = x.data_ptr(), out.data_ptr()
    if res is not None:
        require_device(res, "smix residual")
        if not res.is_contiguous() or res.shape != x.shape:
            raise ValueError("smix: residual must be contiguous and shaped like the input")
        d.res = res.data_ptr()
    if dw is not None:
        d.dw_w, d.dw_b = dw[0].data_ptr(), dw[1].data_ptr()
        d.dw_k = int(dw[0].shape[-1])
    if len(stages) > _lib.SMIX_MAX_STAGES:
        raise ValueError("smix: at most 2 stages per launch")
    require_on(x.device, "smix", x, out, res, *(dw or ()),
               *[t for st in stages for t in (st.ln_w, st.fc0_w, st.fc0_b, st.fc2_w, st.fc2_b)])
    d.nstages = len(stages)
    for i, st in enumerate(stages):
        d.stage[i].ln_w = st.ln_w.data_ptr()
        d.stage[i].fc0_w, d.stage[i].fc0_b = st.fc0_w.data_ptr(), st.fc0_b.data_ptr()
        d.stage[i].fc2_w, d.stage[i].fc2_b = st.fc2_w.data_ptr(), st.fc2_b.data_ptr()
        ctx.hold(st.ln_w, st.fc0_w, st.fc0_b, st.fc2_w, st.fc2_b)
    d.B, d.C, d.H, d.W = B, C, H, W
    ctx.hold(x, out, res, *(dw or ()))
    npix = B * H * W
    ctx.meta.append(dict(name=tag, kind="smix", flops=npix * (2 * C * C * len(stages) + (2 * C * d.dw_k ** 2 if dw else 0)),
                         bytes=4 * npix * C * (3 if res is not None else 2), shape=f"C{C} {H}x{W} dw{d.dw_k}",
                         reads=_spans(x, res), writes=_spans(out)))
    ctx.smix(d)
    return out


# The whole FMBlock as two launches (esm_fmnet_desc.work, smix.hip fm2a / fm2b) on maps of at least this
# many pixels (B x H x W); smaller maps keep the one-launch form, whose halo recompute is cheap there and
# whose single launch boundary matters (S-K: 24 x 78)
FM2_MIN_PIX = int(_ab("ESM_FM2_MIN_PIX", "16384"))


def run_fmnet(ctx: Ctx, x: torch.Tensor, stages: Sequence[SmixStage], dw0: Tuple[torch.Tensor, torch.Tensor],
              dw1: Tuple[torch.Tensor, torch.Tensor], out: Optional[torch.Tensor] = None,
              tag: str = "fmnet", conv: Optional[Tuple[torch.Tensor, ...]] = None,
              two_launch: Optional[bool] = None, work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``FMBlock.net(x) + x`` (shufflemixer.py:129-130) in one launch: stages = SMLayer0.mlp1, .mlp2,
    SMLayer1.mlp1, .mlp2; dw0 / dw1 = the two SMLayers' depthwise convs (weight, bias).  With ``conv`` =
    (conv0 weight [C+16, C, 3, 3], bias, conv2 weight [C, C+16, 1, 1], bias) the whole FMBlock
    (shufflemixer.py:129-131: ``t = net(x) + x; conv(t) + t``) is the one launch, or on large maps
    (``two_launch``; default: B x H x W >= FM2_MIN_PIX) two launches through a scratch buffer (``work``: a
    contiguous [B, C, H, W] buffer to use for it; default: a fresh one)."""
    require_device(x, "fmnet input")
    if not x.is_contiguous():
        raise ValueError("fmnet: input must be contiguous")
    if len(stages) != 4:
        raise ValueError("fmnet: four mlp stages")
    B, C, H, W = (int(v) for v in x.shape)
    if out is None:
        out = ctx.empty(B, C, H, W)
    d = _lib.EsmFmnetDesc()
    d.x, d.out = x.data_ptr(), out.data_ptr()
    d.dw_w[0], d.dw_b[0] = dw0[0].data_ptr(), dw0[1].data_ptr()
    d.dw_w[1], d.dw_b[1] = dw1[0].data_ptr(), dw1[1].data_ptr()
    d.dw_k = int(dw0[0].shape[-1])
    if int(dw1[0].shape[-1]) != d.dw_k:
        raise ValueError("fmnet: both SMLayers need the same depthwise kernel")
    require_on(x.device, "fmnet", x, out, *dw0, *dw1,
               *[t for st in stages for t in (st.ln_w, st.fc0_w, st.fc0_b, st.fc2_w, st.fc2_b)])
    for i, st in enumerate(stages):
        d.stage[i].ln_w = st.ln_w.data_ptr()
        d.stage[i].fc0_w, d.stage[i].fc0_b = st.fc0_w.data_ptr(), st.fc0_b.data_ptr()
        d.stage[i].fc2_w, d.stage[i].fc2_b = st.fc2_w.data_ptr(), st.fc2_b.data_ptr()
        ctx.hold(st.ln_w, st.fc0_w, st.fc0_b, st.fc2_w, st.fc2_b)
    d.B, d.C, d.H, d.W = B, C, H, W
    if conv is not None:
        w0, b0, w2, b2 = conv
        hid = int(w0.shape[0])
        if tuple(w0.shape) != (hid, C, 3, 3) or tuple(w2.shape[:2]) != (C, hid) or hid != C + 16:
            raise ValueError("fmnet: FMBlock.conv must be Conv2d(C, C+16, 3) and Conv2d(C+16, C, 1)")
        for t in conv:
            if not t.is_contiguous():
                raise ValueError("fmnet: conv weights must be contiguous")
        require_on(x.device, "fmnet conv", *conv)
        d.conv0_w, d.conv0_b, d.conv2_w, d.conv2_b = (t.data_ptr() for t in conv)
        d.hid = hid
        ctx.hold(*conv)
        if two_launch is None:
            two_launch = B * H * W >= FM2_MIN_PIX
        if two_launch:
            if work is None:
                work = ctx.empty(B, C, H, W)
            elif tuple(work.shape) != (B, C, H, W) or not work.is_contiguous():
                raise ValueError("fmnet: work must be a contiguous [B, C, H, W] buffer")
            require_on(x.device, "fmnet work", work)
            d.work = work.data_ptr()
            ctx.hold(work)
    ctx.hold(x, out, *dw0, *dw1)
    npix = B * H * W
    # algorithmic flops per pixel: four split-point MLPs (C/2 -> C -> C/2: 2 * C * C), two depthwise
    # KxK convs, and with the fused FMBlock.conv the 3x3 C -> hid and the 1x1 hid -> C
    flops = 2 * C * C * 4 + 2 * 2 * C * d.dw_k ** 2 + (2 * d.hid * C * 9 + 2 * C * d.hid if conv is not None else 0)
    ctx.meta.append(dict(name=tag, kind="fmnet", flops=npix * flops,
                         bytes=4 * npix * C * 2 + 4 * (sum(int(t.numel()) for t in conv) if conv is not None else 0),
                         shape=f"C{C} {H}x{W} dw{d.dw_k} x2" + (f" +conv{d.hid}" if conv is not None else ""),
                         reads=_spans(x), writes=_spans(out),
                         # (from the choice, not from d.work: a dry emission's scratch buffer has no address)
                         launches=2 if conv is not None and two_launch else 1))
    ctx.fmnet(d)
    return out


_SHUFFLE_TAIL_FORMS = {_lib.SHUFFLE_TAIL_FORM_WINDOW: "window", _lib.SHUFFLE_TAIL_FORM_ROW4: "row4",
                       _lib.SHUFFLE_TAIL_FORM_ROW8: "row8"}


@dataclass
class PackedShuffleTail:
    """``upsampling`` (Conv2d 1x1 + PixelShuffle + SiLU) and ``tail`` (Conv2d 3x3 -> 1) weights."""

    up_w: torch.Tensor
    up_b: torch.Tensor
    tail_w: torch.Tensor
    tail_b: Optional[torch.Tensor]
    nf: int
    r: int


def pack_shuffle_tail(up: torch.nn.Conv2d, tail: torch.nn.Conv2d, r: int) -> PackedShuffleTail:
    nf = int(tail.weight.shape[1])
    if tuple(up.weight.shape) != (nf * r * r, nf, 1, 1) or up.bias is None:
        raise ValueError("shuffle_tail: upsampling must be Conv2d(nf, nf*r*r, 1) with bias")
    if tuple(tail.weight.shape) != (1, nf, 3, 3) or tuple(tail.padding) != (1, 1) or tuple(tail.stride) != (1, 1):
        raise ValueError("shuffle_tail: tail must be Conv2d(nf, 1, 3, 1, 1)")
    return PackedShuffleTail(up.weight.detach().float().reshape(nf * r * r, nf).contiguous(),
                             up.bias.detach().float().contiguous(),
                             tail.weight.detach().float().reshape(nf, 3, 3).contiguous(),
                             tail.bias.detach().float().contiguous() if tail.bias is not None else None, nf, int(r))


def run_shuffle_tail(ctx: Ctx, x: torch.Tensor, p: PackedShuffleTail, out: Optional[torch.Tensor] = None,
                     tag: str = "shuffle_tail", form: int = 0) -> torch.Tensor:
    """``tail(SiLU(PixelShuffle(r)(up(x))))`` as one launch (``esm_shuffle_tail_f32``): the
    ``upsampling`` + ``tail`` pair of the ESM upsamplers (models/ESMStereo.py:264-271,301-302).
    ``form`` (nf 8, r 4): 0 automatic, 1 window form, 2 / 3 the row form with 4 / 8 rows per workgroup."""
    require_device(x, "shuffle_tail input")
    B, nf, H, W = (int(v) for v in x.shape)
    r = p.r
    if nf != p.nf:
        raise RuntimeError(f"shuffle_tail: input has {nf} channels, layer expects {p.nf}")
    if out is None:
        out = ctx.empty(B, 1, H * r, W * r)
    require_device(out, "shuffle_tail output")
    if tuple(out.shape) != (B, 1, H * r, W * r):
        raise ValueError("shuffle_tail: output must be [B, 1, r*H, r*W]")
    require_on(x.device, "shuffle_tail", x, out, p.up_w, p.up_b, p.tail_w, p.tail_b)
    d = EsmShuffleTailDesc()
    d.x = _addr(x)
    d.xb, d.xc, d.xh = x.stride(0), x.stride(1), x.stride(2)
    d.up_w, d.up_b, d.tail_w = _addr(p.up_w), _addr(p.up_b), _addr(p.tail_w)
    d.tail_b = _addr(p.tail_b) if p.tail_b is not None else None
    d.out = _addr(out, 1)
    d.ob, d.oh = out.stride(0), out.stride(2)
    d.B, d.nf, d.H, d.W, d.r = B, nf, H, W, r
    npix = B * H * W * r * r
    d.flags = (1 if npix >= XCD_SLAB_MIN_PIX else 0) | (int(form) & 3) << 1
    ctx.hold(x, out, p.up_w, p.up_b, p.tail_w, p.tail_b)
    # upsampling: the 1x1 nf -> nf*r^2 on H x W = nf^2 MACs per full-resolution pixel; tail: 3x3 nf -> 1
    # the kernel as the library names it for this descriptor (shuffle_tail.hip shuffle_tail_form)
    kform = _SHUFFLE_TAIL_FORMS[check(lib.esm_shuffle_tail_form(ctypes.byref(d)), "shuffle_tail")]
    ctx.meta.append(dict(name=tag, kind="shuffle_tail", form=kform, slab=d.flags & 1, flops=2 * npix * nf * (nf + 9),
                         bytes=4 * (B * nf * H * W + npix), shape=f"nf{nf} r{r} in {H}x{W} out {H * r}x{W * r}",
                         reads=_spans(x), writes=_spans(out)))
    ctx.shuffle_tail(d)
    return out


# tail(upsampling(x)) and the refinement's first conv in one launch (esm_shuffle_conv_f32);
# ESM_SHUFFLE_CONV=0 runs them as two launches (A/B measurements)
SHUFFLE_CONV_ENABLED = _ab("ESM_SHUFFLE_CONV", "1") != "0"
# largest low-resolution input (B * H * W) the window form is used on.  Round 3: faster than the two launches
# at S-K's 2x stage (24x78 in: 8.4 vs 10.5 us), slower at the 4x stage (96x312 in: 23.2 vs 20.8 us).  The
# row form (shuffle_conv4_kernel, nf 8, r 4, C 16 only; round 4) has no cap: it won at the 4x stage.  Heads
# without a row form (L's nf 16) keep the cap (at L-K B=4 the fused window form took 145.8 us
# against 116.3 + 26.8 us as two launches).
SHUFFLE_CONV_MAX_PIX = int(_ab("ESM_SHUFFLE_CONV_MAXPIX", "8192"))


def shuffle_conv_supported(p: PackedShuffleTail, conv: PackedConv, x: Optional[torch.Tensor] = None) -> bool:
    row_form = (p.nf, p.r, conv.cout) == (8, 4, 16)
    if x is not None and not row_form and int(x.shape[0]) * int(x.shape[2]) * int(x.shape[3]) > SHUFFLE_CONV_MAX_PIX:
        return False
    return SHUFFLE_CONV_ENABLED and (p.nf, p.r, conv.cout) in ((8, 4, 16), (8, 2, 16), (16, 2, 32), (16, 4, 32)) and \
        conv.nd == 2 and not conv.transposed and (conv.k, conv.stride, conv.pad, conv.cin) == (3, 2, 1, 1) and \
        conv.act == ACT_GELU


# the (nf 8, r 4, C 16) head + conv form with the pre-conv (the 4x stage) where the caller leaves the choice to the
# library (A/B knob: 2 shuffle_conv4_kernel, 3 shuffle_conv5_kernel; 0 = the library's rule)
SC_FORM = int(_ab("ESM_SC_FORM", "0"))
# the upsampler stage's spx_<t>[1] computed inside the row-form shuffle_conv launch (ESM_SHUFFLE_PRE=0: its own
# launch, A/B measurements)
SHUFFLE_PRE_ENABLED = _ab("ESM_SHUFFLE_PRE", "1") != "0"


# the refinement's conv1[1] inside the same launch as well (esm_shuffle_conv_desc.w2, the whole conv1 of the 4x
# stage in one launch; ESM_SC11=0: conv1[1] as its own launch, A/B measurements)
SC11_ENABLED = _ab("ESM_SC11", "1") != "0"
# tile of that launch (esm_shuffle_tail_desc.flags bits 3-4; A/B knob): 0 = 4 low-res rows on 8 waves, two
# workgroups per CU (round 6, the default); 1 = 8 rows on 8 waves (round 5); 2 = 4 rows on 4 waves
SC11_TILE = int(_ab("ESM_SC11_TILE", "1"))


def shuffle_conv_pre_supported(p: PackedShuffleTail, conv: PackedConv, pre: PackedConv) -> bool:
    """Whether ``pre`` (BasicConv(Cp <= 16, nf, 3, 1, 1), BN + GELU) can run inside the row-form launch."""
    return SHUFFLE_PRE_ENABLED and shuffle_conv_supported(p, conv) and (p.nf, p.r, conv.cout) == (8, 4, 16) and \
        pre.nd == 2 and not pre.transposed and (pre.k, pre.stride, pre.pad) == (3, 1, 1) and pre.cin <= 16 and \
        pre.cout == p.nf and pre.act == ACT_GELU


def run_shuffle_conv(ctx: Ctx, x: torch.Tensor, p: PackedShuffleTail, conv: PackedConv,
                     tag: str = "shuffle_conv", form: int = 0, pre: Optional[PackedConv] = None,
                     conv2: Optional[PackedConv] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``conv(tail(SiLU(PixelShuffle(r)(up(x)))))`` with ``conv`` = up_refinement.conv1[0] (BasicConv(1, C,
    3, 2, 1): BN + GELU), one launch (``esm_shuffle_conv_f32``); the 1-channel map between them is never
    stored.  Returns the conv output [B, C, ceil(r*H/2), ceil(r*W/2)].  ``form`` (nf 8, r 4, C 16): 0
    automatic, 1 the window form, 2 the row form (8 low-res rows), 3 the row form with the refinement conv on
    the matrix cores.  ``pre`` (nf 8, r 4, C 16): ``x`` is then the input of
    ``pre`` (the stage's spx_<t>[1], BasicConv(Cp, nf, 3, 1, 1)), computed inside the launch as well.
    ``conv2`` (with ``pre``): up_refinement.conv1[1] (BasicConv(C, C, 3, 1, 1)) too; the result is then its
    output (the whole conv1), the first conv's map never stored."""
    require_device(x, "shuffle_conv input")
    B, nf, H, W = (int(v) for v in x.shape)
    r = p.r
    if (p.nf, p.r, conv.cout) == (8, 4, 16) and form == 0 and SC_FORM and pre is not None:
        form = SC_FORM
    if pre is not None:
        if not shuffle_conv_pre_supported(p, conv, pre):
            raise ValueError("shuffle_conv: unsupported pre-conv")
        if nf != pre.cin:
            raise RuntimeError(f"shuffle_conv: pre-conv input has {nf} channels, layer expects {pre.cin}")
        if x.stride(3) != 1:
            raise ValueError("shuffle_conv: pre-conv input rows must be contiguous")
        nf = p.nf
    if nf != p.nf:
        raise RuntimeError(f"shuffle_conv: input has {nf} channels, layer expects {p.nf}")
    if not shuffle_conv_supported(p, conv):  # (size policy is the caller's: blocks.py)
        raise ValueError("shuffle_conv: unsupported head / conv geometry")
    Ho2, Wo2 = (H * r + 1) // 2, (W * r + 1) // 2
    if out is None:
        out = ctx.empty(B, conv.cout, Ho2, Wo2)
    elif tuple(out.shape) != (B, conv.cout, Ho2, Wo2) or out.stride(3) != 1:
        raise ValueError("shuffle_conv: output must be [B, C, ceil(r*H/2), ceil(r*W/2)] with unit W stride")
    require_on(x.device, "shuffle_conv", x, out, p.up_w, p.up_b, p.tail_w, p.tail_b, conv.w, conv.scale, conv.shift)
    d = EsmShuffleConvDesc()
    t = d.st
    if pre is None:
        t.x = _addr(x)
        t.xb, t.xc, t.xh = x.stride(0), x.stride(1), x.stride(2)
    else:
        t.x = None
        t.xb, t.xc, t.xh = nf * H * W, H * W, W  # the virtual head input (never read)
        d.pre_x = _addr(x)
        d.pb, d.pc, d.ph = x.stride(0), x.stride(1), x.stride(2)
        d.pre_w = _addr(pre.w)
        d.pre_scale = pre.scale.data_ptr() if pre.scale is not None else None
        d.pre_shift = pre.shift.data_ptr() if pre.shift is not None else None
        d.pre_cin, d.pre_cin_pad, d.pre_cout_pad = pre.cin, pre.cin_pad, pre.cout_pad
        require_on(x.device, "shuffle_conv pre-conv", pre.w, pre.scale, pre.shift)
        ctx.hold(pre.w, pre.scale, pre.shift)
        form = form if form == 3 else 2  # the row forms (3: the refinement conv on the matrix cores)
    t.up_w, t.up_b, t.tail_w = _addr(p.up_w), _addr(p.up_b), _addr(p.tail_w)
    t.tail_b = _addr(p.tail_b) if p.tail_b is not None else None
    t.out = None
    t.B, t.nf, t.H, t.W, t.r = B, nf, H, W, r
    t.flags = (1 if B * H * W * r * r >= XCD_SLAB_MIN_PIX else 0) | (int(form) & 3) << 1
    d.w = _addr(conv.w)
    d.scale = conv.scale.data_ptr() if conv.scale is not None else None
    d.shift = conv.shift.data_ptr() if conv.shift is not None else None
    d.out = _addr(out, 1)
    d.ob, d.oc, d.oh = out.stride(0), out.stride(1), out.stride(2)
    d.C, d.cin_pad, d.cout_pad = conv.cout, conv.cin_pad, conv.cout_pad
    ctx.hold(x, out, p.up_w, p.up_b, p.tail_w, p.tail_b, conv.w, conv.scale, conv.shift)
    if conv2 is not None:
        if pre is None or (p.nf, p.r, conv.cout) != (8, 4, 16) or conv2.nd != 2 or conv2.transposed or \
                (conv2.k, conv2.stride, conv2.pad, conv2.cin, conv2.cout) != (3, 1, 1, conv.cout, conv.cout) or \
                conv2.act != ACT_GELU:
            raise ValueError("shuffle_conv: the fused second conv must be BasicConv(C, C, 3, 1, 1) behind the "
                             "(8, 4, 16) row form with its pre-conv")
        require_on(x.device, "shuffle_conv second conv", conv2.w, conv2.scale, conv2.shift)
        d.w2 = _addr(conv2.w)
        d.scale2 = conv2.scale.data_ptr() if conv2.scale is not None else None
        d.shift2 = conv2.shift.data_ptr() if conv2.shift is not None else None
        d.cin_pad2, d.cout_pad2 = conv2.cin_pad, conv2.cout_pad
        t.flags |= (SC11_TILE & 3) << 3
        ctx.hold(conv2.w, conv2.scale, conv2.shift)
    npix = B * H * W * r * r
    flops = 2 * npix * nf * (nf + 9) + 2 * B * Ho2 * Wo2 * conv.cout * 9  # head as shuffle_tail + the 1 -> C 3x3
    cin_read = nf
    if pre is not None:  # + the 3x3 Cp -> nf pre-conv on the low-resolution map, whose weights are read too
        flops += 2 * B * H * W * nf * pre.cin * 9
        cin_read = pre.cin
    if conv2 is not None:  # + the 3x3 C -> C second conv on the output map
        flops += 2 * B * Ho2 * Wo2 * conv.cout * conv.cout * 9
    # the kernel as the library names it for this descriptor (shuffle_tail.hip shuffle_conv_form).  "+pre" /
    # "+conv2": the convs fused around the head
    kf = check(lib.esm_shuffle_conv_form(ctypes.byref(d)), "shuffle_conv")
    if kf >= _lib.SHUFFLE_CONV_FORM_CONV1:
        kform = f"row+pre+conv2/tile{kf - _lib.SHUFFLE_CONV_FORM_CONV1}"
    else:
        kform = ("window", "row-valu", "row-mfma")[kf & ~_lib.SHUFFLE_CONV_FORM_PRE] + \
            ("+pre" if kf & _lib.SHUFFLE_CONV_FORM_PRE else "")
    ctx.meta.append(dict(name=tag, kind="shuffle_conv", form=kform, slab=t.flags & 1, flops=flops,
                         bytes=4 * (B * cin_read * H * W + B * conv.cout * Ho2 * Wo2) +
                         (4 * 9 * pre.cin * nf if pre is not None else 0) +
                         (4 * 9 * conv.cout * conv.cout if conv2 is not None else 0),
                         shape=(f"pre {pre.cin}->{nf} k3 " if pre is not None else "") +
                         f"nf{nf} r{r} in {H}x{W} -> x {H * r}x{W * r} -> C{conv.cout} {Ho2}x{Wo2}" +
                         (f" -> k3 C{conv.cout}" if conv2 is not None else ""),
                         reads=_spans(x), writes=_spans(out)))
    ctx.shuffle_conv(d)
    return out
