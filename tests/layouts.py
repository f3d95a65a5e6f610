"""Layout harness: a tensor's values as a strided view inside a larger, poisoned allocation.

The kernels run on views (crops, channel slices, buffers carved 256 B apart out of one arena) whose
neighbouring bytes belong to somebody else.  ``embed`` builds such a view on purpose: every element of the
allocation outside the view holds ``SENTINEL``, a quiet NaN with a payload, so

* a load one element outside the logical extent poisons the result (a zero weight or a 0/1 mask does not
  hide NaN), and
* a store one element outside it changes a bit pattern that ``assert_guards_intact`` compares.

A flat guard of ``GUARD`` elements at both ends keeps a stray access of a few rows inside the allocation: the
tests detect it, they provoke nothing.  Works on CPU and GPU tensors (the host tests of this module are the
proof that the GPU tests would fail on a kernel that writes one element too far).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

SENTINEL = 0x7FC0BEEF       # int32 bit pattern of the float32 guard cells: a quiet NaN, payload 0xbeef
SENTINEL_BYTE = 0xA5        # guard bytes around the u8 / u16 buffers
GUARD = 16 * 1024           # elements of flat guard at each end of every allocation
PLACEMENTS = ("gapped16", "odd")

# (before, after) margins in elements: batch, channel, plane, row, column
_MARGIN = {"b": 1, "c": 3, "d": 1, "h": 2, "w": 3}
_AXES = {3: "chw", 4: "bchw", 5: "bcdhw"}
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _raw(n: int, dtype: torch.dtype, device) -> torch.Tensor:
    """``n`` elements of ``dtype`` holding the sentinel."""
    if dtype == torch.float32:
        return torch.full((n,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full((n * size,), SENTINEL_BYTE, dtype=torch.uint8, device=device).view(dtype)


def embed(t: torch.Tensor, where: str, device=None, spatial: bool = True) -> torch.Tensor:
    """A view with ``t``'s shape and values inside a larger allocation full of the sentinel.

    ``where``:
      ``"gapped16"``  margins on every axis (>= 1 batch, 3 channels, 1 plane, 2 rows, 3 columns); the base
                      offset and every stride are multiples of 4 floats, so 16-byte vector paths stay
                      active and a store past the row end lands on a guard cell;
      ``"odd"``       the same margins with column offset 3 and an odd row stride: the base is only
                      4-byte aligned and row starts take every alignment (the scalar fall-backs run);
      ``"carved"``    a contiguous block at a 256-byte-aligned offset, as an arena hands buffers out (for
                      entry points that take bare pointers; any dtype).
    ``spatial=False`` (gapped16 / odd): margins along batch and channel only, whole planes stay contiguous
    (the pointwise form's layout); "odd" then only moves the base off 16-byte alignment.
    """
    dev = torch.device(device) if device is not None else t.device
    if where == "carved":
        size = t.element_size()
        n = t.numel()
        body = (n * size + 255) // 256 * 256 // size
        raw = _raw(GUARD + 256 // size + body + GUARD, t.dtype, dev)
        start = GUARD + (-(raw.data_ptr() + GUARD * size)) % 256 // size  # (a host allocation may be 64-byte aligned)
        v = raw[start:start + n].view(t.shape)
        v.copy_(t)
        return v
    if where not in PLACEMENTS:
        raise ValueError(f"embed: unknown placement {where!r}")
    if t.dtype != torch.float32 or t.dim() not in _AXES:
        raise ValueError("embed: strided placements take float32 [C,H,W], [B,C,H,W] or [B,C,D,H,W] tensors")
    axes = _AXES[t.dim()]
    lo = [_MARGIN[a] if (spatial or a in "bc") else 0 for a in axes]
    hi = list(lo)
    if spatial:
        if where == "gapped16":
            lo[-1] = 4                                   # column offset: >= 3 and a multiple of 4
            hi[-1] += -(t.shape[-1] + lo[-1] + hi[-1]) % 4  # row stride a multiple of 4
        else:
            hi[-1] += (t.shape[-1] + lo[-1] + hi[-1] + 1) % 2  # an odd row stride
    padded = [n + a + b for n, a, b in zip(t.shape, lo, hi)]
    strides = [1] * len(padded)
    for i in range(len(padded) - 2, -1, -1):
        strides[i] = strides[i + 1] * padded[i + 1]
    if where == "gapped16" and any(s % 4 for s, ax in zip(strides[:-1], axes) if spatial or ax in "bc"):
        # (spatial=False: planes whose size is no multiple of 4 cannot be 16-byte aligned; say so)
        raise ValueError("embed: gapped16 needs a plane size that is a multiple of 4 without spatial margins")
    inner = strides[0] * padded[0]
    off = sum(a * s for a, s in zip(lo, strides))
    front = GUARD
    if where == "odd":
        front += (3 - (GUARD + off)) % 4  # base offset = 3 mod 4 elements: 4-byte aligned only
    raw = _raw(front + inner + GUARD, torch.float32, dev)
    v = raw.as_strided(tuple(t.shape), tuple(strides), front + off)
    v.copy_(t)
    return v


FAR_AXES = ("b", "c", "d", "h")
FAR_ALIGN = 4               # elements: the far stride is a multiple of it (16-byte aligned entries, as a fresh tensor's)


class FarArena:
    """One device allocation that successive ``embed_far`` views of a test share, one view at a time: each ``take``
    fills it with the sentinel again (milliseconds), where a fresh allocation of several GiB after the release of
    the last one was measured to stall for 3 to 5 s now and then.  Grows when asked for more (to a multiple of
    ``round_to`` elements); ``release`` frees it."""

    def __init__(self, device, round_to: int = 1):
        self.device, self.raw, self.round_to = torch.device(device), None, round_to

    def take(self, n: int) -> torch.Tensor:
        if self.raw is None or self.raw.numel() < n:
            self.release()
            # (rounded up, so that operands of nearly the same size share one allocation)
            self.raw = _raw(-(-n // self.round_to) * self.round_to, torch.float32, self.device)
        else:
            self.raw.view(torch.int32).fill_(SENTINEL)
        return self.raw

    def release(self) -> None:
        self.raw = None
        if self.device.type == "cuda":
            torch.cuda.empty_cache()


def embed_far(t: torch.Tensor, axis: str, stride_elems: int, device=None, tail_bytes: int = 0,
              arena: Optional[FarArena] = None) -> torch.Tensor:
    """A view with ``t``'s shape and values whose ``axis`` ("b" | "c" | "d" | "h") has the element stride
    ``stride_elems``; every other axis is packed: contiguous inside it, and outside it as the axes of a tensor whose
    ``axis`` entries are padded to the stride (the layout of a slice of such a tensor: a batch stride of C channel
    strides, as the launchers' stride checks expect).  For operands near and beyond the 32-bit addressing limits
    of the kernels (tests/test_gpu_addressing_limits.py).

    The view lies in one allocation full of the sentinel with ``GUARD`` elements in front, long enough to hold the
    view and ``tail_bytes`` past the base of every batch item (``far_tail_elems``).  With a tail of 4 GiB every 32-bit
    byte offset from an item's base -- a wrapped offset, an out-of-range mark taken for an address -- lands on a
    sentinel cell of this allocation or on the view: a load reads NaN (or another cell's value), a store is seen by
    ``assert_guards_intact``, and nothing leaves the allocation.  ``guard_snapshot`` keeps no copy of an allocation
    this large (``SPARSE_FROM``).  ``arena``: take the allocation from it (at least as long, all sentinel; any
    earlier view of the arena is overwritten)."""
    dev = torch.device(device) if device is not None else t.device
    if t.dtype != torch.float32 or t.dim() not in (4, 5):
        raise ValueError("embed_far: float32 [B,C,H,W] or [B,C,D,H,W] tensors")
    axes = _AXES[t.dim()]
    if axis not in FAR_AXES or axis not in axes:
        raise ValueError(f"embed_far: axis {axis!r} of a {t.dim()}-D tensor")
    if stride_elems % FAR_ALIGN or tail_bytes % 4:
        raise ValueError("embed_far: the stride must be a multiple of 4 elements, the tail of 4 bytes")
    k = axes.index(axis)
    strides = [0] * t.dim()
    run = 1
    for i in range(t.dim() - 1, -1, -1):
        if i == k and stride_elems < run:
            raise ValueError(f"embed_far: stride {stride_elems} overlaps entries of {run} elements")
        strides[i] = stride_elems if i == k else run
        run = t.shape[i] * strides[i]
    item = sum((n - 1) * st for n, st in zip(t.shape[1:], strides[1:])) + 1  # one batch item, first cell to last + 1
    reach = (t.shape[0] - 1) * strides[0] + max(item, tail_bytes // 4)
    need = GUARD + reach + GUARD
    raw = arena.take(need) if arena is not None else _raw(need, torch.float32, dev)
    v = raw.as_strided(tuple(t.shape), tuple(strides), GUARD)
    v.copy_(t)
    return v


def far_tail_elems(view: torch.Tensor) -> int:
    """Elements of ``view``'s allocation from the base of its last batch item to the end guard."""
    n = view.untyped_storage().nbytes() // view.element_size()
    return n - GUARD - (view.storage_offset() + (view.shape[0] - 1) * view.stride(0))


SPARSE_FROM = 1 << 26       # elements: from this size on a snapshot counts cells instead of copying them
_CHUNK = 1 << 27


class GuardSnapshot(NamedTuple):
    bits: Optional[torch.Tensor]    # the whole allocation's bit patterns when the snapshot was taken
    inside: Optional[torch.Tensor]  # bool, True for the cells of the view
    # allocations of SPARSE_FROM elements and more: no copy (bits, inside: None).  Every cell outside the view
    # held the sentinel when the snapshot was taken; the check counts the cells that no longer do.
    sparse: bool = False


def _flat_bits(view: torch.Tensor) -> torch.Tensor:
    flat = torch.empty(0, dtype=view.dtype, device=view.device).set_(view.untyped_storage())
    return flat.view(_BITS[view.element_size()])


def _view_offsets(view: torch.Tensor) -> torch.Tensor:
    """The element offset of every cell of ``view`` in its allocation."""
    off = torch.full((), view.storage_offset(), dtype=torch.int64, device=view.device)
    for n, s in zip(view.shape, view.stride()):
        off = off.unsqueeze(-1) + torch.arange(n, dtype=torch.int64, device=view.device) * s
    return off.flatten()


def _strays(view: torch.Tensor, want_first: int = 0):
    """Cells outside ``view`` that do not hold the sentinel: their number (and the offsets of the first few),
    chunk by chunk, without a mask of the allocation's size."""
    bits = _flat_bits(view)
    word = SENTINEL
    offs = _view_offsets(view)
    total = 0
    for lo in range(0, bits.numel(), _CHUNK):
        total += int((bits[lo:lo + _CHUNK] != word).sum())
    n = total - int((bits[offs] != word).sum())
    first = []
    if n and want_first:
        for lo in range(0, bits.numel(), _CHUNK):
            idx = (bits[lo:lo + _CHUNK] != word).nonzero().flatten() + lo
            idx = idx[~torch.isin(idx, offs)]
            first += idx[:want_first - len(first)].cpu().tolist()
            if len(first) >= want_first:
                break
    return n, first


def guard_snapshot(view: torch.Tensor) -> GuardSnapshot:
    """The bit pattern of every cell of ``view``'s allocation and which of them the view covers."""
    if view.dtype == torch.float32 and view.untyped_storage().nbytes() // 4 >= SPARSE_FROM:
        n, first = _strays(view, 8)
        if n:
            raise ValueError(f"guard_snapshot: {n} cell(s) outside the view hold no sentinel, first at {first}")
        return GuardSnapshot(None, None, True)
    bits = _flat_bits(view).clone()
    inside = torch.zeros(bits.numel(), dtype=torch.bool, device=view.device)
    inside.as_strided(tuple(view.shape), tuple(view.stride()), view.storage_offset()).fill_(True)
    return GuardSnapshot(bits, inside)


def assert_guards_intact(view: torch.Tensor, snap: GuardSnapshot, what: str = "output") -> None:
    """Every cell outside ``view`` is bitwise what it was at ``snap``."""
    if snap.sparse:
        n, first = _strays(view, 8)
        if n:
            base = view.storage_offset()
            raise AssertionError(f"{what}: {n} guard cell(s) overwritten outside a view of shape {tuple(view.shape)}, "
                                 f"strides {tuple(view.stride())}; first at element offsets "
                                 f"{[i - base for i in first]} from the view's base")
        return
    bad = (_flat_bits(view) != snap.bits) & ~snap.inside
    n = int(bad.sum())
    if n:
        idx = bad.nonzero().flatten()[:8].cpu().tolist()
        base = view.storage_offset()
        raise AssertionError(f"{what}: {n} guard cell(s) overwritten outside a view of shape {tuple(view.shape)}, "
                             f"strides {tuple(view.stride())}; first at element offsets "
                             f"{[i - base for i in idx]} from the view's base")


def alignment(view: torch.Tensor) -> int:
    """Largest power of two (bytes, up to 256) that divides the view's base address."""
    a = view.data_ptr()
    return 256 if a % 256 == 0 else a & -a
