"""CPU tests of the layout harness (tests/layouts.py): the views have the promised strides, alignment and
poisoned surroundings, and the guard check fails on a single overwritten cell next to a row end or between
channels.  These are the proof that the GPU layout tests fail on a kernel that writes one element too far."""
import pytest
import torch

import layouts as LY
from layouts import GUARD, SENTINEL, assert_guards_intact, embed, guard_snapshot

SHAPES = [(2, 5, 7, 19), (2, 12, 3, 7, 21), (1, 1, 9, 37), (3, 6, 4)]


def _data(shape):
    return torch.arange(1, 1 + torch.Size(shape).numel(), dtype=torch.float32).view(shape)


def _flat(v):
    return torch.empty(0, dtype=v.dtype).set_(v.untyped_storage())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("where", LY.PLACEMENTS)
def test_embed_values_margins_and_poison(shape, where):
    t = _data(shape)
    v = embed(t, where)
    assert v.shape == t.shape and torch.equal(v, t) and v.stride(-1) == 1
    flat = _flat(v)
    snap = guard_snapshot(v)
    assert int(snap.inside.sum()) == t.numel()
    # everything outside the view is the sentinel, which reads as NaN
    assert bool((flat.view(torch.int32)[~snap.inside] == SENTINEL).all())
    assert bool(torch.isnan(flat[~snap.inside]).all())
    # flat guards at both ends
    first = v.storage_offset()
    last = first + sum((n - 1) * s for n, s in zip(v.shape, v.stride()))
    assert first >= GUARD and flat.numel() - 1 - last >= GUARD
    # margins: columns >= 3, rows >= 2, (planes >= 1,) channels >= 3, batch >= 1 on both sides
    need = {3: (3, 2, 3), 4: (1, 3, 2, 3), 5: (1, 3, 1, 2, 3)}[t.dim()]
    st = v.stride()
    for ax, m in enumerate(need):
        outer = st[ax - 1] if ax else None
        assert st[ax] * (v.shape[ax] + 2 * m) <= (outer if outer is not None else flat.numel() - 2 * GUARD), (ax, st)
    for sign in (-1, 1):  # the margin cells themselves, at each corner of the view
        for ax, m in enumerate(need):
            corner = first if sign < 0 else last
            for step in range(1, m + 1):
                assert not bool(snap.inside[corner + sign * step * st[ax]]), (ax, step)


@pytest.mark.parametrize("shape", SHAPES)
def test_gapped16_keeps_vector_alignment(shape):
    v = embed(_data(shape), "gapped16")
    assert v.data_ptr() % 16 == 0 and v.storage_offset() % 4 == 0
    assert all(s % 4 == 0 for s in v.stride()[:-1])


@pytest.mark.parametrize("shape", SHAPES)
def test_odd_breaks_vector_alignment(shape):
    v = embed(_data(shape), "odd")
    assert LY.alignment(v) == 4 and v.stride(-2) % 2 == 1
    # column offset 3: the three cells before a row start are guard cells of the same padded row
    assert (v.storage_offset() - GUARD) % v.stride(-2) % 4 in (0, 1, 2, 3)
    rows = {(v.storage_offset() + y * v.stride(-2)) % 4 for y in range(4)}
    assert len(rows) == 4  # row starts take every 4-element phase: 16-byte paths must fall back


@pytest.mark.parametrize("where", LY.PLACEMENTS)
def test_planes_only_embedding(where):
    t = _data((2, 16, 6, 20))
    v = embed(t, where, spatial=False)
    assert torch.equal(v, t) and v.stride()[1:] == (120, 20, 1) and v.stride(0) == 120 * (16 + 6)
    assert LY.alignment(v) == (4 if where == "odd" else 256) or v.data_ptr() % 16 == 0
    assert (v.data_ptr() % 16 == 0) == (where == "gapped16")
    v3 = embed(_data((2, 16, 2, 6, 10)), where, spatial=False)  # rows of 10: only whole planes need the alignment
    assert v3.stride()[1:] == (120, 60, 10, 1) and (v3.data_ptr() % 16 == 0) == (where == "gapped16")
    with pytest.raises(ValueError):
        embed(_data((1, 2, 3, 5)), "gapped16", spatial=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.uint16])
def test_carved_is_contiguous_and_256_aligned(dtype):
    t = (torch.arange(3 * 5 * 19) % 251).to(dtype).view(3, 5, 19)
    v = embed(t, "carved")
    assert v.is_contiguous() and v.data_ptr() % 256 == 0 and v.dtype == dtype
    assert torch.equal(v.view(torch.uint8), t.view(torch.uint8))
    snap = guard_snapshot(v)
    assert int(snap.inside.sum()) == t.numel()
    assert v.storage_offset() >= GUARD and snap.bits.numel() - v.storage_offset() - t.numel() >= GUARD
    assert_guards_intact(v, snap)
    _flat(v)[v.storage_offset() + t.numel()] = 1  # the first cell past the block
    with pytest.raises(AssertionError, match="guard"):
        assert_guards_intact(v, snap)


@pytest.mark.parametrize("where", LY.PLACEMENTS)
def test_guard_check_catches_one_cell_past_a_row_end(where):
    v = embed(torch.zeros(2, 5, 7, 19), where)
    snap = guard_snapshot(v)
    # x = W of row (b 1, c 2, y 3): what a store masked one element short writes
    _flat(v)[v.storage_offset() + 1 * v.stride(0) + 2 * v.stride(1) + 3 * v.stride(2) + 19] = 0.0
    with pytest.raises(AssertionError, match="1 guard cell"):
        assert_guards_intact(v, snap)


@pytest.mark.parametrize("where", LY.PLACEMENTS)
def test_guard_check_catches_a_cell_between_channels(where):
    v = embed(torch.zeros(2, 5, 7, 19), where)
    snap = guard_snapshot(v)
    # row H of channel 1 (the margin between channels 1 and 2), written with the sentinel's own VALUE class
    # (a NaN with another payload): only a bitwise comparison sees it
    cell = v.storage_offset() + 1 * v.stride(1) + 7 * v.stride(2) + 4
    flat = _flat(v)
    assert bool(torch.isnan(flat[cell]))
    flat.view(torch.int32)[cell] = 0x7FC00001
    with pytest.raises(AssertionError, match="1 guard cell"):
        assert_guards_intact(v, snap)


@pytest.mark.parametrize("where", LY.PLACEMENTS + ("carved",))
def test_guard_check_passes_when_only_the_view_is_written(where):
    v = embed(torch.zeros(2, 5, 3, 7, 19), where)
    snap = guard_snapshot(v)
    v.copy_(torch.randn(2, 5, 3, 7, 19))
    v[1, 4, 2, 6, 18] = float("nan")
    assert_guards_intact(v, snap)


# ----------------------------------------------------------------------------- far placements (embed_far)

FAR_CASES = [  # (shape, axis, stride in elements, tail in bytes)
    ((2, 5, 7, 19), "c", 7 * 19 + 31 * 4 - 1 - (7 * 19 - 1) % 4, 0),
    ((2, 5, 7, 19), "c", 1024, 1 << 16),
    ((2, 1, 7, 19), "h", 64, 1 << 14),
    ((2, 3, 4, 7, 19), "d", 7 * 19 * 4, 4096),
    ((2, 3, 4, 7, 19), "h", 20, 0),
    ((2, 5, 7, 19), "b", 1 << 12, 1 << 15),
]


@pytest.mark.parametrize("shape,axis,stride,tail", FAR_CASES)
def test_embed_far_values_strides_poison_and_tail(shape, axis, stride, tail):
    t = _data(shape)
    v = LY.embed_far(t, axis, stride, tail_bytes=tail)
    axes = {4: "bchw", 5: "bcdhw"}[t.dim()]
    k = axes.index(axis)
    assert v.shape == t.shape and torch.equal(v, t)
    assert v.stride(k) == stride and v.storage_offset() == GUARD and v.data_ptr() % 16 == 0
    # every other axis packed: inside the named axis contiguous, outside it over entries padded to the stride
    st = v.stride()
    assert st[-1] == 1
    for i in range(t.dim() - 2, -1, -1):
        if i != k:
            assert st[i] == st[i + 1] * shape[i + 1], (i, st)
    flat = _flat(v)
    snap = guard_snapshot(v)
    assert int(snap.inside.sum()) == t.numel()
    assert bool((flat.view(torch.int32)[~snap.inside] == SENTINEL).all()) and bool(torch.isnan(flat[~snap.inside]).all())
    # the allocation: GUARD in front, and behind the base of every batch item at least the tail and the item itself
    item = sum((n - 1) * s for n, s in zip(shape[1:], st[1:])) + 1
    assert LY.far_tail_elems(v) == max(item, tail // 4)
    assert flat.numel() == GUARD + (shape[0] - 1) * st[0] + max(item, tail // 4) + GUARD
    # any offset below the tail from any item's base is a cell of this allocation: the sentinel, or the view
    for b in range(shape[0]):
        base = v.storage_offset() + b * st[0]
        for off in (item, tail // 4 - 1, (tail // 4) // 2 + 1):
            if 0 <= off < max(item, tail // 4) and not bool(snap.inside[base + off]):
                assert bool(torch.isnan(flat[base + off]))


def test_embed_far_refuses_overlap_and_misalignment():
    with pytest.raises(ValueError, match="overlaps"):
        LY.embed_far(_data((2, 5, 7, 19)), "c", 7 * 19 - 1 - (7 * 19 - 1) % 4)
    with pytest.raises(ValueError, match="multiple of 4"):
        LY.embed_far(_data((2, 5, 7, 19)), "c", 7 * 19 + 2)
    with pytest.raises(ValueError, match="axis"):
        LY.embed_far(_data((2, 5, 7, 19)), "d", 1024)


@pytest.mark.parametrize("sparse", [False, True], ids=["copy", "sparse"])
@pytest.mark.parametrize("shape,axis,stride,tail", FAR_CASES)
def test_far_guard_check_catches_strays(shape, axis, stride, tail, sparse, monkeypatch):
    """One cell past a row's end, one cell in the gap between two entries of the far axis and the last cell of the
    tail, each caught; writing the view itself is not.  ``sparse``: the snapshot that keeps no copy, which the GPU
    tests' allocations of several GiB take (forced here by lowering its threshold; small chunks)."""
    if sparse:
        monkeypatch.setattr(LY, "SPARSE_FROM", 1)
        monkeypatch.setattr(LY, "_CHUNK", 1000)
    t = _data(shape)
    axes = {4: "bchw", 5: "bcdhw"}[t.dim()]
    k = axes.index(axis)

    def fresh():
        v = LY.embed_far(t, axis, stride, tail_bytes=tail)
        snap = guard_snapshot(v)
        assert snap.sparse == sparse
        return v, snap, _flat(v)

    v, snap, flat = fresh()
    v.copy_(torch.randn(shape))
    v[tuple(n - 1 for n in shape)] = float("nan")
    assert_guards_intact(v, snap)
    last = v.storage_offset() + sum((n - 1) * s for n, s in zip(v.shape, v.stride()))
    row_end = v.storage_offset() + v.stride(0) + shape[-1]  # x = W of the first row of batch item 1
    gap = v.storage_offset() + v.stride(k) - 1              # the cell in front of entry 1 of the far axis
    for cell in (row_end, gap, last + 1, flat.numel() - GUARD - 1):
        v, snap, flat = fresh()
        inside = torch.zeros(flat.numel(), dtype=torch.bool)
        inside.as_strided(tuple(v.shape), tuple(v.stride()), v.storage_offset()).fill_(True)
        if bool(inside[cell]):
            continue  # (packed there: the cell belongs to the view)
        flat[cell] = 0.0
        with pytest.raises(AssertionError, match=rf"1 guard cell.*\[{cell - v.storage_offset()}\]"):
            assert_guards_intact(v, snap)


def test_sparse_snapshot_refuses_a_dirty_allocation(monkeypatch):
    monkeypatch.setattr(LY, "SPARSE_FROM", 1)
    v = LY.embed_far(_data((2, 5, 7, 19)), "c", 1024)
    _flat(v)[3] = 1.0
    with pytest.raises(ValueError, match="hold no sentinel"):
        guard_snapshot(v)


def test_far_arena_is_refilled_and_grows():
    """Views that share a FarArena: each take finds every cell outside the new view holding the sentinel again,
    whatever the last view and a stray store left; a larger request replaces the allocation."""
    arena = LY.FarArena("cpu")
    v = LY.embed_far(_data((2, 5, 7, 19)), "c", 1024, tail_bytes=1 << 16, arena=arena)
    first = arena.raw
    _flat(v)[5] = 1.0
    w = LY.embed_far(_data((2, 3, 7, 19)), "c", 512, arena=arena)
    assert arena.raw is first and w.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
    snap = guard_snapshot(w)
    flat = _flat(w)
    assert int(snap.inside.sum()) == w.numel() and bool((flat.view(torch.int32)[~snap.inside] == SENTINEL).all())
    assert torch.equal(w, _data((2, 3, 7, 19))) and LY.far_tail_elems(w) >= 2 * 512 + 7 * 19
    big = LY.embed_far(_data((2, 5, 7, 19)), "c", 4096, tail_bytes=1 << 20, arena=arena)
    assert arena.raw is not first and arena.raw.numel() == GUARD + 5 * 4096 + (1 << 18) + GUARD
    assert torch.equal(big, _data((2, 5, 7, 19)))
    arena.release()
    assert arena.raw is None
