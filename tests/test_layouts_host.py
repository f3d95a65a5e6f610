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
