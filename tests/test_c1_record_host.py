"""c1_record_pack and c1_tile (csrc/conv_c1_rec.h) through their exported hooks esm_c1_record_pack and
esm_c1_record_tile: the 16-dword first-load record of the 2-D single-output-channel ConvTranspose.  Host only: the
hooks read the descriptor's fields and never its pointers.

Checked: every field survives the round trip at its maximum, the stride of a one-entry axis is stored as 0; the slab
bit and the grid dwords are set only with the hint, within 16-bit grid extents and while workgroups x extent <= 2^32
(where the reciprocals divide exactly); the tile of every workgroup equals a model of common.h's xcd_block and the map
is a bijection onto the grid."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esmstereo_amd._lib import EsmConvDesc, HINT_XCD_SLAB, lib  # noqa: E402

FIELDS = ("src", "w", "sb", "sc", "sh", "Hi", "Wi", "Cin", "cin_pad", "cout_pad", "slab", "gx", "gy", "nwg", "m_gx",
          "m_gy")
SRC, W = 0x7F0000001000, 0x7E0000002000  # never dereferenced


def magic(d: int) -> int:
    return 0 if d <= 1 else ((1 << 32) + d - 1) // d


def desc(cin=8, hi=24, wi=78, sb=None, sc=None, sh=None, cin_pad=16, cout_pad=32, hint=HINT_XCD_SLAB) -> EsmConvDesc:
    d = EsmConvDesc()
    d.nsrc, d.B, d.Cin, d.Cout = 1, 2, cin, 1
    d.Di, d.Hi, d.Wi, d.Do, d.Ho, d.Wo = 1, hi, wi, 1, 2 * hi, 2 * wi
    d.kd, d.kh, d.kw, d.stride, d.transposed, d.ph, d.pw = 1, 4, 4, 2, 1, 1, 1
    d.cin_pad, d.cout_pad = cin_pad, cout_pad
    d.src[0].ptr, d.src[0].C = SRC, cin
    d.src[0].sh = wi if sh is None else sh
    d.src[0].sc = hi * wi if sc is None else sc
    d.src[0].sb = cin * hi * wi if sb is None else sb
    d.w, d.hint = W, hint
    return d


def pack(d: EsmConvDesc, grid):
    rec = (ctypes.c_uint32 * 16)()
    fields = (ctypes.c_int64 * 16)()
    assert lib.esm_c1_record_pack(ctypes.byref(d), (ctypes.c_uint32 * 3)(*grid), rec, fields) == 1
    return rec, dict(zip(FIELDS, fields))


def tile(rec, bx, by, bz):
    xyz = (ctypes.c_int32 * 3)()
    assert lib.esm_c1_record_tile(rec, bx, by, bz, xyz) == 1
    return tuple(xyz)


def xcd_block(orig: int, grid):
    """common.h xcd_block: XCD k (the workgroups dispatched as k mod 8) runs a contiguous range of logical tiles."""
    gx, gy, gz = grid
    nwg = gx * gy * gz
    q, r, xcd = nwg // 8, nwg % 8, orig % 8
    wg = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + orig // 8
    return wg % gx, wg // gx % gy, wg // (gx * gy)


def test_every_field_at_its_maximum():
    big = (1 << 31) - 1
    d = desc(cin=255, hi=big, wi=big, sb=(1 << 63) - 1, sc=big, sh=big, cin_pad=16 * 0xFFFF, cout_pad=32 * 0xFFFF)
    rec, f = pack(d, (3, 5, 2))
    assert rec[0] | rec[1] << 32 == SRC and rec[2] | rec[3] << 32 == W
    assert f == dict(src=SRC, w=W, sb=(1 << 63) - 1, sc=big, sh=big, Hi=big, Wi=big, Cin=255, cin_pad=16 * 0xFFFF,
                     cout_pad=32 * 0xFFFF, slab=1, gx=3, gy=5, nwg=30, m_gx=magic(3), m_gy=magic(5))
    assert rec[10] >> 9 == 0  # the spare bits stay clear


def test_stride_of_a_one_entry_axis_is_zero():
    _, f = pack(desc(cin=1, hi=6, sc=1234, sh=78), (1, 1, 1))
    assert (f["sc"], f["sh"]) == (0, 78)
    _, f = pack(desc(cin=8, hi=1, sc=1234, sh=5678), (1, 1, 1))
    assert (f["sc"], f["sh"]) == (1234, 0)


@pytest.mark.parametrize("grid", [(3, 5, 2), (65535, 1, 1)])
def test_slab_within_the_limits(grid):
    rec, f = pack(desc(), grid)
    nwg = grid[0] * grid[1] * grid[2]
    assert nwg * max(grid[:2]) <= 1 << 32
    assert (f["slab"], f["gx"], f["gy"], f["nwg"], f["m_gx"], f["m_gy"]) == (1, grid[0], grid[1], nwg, magic(grid[0]),
                                                                           magic(grid[1]))
    assert list(rec[12:16]) == [grid[0] | grid[1] << 16, nwg, magic(grid[0]), magic(grid[1])]


@pytest.mark.parametrize("grid, hint", [((3, 5, 2), 0),                     # no hint
                                        ((65536, 1, 1), HINT_XCD_SLAB),     # grid x past 16 bits
                                        ((65535, 2, 1), HINT_XCD_SLAB)])    # 131070 x 65535 > 2^32
def test_slab_refused(grid, hint):
    if grid == (65535, 2, 1):
        assert 131070 * 65535 > 1 << 32
    rec, f = pack(desc(hint=hint), grid)
    assert (f["slab"], f["gx"], f["gy"], f["nwg"], f["m_gx"], f["m_gy"]) == (0, 0, 0, 0, 0, 0)
    assert rec[10] >> 8 == 0 and list(rec[12:16]) == [0, 0, 0, 0]
    for b in [(0, 0, 0), (grid[0] - 1, grid[1] - 1, grid[2] - 1)]:
        assert tile(rec, *b) == b  # dispatch order


@pytest.mark.parametrize("grid", [(1, 1, 1), (8, 1, 1), (3, 5, 2), (7, 1, 3)])
def test_tile_map_is_xcd_block_and_a_bijection(grid):
    gx, gy, gz = grid
    rec, _ = pack(desc(), grid)
    seen = set()
    for bz in range(gz):
        for by in range(gy):
            for bx in range(gx):
                t = tile(rec, bx, by, bz)
                assert t == xcd_block(bx + gx * (by + gy * bz), grid), (bx, by, bz)
                seen.add(t)
    assert seen == {(x, y, z) for x in range(gx) for y in range(gy) for z in range(gz)}
    rec, _ = pack(desc(hint=0), grid)
    assert all(tile(rec, bx, by, bz) == (bx, by, bz) for bz in range(gz) for by in range(gy) for bx in range(gx))


def test_tile_map_at_the_largest_slab_grid():
    """(65535, 1, 1): the first and last workgroup and both sides of each of the seven XCD range boundaries."""
    grid = (65535, 1, 1)
    rec, f = pack(desc(), grid)
    assert f["slab"] == 1
    q, r = divmod(65535, 8)
    starts = [k * (q + 1) if k < r else r * (q + 1) + (k - r) * q for k in range(9)]  # XCD k runs [starts[k], starts[k + 1])
    assert starts[0] == 0 and starts[8] == 65535
    inverse = {}
    for k in range(8):
        for j in range(starts[k + 1] - starts[k]):
            inverse[starts[k] + j] = k + 8 * j  # logical tile -> dispatch index
    assert sorted(inverse.values()) == list(range(65535))
    logical = [0, 65534] + [s + e for s in starts[1:8] for e in (-1, 0)]
    origs = {0, 65534} | {inverse[t] for t in logical}
    for orig in sorted(origs):
        t = tile(rec, orig, 0, 0)
        assert t == xcd_block(orig, grid), orig
        assert inverse[t[0]] == orig and t[1:] == (0, 0)
    assert {tile(rec, inverse[t], 0, 0)[0] for t in logical} == set(logical)
