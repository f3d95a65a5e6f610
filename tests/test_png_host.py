"""CPU tests of the PNG encoder's host side (csrc/png.hip, csrc/deflate_lengths.h), through ctypes as test_host.py:
the code-length builder the device runs per image, the 1106-bit block header, the size formulas and the argument
checks.  No GPU: none of these calls touches a device."""
import ctypes
import heapq
import struct
import zlib

import numpy as np
import pytest

import png_ref
from esmstereo_amd import _lib

lib = _lib.lib
RAW_LIMIT = 1 << 28


def code_lengths(hist) -> np.ndarray:
    h = (ctypes.c_uint32 * 257)(*[int(v) for v in hist])
    out = (ctypes.c_uint8 * 257)()
    assert lib.esm_deflate_code_lengths(h, out) == 0, lib.esm_last_error()
    return np.array(out[:], dtype=np.int64)


def huffman(counts):
    """(cost, depth) of an unrestricted Huffman tree of the positive ``counts`` (heapq: any optimal tree costs the same;
    the depth is the smallest one among them: ties go to the shallower subtree)."""
    heap = [(int(c), 0) for c in counts]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def _fibonacci_hist():
    h = np.zeros(257, dtype=np.int64)
    for v, n in png_ref.fibonacci_counts().items():
        h[v] = n
    return h


def _histograms():
    rng = np.random.default_rng(20240611)
    out = {}
    for k in range(24):
        present = rng.random(256) < rng.uniform(0.02, 1.0)
        scale = 10 ** rng.uniform(0, 6)
        h = np.zeros(257, dtype=np.int64)
        h[:256] = np.where(present, rng.integers(1, max(2, int(scale)), 256), 0)
        if not h[:256].any():
            h[int(rng.integers(256))] = 1
        if k % 3 == 0:  # a geometric tail: deep trees
            h[:256] = np.where(present, (1.7 ** (rng.permutation(256) % 34)).astype(np.int64), 0)
            h[int(rng.integers(256))] += 1
        out[f"random{k}"] = h
    h = np.full(257, 1000, dtype=np.int64)
    h[256] = 0
    out["all_equal"] = h
    h = np.zeros(257, dtype=np.int64)
    h[0] = 931875
    out["one_literal"] = h
    out["all_256_present"] = np.concatenate([np.arange(1, 257, dtype=np.int64) ** 2, [0]])
    out["fibonacci"] = _fibonacci_hist()
    h = np.zeros(257, dtype=np.int64)  # F(1) .. F(20), 17,710 in all: deep only under an unlucky tie-break
    h[3:23] = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765]
    out["fibonacci_from_two_ones"] = h
    h = np.zeros(257, dtype=np.int64)  # a Sub-filtered smooth map: a two-sided geometric distribution around 0
    for d in range(-40, 41):
        h[d % 256] += int(2.0e5 * 0.55 ** abs(d)) + (abs(d) < 30)
    out["laplace"] = h
    return out


HISTOGRAMS = _histograms()


@pytest.mark.parametrize("name", sorted(HISTOGRAMS))
def test_code_lengths_are_complete_limited_and_optimal(name):
    hist = HISTOGRAMS[name].copy()
    length = code_lengths(hist)
    counts = hist.copy()
    counts[256] = max(counts[256], 1)  # end-of-block is sent once
    used = length > 0
    assert length.max() <= 15
    assert int((1 << (15 - length[used])).sum()) == 1 << 15, "the code is not complete (Kraft sum != 1)"
    assert np.array_equal(used, counts > 0), "a zero count has a code, or a symbol that occurs has none"
    cost = int((counts * length).sum())
    flat = 8 * int(counts.sum()) + int(np.sort(counts)[:2].sum())  # 255 symbols of 8 bits, the two rarest 9
    assert cost <= flat
    best, depth = huffman(counts[counts > 0])
    print(f"{name}: {int(used.sum())} symbols, cost {cost}, Huffman {best} at depth {depth}, flat {flat}, "
          f"longest {length.max()}")
    assert cost >= best
    if depth <= 15:
        assert cost == best


def test_fibonacci_histogram_needs_limiting():
    """The case the prototype met on a real Sub-filtered map: the unrestricted tree is deeper than 15."""
    counts = _fibonacci_hist()
    counts[256] = 1
    assert (counts > 0).sum() >= 20 and counts.sum() < 30000
    assert huffman(counts[counts > 0])[1] > 15
    assert code_lengths(counts).max() == 15
    got = png_ref.fibonacci_map()
    raw = np.frombuffer(png_ref.filtered_u16(got, 0), dtype=np.uint8)
    assert np.array_equal(np.bincount(raw, minlength=256), _fibonacci_hist()[:256])


def _header(length):
    out = (ctypes.c_uint8 * 139)(*([0xFF] * 139))
    nbits = ctypes.c_int(-1)
    assert lib.esm_deflate_header((ctypes.c_uint8 * 257)(*[int(v) for v in length]), out, ctypes.byref(nbits)) == 0
    assert nbits.value == png_ref.HEADER_BITS == 1106
    return bytes(out)


def _stream_with_library_header(filtered: bytes, length) -> bytes:
    """78 01 | esm_deflate_header's 1106 bits | png_ref's body bit-packed behind them | Adler-32."""
    head = np.unpackbits(np.frombuffer(_header(length), dtype=np.uint8), bitorder="little")
    assert not head[1106:].any(), "the header's unused bits are not zero"
    bits = np.concatenate([head[:1106], png_ref.body_bits(filtered, length)])
    bits = np.concatenate([bits, np.zeros(-len(bits) % 8, dtype=np.uint8)])
    return b"\x78\x01" + np.packbits(bits, bitorder="little").tobytes() + struct.pack(">I", zlib.adler32(filtered))


def _smooth_u16(h, w, seed=3):
    y, x = np.mgrid[0:h, 0:w]
    d = 20 + 0.11 * x + 0.07 * y + 2 * np.sin(x / 9.0) + np.random.default_rng(seed).normal(0, 0.05, (h, w))
    return np.round(d * 256).astype(np.uint16)


@pytest.mark.parametrize("filt", [0, 1, 2])
def test_header_and_body_decode_with_zlib_and_pil(filt):
    Image = pytest.importorskip("PIL.Image")
    import io as _io

    a = _smooth_u16(37, 53)
    filtered = png_ref.filtered_u16(a, filt)
    length = code_lengths(np.concatenate([np.bincount(np.frombuffer(filtered, dtype=np.uint8), minlength=256), [1]]))
    stream = _stream_with_library_header(filtered, length)
    assert zlib.decompress(stream) == filtered
    assert stream == png_ref.encode(filtered, length)  # the reference's own header is the library's
    assert len(stream) <= lib.esm_png_stream_bound(len(filtered))
    png = png_ref.wrap(stream, 53, 37, 16, 0)
    assert np.array_equal(np.asarray(Image.open(_io.BytesIO(png))).astype(np.uint16), a)
    assert np.array_equal(png_ref.parse(png), a)


def test_rgb_reference_round_trip():
    Image = pytest.importorskip("PIL.Image")
    import io as _io

    a = np.random.default_rng(5).integers(0, 256, (9, 14, 3), dtype=np.uint8)
    for order in ("bgr", "rgb"):
        for filt in (0, 1, 2):
            filtered = png_ref.filtered_rgb8(a, order, filt)
            length = code_lengths(np.concatenate([np.bincount(np.frombuffer(filtered, dtype=np.uint8), minlength=256), [1]]))
            png = png_ref.wrap(png_ref.encode(filtered, length), 14, 9, 8, 2)
            rgb = a[:, :, ::-1] if order == "bgr" else a
            assert np.array_equal(np.asarray(Image.open(_io.BytesIO(png))), rgb)
            assert np.array_equal(png_ref.parse(png), rgb)


def test_header_rejects_bad_arguments():
    out = (ctypes.c_uint8 * 139)()
    ok = (ctypes.c_uint8 * 257)(*([8] * 257))
    assert lib.esm_deflate_header(None, out, None) == -1 and b"null" in lib.esm_last_error()
    assert lib.esm_deflate_header(ok, None, None) == -1
    ok[7] = 16
    assert lib.esm_deflate_header(ok, out, None) == -1 and b"15" in lib.esm_last_error()
    assert lib.esm_deflate_code_lengths(None, (ctypes.c_uint8 * 257)()) == -1
    assert lib.esm_deflate_code_lengths((ctypes.c_uint32 * 257)(), None) == -1
    assert lib.esm_deflate_code_lengths((ctypes.c_uint32 * 257)(*([1 << 31] * 2 + [0] * 255)),
                                        (ctypes.c_uint8 * 257)()) == -1


def test_stream_bound_covers_the_formula_and_is_monotone():
    C = lib.esm_png_chunk_bytes()
    assert C > 0
    sizes = sorted({1, 2, 3, 7, 8, 100, C - 1, C, C + 1, 3 * C + 5, 931875, 2796750, RAW_LIMIT - 1})
    prev = 0
    for raw in sizes:
        bound = lib.esm_png_stream_bound(raw)
        assert bound >= 2 + -(-(1106 + 9 * (raw + 1)) // 8) + 4
        assert bound >= prev and bound % 4 == 0
        prev = bound
    for raw in (0, -1, RAW_LIMIT, RAW_LIMIT + 1):
        assert lib.esm_png_stream_bound(raw) == -1
    # the worst stream: noise over all 256 values costs at most the flat code, which the bound is built on
    filtered = np.random.default_rng(1).integers(0, 256, 5000, dtype=np.uint8).tobytes()
    length = code_lengths(np.concatenate([np.bincount(np.frombuffer(filtered, dtype=np.uint8), minlength=256), [1]]))
    assert len(png_ref.encode(filtered, length)) <= lib.esm_png_stream_bound(5000)


def test_workspace_bytes_is_monotone_and_holds_the_histograms():
    C = lib.esm_png_chunk_bytes()
    prev = 0
    for rows, row_bytes in ((1, 2), (1, C - 2), (1, C - 1), (1, C), (4, C), (375, 2484), (750, 3726)):
        n = lib.esm_png_workspace_bytes(1, rows, row_bytes)
        chunks = -(-rows * (1 + row_bytes) // C)
        assert n >= chunks * (256 * 4 + 8 + 4) + 257 * 4 and n % 4 == 0  # histograms, Adler partials, offsets, table
        assert n >= prev
        prev = n
        assert lib.esm_png_workspace_bytes(3, rows, row_bytes) == 3 * n
    for bad in ((0, 1, 2), (1, 0, 2), (1, 1, 0), (-1, 1, 2), (1, 1 << 14, 1 << 14)):
        assert lib.esm_png_workspace_bytes(*bad) == -1


def test_encode_calls_reject_bad_arguments_before_touching_a_pointer():
    """Every refusal is decided with all pointers null (or a never-dereferenced address), on a machine with no GPU."""
    E, P = -1, 0x1000
    slot = lib.esm_png_stream_bound(4 * (1 + 2 * 5))

    def u16(src=None, B=1, h=4, w=5, work=None, out=None, stride=slot, lengths=None, filt=1):
        return lib.esm_png_encode_u16(src, B, h, w, work, out, stride, lengths, filt, None)

    def rgb8(B=1, h=4, w=5, stride=lib.esm_png_stream_bound(4 * 16), filt=1):
        return lib.esm_png_encode_rgb8(None, B, h, w, 1, None, None, stride, None, filt, None)

    def disp(Hp=8, Wp=8, top=2, left=3, h=4, w=5, filt=1, src=None):
        return lib.esm_png_encode_disp_f32(src, 1, Hp, Wp, top, left, h, w, src, src, slot, src, filt, None)

    for filt in (-1, 3, 4):
        assert u16(filt=filt) == E and b"filter" in lib.esm_last_error()
        assert rgb8(filt=filt) == E and b"filter" in lib.esm_last_error()
        assert disp(filt=filt) == E and b"filter" in lib.esm_last_error()
    for kw in ({"B": 0}, {"h": 0}, {"w": 0}, {"h": -3}):
        assert u16(**kw) == E and b"non-positive" in lib.esm_last_error()
        assert rgb8(**kw) == E and b"non-positive" in lib.esm_last_error()
    assert u16(stride=slot - 4) == E and b"bound" in lib.esm_last_error()
    assert rgb8(stride=16) == E and b"bound" in lib.esm_last_error()
    assert u16(h=1 << 14, w=1 << 13, stride=1 << 40) == E and b"2^28" in lib.esm_last_error()
    assert rgb8(h=1 << 14, w=1 << 13, stride=1 << 40) == E and b"2^28" in lib.esm_last_error()
    assert u16() == E and b"null" in lib.esm_last_error()
    assert rgb8() == E and b"null" in lib.esm_last_error()
    assert u16(src=P, work=P, out=P, lengths=None) == E and b"null" in lib.esm_last_error()
    assert u16(src=P, work=P, out=P + 2, lengths=P) == E and b"aligned" in lib.esm_last_error()
    assert u16(src=P, work=P, out=P, lengths=P, stride=slot + 2) == E and b"multiple of 4" in lib.esm_last_error()
    assert disp() == E and b"null" in lib.esm_last_error()
    for kw in ({"top": 5}, {"left": 4}, {"top": -1}, {"Hp": 0}):
        assert disp(src=P, **kw) == E and (b"window" in lib.esm_last_error() or b"non-positive" in lib.esm_last_error())


def test_python_entry_points_refuse_cpu_tensors():
    import torch

    from esmstereo_amd import io as eio, render

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eio.png_encode_u16(torch.zeros(1, 4, 5, dtype=torch.int16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eio.png_encode_disparity(torch.zeros(1, 8, 8), 2, 3, 4, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.png_encode_bgr8(torch.zeros(4, 5, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="filter"):
        eio._png_filter("paeth")


def _png_file(rows: bytes, w: int, h: int, bit_depth: int, color_type: int) -> bytes:
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))

    ihdr = struct.pack(">IIBBBBB", w, h, bit_depth, color_type, 0, 0, 0)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(rows, 6)) +
            chunk(b"IEND", b""))


def test_host_png_writers_file_bytes():
    """png_u16_bytes / png_rgb8_bytes byte for byte: the signature and three chunks framed here (CRC-32 over
    tag + data), around zlib level 6 of the filter-0 rows, independently of png_wrap."""
    from esmstereo_amd.io import png_u16_bytes
    from esmstereo_amd.render import png_rgb8_bytes

    rng = np.random.default_rng(7)
    a = rng.integers(0, 65536, (3, 5), dtype=np.uint16)
    a[0, 0], a[-1, -1] = 0, 65535
    rows = b"".join(b"\0" + a[r].astype(">u2").tobytes() for r in range(3))
    assert png_u16_bytes(a) == _png_file(rows, 5, 3, 16, 0)
    c = rng.integers(0, 256, (2, 3, 3), dtype=np.uint8)
    for order, rgb in (("rgb", c), ("bgr", c[:, :, ::-1])):
        rows = b"".join(b"\0" + np.ascontiguousarray(rgb[r]).tobytes() for r in range(2))
        assert png_rgb8_bytes(c, order) == _png_file(rows, 3, 2, 8, 2)
