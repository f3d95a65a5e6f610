"""numpy restatement of what csrc/png.hip writes, from the public formats alone (PNG 1.2 sections 6 and 9, RFC 1950, RFC 1951).

* ``filtered_u16`` / ``filtered_rgb8``: the filtered scanlines (filter byte, big-endian samples / R, G, B; None, Sub, Up).
* ``encode``: the zlib stream of the issue's fixed format, by a plain bit-at-a-time writer, for code lengths given as an
  argument (the library's): ``78 01``, the 1106-bit dynamic block header, canonical codes, end-of-block, padding, Adler-32.
* ``parse``: a PNG reader with its own un-filter (``zlib.decompress`` for the stream), giving the array back.
"""
import struct
import zlib

import numpy as np

FILTERS = {"none": 0, "sub": 1, "up": 2}
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEADER_BITS = 1106


def fibonacci_counts():
    """{byte value: count} over 20 byte values: the Fibonacci numbers F(2) .. F(21) = 1, 2, 3, 5, ..., 10946, 28,655
    in all.  With the one end-of-block as F(1) the counts are the whole Fibonacci sequence, whose Huffman tree is a
    chain 20 deep under EVERY tie-break (F(1) .. F(20) and an end-of-block still have an optimal tree of depth 11, which
    a shallowest-tree builder finds), so length limiting is active.  Byte 0 takes the largest count (the filter byte of
    a filter-0 row is a zero)."""
    fib = [1, 2]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    values = [0] + [13 * k + 3 for k in range(1, 20)]  # distinct, spread over the byte range
    return dict(zip(values, sorted(fib, reverse=True)))


def fibonacci_map(seed: int = 0) -> np.ndarray:
    """A one-row uint16 map [1, 14327] whose filter-0 scanline (28,655 bytes with the filter byte) has exactly
    ``fibonacci_counts()``, in seeded random order."""
    counts = fibonacci_counts()
    body = np.concatenate([np.full(n - (v == 0), v, dtype=np.uint8) for v, n in counts.items()])
    np.random.default_rng(seed).shuffle(body)
    return body.view(">u2").astype(np.uint16).reshape(1, -1)


def _filter_rows(rows: np.ndarray, bpp: int, filt: int) -> bytes:
    """rows: uint8 [h, n] of unfiltered scanlines -> the filtered scanlines with their filter bytes."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    h, n = rows.shape
    out = np.empty((h, 1 + n), dtype=np.uint8)
    out[:, 0] = filt
    if filt == 0:
        out[:, 1:] = rows
    elif filt == 1:
        left = np.zeros_like(rows)
        left[:, bpp:] = rows[:, :-bpp] if n > bpp else rows[:, :0]
        out[:, 1:] = rows - left  # uint8 arithmetic wraps modulo 256
    elif filt == 2:
        up = np.zeros_like(rows)
        up[1:] = rows[:-1]
        out[:, 1:] = rows - up
    else:
        raise ValueError(filt)
    return out.tobytes()


def filtered_u16(a: np.ndarray, filt: int) -> bytes:
    a = np.ascontiguousarray(a, dtype=np.uint16)
    h, w = a.shape
    return _filter_rows(a.astype(">u2").view(np.uint8).reshape(h, 2 * w), 2, filt)


def filtered_rgb8(a: np.ndarray, order: str, filt: int) -> bytes:
    a = np.asarray(a, dtype=np.uint8)
    h, w, _ = a.shape
    rgb = a[:, :, ::-1] if order == "bgr" else a
    return _filter_rows(np.ascontiguousarray(rgb).reshape(h, 3 * w), 3, filt)


def canonical_codes(lengths):
    """RFC 1951 section 3.2.2: {symbol: code} for the non-zero lengths."""
    lengths = [int(v) for v in lengths]
    bl_count = [0] * (max(lengths) + 2)
    for v in lengths:
        if v:
            bl_count[v] += 1
    code, next_code = 0, [0] * (max(lengths) + 2)
    for bits in range(1, max(lengths) + 1):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    codes = {}
    for sym, v in enumerate(lengths):
        if v:
            codes[sym] = next_code[v]
            next_code[v] += 1
    return codes


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value: int, n: int) -> None:
        """n bits of a plain integer field: least significant bit first."""
        self.bits.extend((value >> k) & 1 for k in range(n))

    def put_code(self, code: int, n: int) -> None:
        """a Huffman code: most significant bit first."""
        self.bits.extend((code >> k) & 1 for k in range(n - 1, -1, -1))

    def tobytes(self) -> bytes:
        b = np.array(self.bits + [0] * (-len(self.bits) % 8), dtype=np.uint8)
        return np.packbits(b, bitorder="little").tobytes()


def header(lengths, w: BitWriter) -> None:
    """The fixed-shape dynamic block header: literals only, 4-bit length codes."""
    w.put(1, 1)   # BFINAL
    w.put(2, 2)   # BTYPE 10: dynamic
    w.put(0, 5)   # HLIT: 257
    w.put(0, 5)   # HDIST: 1
    w.put(15, 4)  # HCLEN: 19
    for sym in CL_ORDER:
        w.put(4 if sym < 16 else 0, 3)
    # symbols 0-15 of the code-length code all have length 4: canonical code of symbol s is s
    for v in lengths:
        w.put_code(int(v), 4)
    w.put_code(1, 4)  # the one distance code, length 1


def body_bits(filtered: bytes, lengths) -> np.ndarray:
    """The bits of the coded symbols and end-of-block, as a uint8 array of 0 / 1 (vectorised: a map has ~10^5 symbols)."""
    codes = canonical_codes(lengths)
    lens = np.array([int(v) for v in lengths], dtype=np.int64)
    table = np.zeros(257, dtype=np.int64)
    for s, c in codes.items():
        table[s] = c
    syms = np.concatenate([np.frombuffer(filtered, dtype=np.uint8).astype(np.int64), [256]])
    assert (lens[syms] > 0).all(), "a symbol that occurs has no code"
    ln, cd = lens[syms], table[syms]
    start = np.concatenate([[0], np.cumsum(ln)])
    out = np.zeros(int(start[-1]), dtype=np.uint8)
    for k in range(15):  # bit k of every code, counted from its most significant bit
        has = ln > k
        out[start[:-1][has] + k] = (cd[has] >> (ln[has] - 1 - k)) & 1
    return out


def encode(filtered: bytes, lengths) -> bytes:
    """The whole zlib stream for ``filtered`` with the code ``lengths`` (257 values)."""
    w = BitWriter()
    header(lengths, w)
    assert len(w.bits) == HEADER_BITS
    bits = np.concatenate([np.array(w.bits, dtype=np.uint8), body_bits(filtered, lengths)])
    bits = np.concatenate([bits, np.zeros(-len(bits) % 8, dtype=np.uint8)])
    return b"\x78\x01" + np.packbits(bits, bitorder="little").tobytes() + struct.pack(">I", zlib.adler32(filtered))


def wrap(stream: bytes, width: int, height: int, bit_depth: int, color_type: int) -> bytes:
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, bit_depth, color_type, 0, 0, 0)) +
            chunk(b"IDAT", stream) + chunk(b"IEND", b""))


def split(png: bytes):
    """(ihdr fields, the concatenated IDAT payload) of a PNG file, every chunk's CRC checked."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG signature"
    pos, ihdr, idat, seen_end = 8, None, b"", False
    while pos < len(png):
        n, tag = struct.unpack(">I4s", png[pos:pos + 8])
        data = png[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xFFFFFFFF, f"CRC of {tag}"
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat += data
        elif tag == b"IEND":
            seen_end = True
        pos += 12 + n
    assert ihdr is not None and seen_end and pos == len(png)
    return ihdr, idat


def parse(png: bytes) -> np.ndarray:
    """The image of a non-interlaced 16-bit grayscale (-> uint16 [h, w]) or 8-bit RGB (-> uint8 [h, w, 3], R G B) PNG."""
    (w, h, depth, ctype, comp, fmethod, interlace), idat = split(png)
    assert (comp, fmethod, interlace) == (0, 0, 0)
    assert (depth, ctype) in ((16, 0), (8, 2)), (depth, ctype)
    bpp = 2 if ctype == 0 else 3
    n = bpp * w
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8)
    assert raw.size == h * (1 + n), "scanline bytes"
    raw = raw.reshape(h, 1 + n)
    rows = np.zeros((h, n), dtype=np.uint8)
    for y in range(h):
        f, line = int(raw[y, 0]), raw[y, 1:]
        if f == 0:
            rows[y] = line
        elif f == 1:  # Sub: every byte adds the byte bpp to its left of the RECONSTRUCTED row: bpp interleaved prefix sums
            for k in range(bpp):
                rows[y, k::bpp] = np.cumsum(line[k::bpp].astype(np.uint64)).astype(np.uint8)
        elif f == 2:
            rows[y] = line + (rows[y - 1] if y else 0)
        else:
            raise AssertionError(f"filter {f} is not written by this encoder")
    if ctype == 0:
        return rows.view(">u2").astype(np.uint16).reshape(h, w)
    return rows.reshape(h, w, 3)
