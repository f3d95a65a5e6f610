"""The JPEG definition of include/esmstereo_amd.h restated in numpy, one bit at a time: encoder, header, RIFF walker.

No GPU and no package code: the tables below are typed from ITU-T T.81 Annex K (K.1, K.2 quantisation, K.3-K.6
Huffman) and test_jpeg_host.py checks them against the DQT / DHT segments of a PIL-saved file.  Everything is plain
Python integers or int64 numpy, so ``>>`` is an arithmetic shift and ``//`` floors (divisions here are of
non-negative numbers only).
"""
import struct

import numpy as np

BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# zigzag position -> natural index (row * 8 + column)
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
          14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
          46, 53, 60, 61, 54, 47, 55, 62, 63]

# (class, id) -> (the 16 counts per code length, the values in code order)
HUFF = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
             [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22,
              0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33,
              0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34,
              0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
              0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76,
              0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96,
              0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5,
              0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
              0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1,
              0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13,
              0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62,
              0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29,
              0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54,
              0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
              0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94,
              0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3,
              0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2,
              0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA,
              0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]),
}


def dct_matrix() -> np.ndarray:
    k, n = np.mgrid[0:8, 0:8]
    c = np.where(k == 0, 1 / np.sqrt(2), 1.0)
    return np.round(8192 * 0.5 * c * np.cos((2 * n + 1) * k * np.pi / 16)).astype(np.int64)


M = dct_matrix()


def quant_table(quality: int, which: int) -> list:
    """64 entries in natural order; which 0 luminance, 1 chrominance."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * s + 50) // 100, 1), 255) for b in (BASE_CHROMA if which else BASE_LUMA)]


def huff_codes(cls: int, ident: int) -> dict:
    """{value: (code, length)} of the canonical code (T.81 Annex C)."""
    bits, vals = HUFF[cls, ident]
    out, code, i = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[i]] = (code, length)
            code += 1
            i += 1
        code <<= 1
    return out


def header(w: int, h: int, quality: int, subsampling: int, ri: int) -> bytes:
    out = b"\xff\xd8" + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for which in (0, 1):
        q = quant_table(quality, which)
        out += b"\xff\xdb\x00\x43" + bytes([which]) + bytes(q[ZIGZAG[i]] for i in range(64))
    sf = {420: 0x22, 444: 0x11}[subsampling]
    out += b"\xff\xc0\x00\x11\x08" + struct.pack(">HH", h, w) + bytes([3, 1, sf, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls, ident in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = HUFF[cls, ident]
        out += b"\xff\xc4" + struct.pack(">H", 19 + len(vals)) + bytes([cls << 4 | ident]) + bytes(bits) + bytes(vals)
    out += b"\xff\xdd\x00\x04" + struct.pack(">H", ri)
    return out + b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"


def planes(rgb: np.ndarray, subsampling: int):
    """Padded Y, Cb, Cr planes (int64) of uint8 [H, W, 3] in R, G, B order; chroma halved for 420."""
    m = 16 if subsampling == 420 else 8
    h, w, _ = rgb.shape
    a = np.pad(rgb, ((0, -h % m), (0, -w % m), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    if subsampling == 420:
        cb, cr = ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2 for c in (cb, cr))
    return y, cb, cr


def quantised_block(block: np.ndarray, q: list, guard_hits: list = None) -> list:
    """The 64 quantised coefficients of an 8x8 block of samples 0..255, in zigzag order."""
    s = block.astype(np.int64) - 128
    t = (s @ M.T + 512) >> 10           # t[y][u] = sum_n M[u][n] s[y][n]
    c8 = (M @ t + 4096) >> 13           # c8[v][u] = sum_y M[v][y] t[y][u]
    out = []
    for i in range(64):
        c, d = int(c8.flat[ZIGZAG[i]]), q[ZIGZAG[i]]
        v = (abs(c) + 4 * d) // (8 * d)
        v = -v if c < 0 else v
        if i > 0 and abs(v) > 1023:
            if guard_hits is not None:
                guard_hits.append(v)
            v = max(min(v, 1023), -1023)
        out.append(v)
    return out


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value: int, nbits: int):
        for k in range(nbits - 1, -1, -1):
            self.acc = self.acc << 1 | ((value >> k) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc, self.n = 0, 0

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)

    def marker(self, m: int):
        self.out += bytes([0xFF, m])


def _value_bits(v: int):
    size = abs(v).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


def encode_block(bw: BitWriter, zz: list, pred: int, dc: dict, ac: dict):
    size, bits = _value_bits(zz[0] - pred)
    bw.put(*dc[size])
    bw.put(bits, size)
    run = 0
    for i in range(1, 64):
        if zz[i] == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        size, bits = _value_bits(zz[i])
        bw.put(*ac[run << 4 | size])
        bw.put(bits, size)
        run = 0
    if zz[63] == 0:
        bw.put(*ac[0x00])


def encode_scan(rgb: np.ndarray, quality: int = 75, subsampling: int = 420, ri: int = 8, guard_hits=None) -> bytes:
    """The entropy-coded scan of uint8 [H, W, 3] (R, G, B), restart markers and EOI included."""
    y, cb, cr = planes(rgb, subsampling)
    ql, qc = quant_table(quality, 0), quant_table(quality, 1)
    tables = [(huff_codes(0, 0), huff_codes(1, 0)), (huff_codes(0, 1), huff_codes(1, 1))]
    m = 16 if subsampling == 420 else 8
    rows, cols = y.shape[0] // m, y.shape[1] // m
    bw, pred = BitWriter(), [0, 0, 0]
    for n in range(rows * cols):
        if n > 0 and n % ri == 0:
            bw.pad()
            bw.marker(0xD0 + ((n // ri - 1) & 7))
            pred = [0, 0, 0]
        my, mx = divmod(n, cols)
        blocks = []
        if subsampling == 420:
            for by in (0, 1):
                for bx in (0, 1):
                    blocks.append((0, y[16 * my + 8 * by:16 * my + 8 * by + 8, 16 * mx + 8 * bx:16 * mx + 8 * bx + 8]))
        else:
            blocks.append((0, y[8 * my:8 * my + 8, 8 * mx:8 * mx + 8]))
        blocks.append((1, cb[8 * my:8 * my + 8, 8 * mx:8 * mx + 8]))
        blocks.append((2, cr[8 * my:8 * my + 8, 8 * mx:8 * mx + 8]))
        for comp, blk in blocks:
            zz = quantised_block(blk, qc if comp else ql, guard_hits)
            dc, ac = tables[1 if comp else 0]
            encode_block(bw, zz, pred[comp], dc, ac)
            pred[comp] = zz[0]
    bw.pad()
    bw.marker(0xD9)
    return bytes(bw.out)


def encode(img: np.ndarray, quality: int = 75, subsampling: int = 420, ri: int = 8, order: str = "rgb") -> bytes:
    """The complete JFIF file of uint8 [H, W, 3] whose channels are in ``order``."""
    rgb = img[:, :, ::-1] if order == "bgr" else img
    h, w, _ = rgb.shape
    return header(w, h, quality, subsampling, ri) + encode_scan(rgb, quality, subsampling, ri)


def anchor_picture(h: int, w: int) -> np.ndarray:
    """img[y, x] = ((5x + 3y) & 255, (x y) & 255, 255 y // max(H - 1, 1)), in R, G, B."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(5 * x + 3 * y) & 255, (x * y) & 255, 255 * y // max(h - 1, 1)], axis=-1).astype(np.uint8)


def smooth_noise_picture(h: int, w: int, seed: int = 0, amp: int = 12) -> np.ndarray:
    """A smooth colour field plus uniform noise of +-amp, uint8 [H, W, 3]."""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(x / 7.0 + y / 11.0), 128 + 80 * np.cos(x / 5.0 - y / 9.0),
                     40 + 170.0 * (x + y) / max(h + w - 2, 1)], axis=-1)
    noise = np.random.default_rng(seed).integers(-amp, amp + 1, (h, w, 3))
    return np.clip(np.rint(base) + noise, 0, 255).astype(np.uint8)


def basis_sign_picture(k: int) -> np.ndarray:
    """An 8x8 grey block whose samples are 255 where DCT basis function k (v = k // 8, u = k % 8) is positive and 0
    elsewhere: the largest coefficient k a block can have."""
    v, u = divmod(k, 8)
    b = np.outer(M[v], M[u])
    g = np.where(b >= 0, 255, 0).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


# ---- RIFF
def riff_walk(data: bytes, pos: int = 0, end: int = None) -> list:
    """[(fourcc, offset of the chunk's data, size, children or None)]; RIFF and LIST chunks carry their form type as
    ``fourcc + b':' + type`` and are walked.  Raises on a chunk that passes its parent or on an odd offset."""
    end = len(data) if end is None else end
    out = []
    while pos < end:
        if pos + 8 > end:
            raise ValueError(f"riff: chunk header at {pos} passes the end {end}")
        if pos % 2:
            raise ValueError(f"riff: chunk at odd offset {pos}")
        cc, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        if pos + 8 + size > end:
            raise ValueError(f"riff: chunk {cc!r} at {pos} of {size} bytes passes the end {end}")
        if cc in (b"RIFF", b"LIST"):
            out.append((cc + b":" + data[pos + 8:pos + 12], pos + 8, size, riff_walk(data, pos + 12, pos + 8 + size)))
        else:
            out.append((cc, pos + 8, size, None))
        pos += 8 + size + (size & 1)
    return out


def riff_find(tree: list, name: bytes):
    for node in tree:
        if node[0] == name:
            return node
        if node[3] is not None:
            hit = riff_find(node[3], name)
            if hit is not None:
                return hit
    return None
