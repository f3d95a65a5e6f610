"""The JPEG definition without a GPU: tests/jpeg_ref.py against its anchors and PIL, the library's host-only calls
(quantisation tables, header, bound, argument checks) against jpeg_ref, and the AVI writer's layout.

The anchors are five (size, quality, subsampling, Ri) rows recorded with the definition: file length, scan length and
the CRC-32 of the file that an independent numpy restatement of it gave for jpeg_ref.anchor_picture.  They pin
jpeg_ref; the GPU
tests (test_gpu_jpeg.py) then hold the device bytes to jpeg_ref.

PSNR bound: the definition's DCT and colour conversion are fixed-point restatements of what libjpeg computes, so a
decoded file can differ from PIL's own encode of the same picture only by rounding; the condition is PSNR(ours) >=
PSNR(PIL) - 0.25 dB at the same quality and subsampling (worst measured: -0.03 dB, 40 x 56 at quality 95 / 420).
"""
import ctypes
import io as _io
import struct
import zlib

import numpy as np
import pytest

import jpeg_ref
from esmstereo_amd import _lib
from esmstereo_amd.video import MjpegWriter

lib = _lib.lib
E = -1  # ESM_ERR_ARG
P = 0x1000  # a non-null address that is never dereferenced: every call it goes to is refused before any device work

ANCHORS = [  # h, w, quality, subsampling, Ri, file bytes, scan bytes without EOI, CRC-32 of the file
    (37, 50, 75, 420, 8, 1767, 1136, 0xDB46B121),
    (37, 50, 75, 444, 3, 2197, 1566, 0xA9B47CF0),
    (16, 16, 100, 420, 1, 787, 156, 0x7BEA1431),
    (1, 1, 50, 444, 16, 634, 3, 0x29078D01),
    (33, 129, 90, 420, 16, 4134, 3503, 0x6BD66277),
]
QUALITIES = (1, 10, 25, 50, 75, 90, 95, 100)
PIL_SUB = {420: 2, 444: 0}


def lib_header(w, h, quality, sub, ri, cap=1024) -> bytes:
    buf = (ctypes.c_uint8 * max(cap, 1))()
    n = lib.esm_jpeg_header(buf, cap, w, h, quality, sub, ri)
    assert n > 0, lib.esm_last_error()
    return bytes(buf[:n])


def pil_save(rgb: np.ndarray, quality: int, sub: int) -> bytes:
    Image = pytest.importorskip("PIL.Image")
    b = _io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=PIL_SUB[sub])
    return b.getvalue()


def pil_open(data: bytes) -> np.ndarray:
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(_io.BytesIO(data)).convert("RGB"))


def segments(data: bytes):
    """[(marker, payload)] of a JPEG file up to its scan."""
    out, pos = [], 2
    while data[pos + 1] != 0xDA:
        size = struct.unpack_from(">H", data, pos + 2)[0]
        out.append((data[pos + 1], data[pos + 4:pos + 2 + size]))
        pos += 2 + size
    return out


def dht_tables(data: bytes) -> dict:
    """{(class, id): (bits, vals)} of every table of every DHT segment."""
    out = {}
    for marker, body in segments(data):
        pos = 0
        while marker == 0xC4 and pos < len(body):
            bits = list(body[pos + 1:pos + 17])
            out[body[pos] >> 4, body[pos] & 15] = (bits, list(body[pos + 17:pos + 17 + sum(bits)]))
            pos += 17 + sum(bits)
    return out


@pytest.mark.parametrize("row", ANCHORS, ids=lambda r: f"{r[0]}x{r[1]}-q{r[2]}-{r[3]}-ri{r[4]}")
def test_reference_reproduces_the_anchors(row):
    h, w, quality, sub, ri, nfile, nscan, crc = row
    data = jpeg_ref.encode(jpeg_ref.anchor_picture(h, w), quality, sub, ri)
    head = jpeg_ref.header(w, h, quality, sub, ri)
    assert len(head) == 629 and data.startswith(head) and data.endswith(b"\xff\xd9")
    assert (len(data), len(data) - len(head) - 2, zlib.crc32(data)) == (nfile, nscan, crc)


def test_dct_matrix_rows():
    assert list(jpeg_ref.M[0]) == [2896] * 8
    assert list(jpeg_ref.M[1]) == [4017, 3406, 2276, 799, -799, -2276, -3406, -4017]
    assert list(jpeg_ref.M[2]) == [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784]
    assert list(jpeg_ref.M[7]) == [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]


@pytest.mark.parametrize("quality", QUALITIES)
def test_quant_tables_equal_pil(quality):
    Image = pytest.importorskip("PIL.Image")
    pil = Image.open(_io.BytesIO(pil_save(jpeg_ref.anchor_picture(16, 16), quality, 420))).quantization
    for which in (0, 1):
        out = (ctypes.c_uint8 * 64)()
        assert lib.esm_jpeg_quant_table(quality, which, out) == 0
        assert list(out) == jpeg_ref.quant_table(quality, which) == list(pil[which])


def test_huffman_tables_equal_pil_dht():
    """A non-optimised PIL file carries the Annex K.3 tables; so do jpeg_ref and the library's header."""
    pil = dht_tables(pil_save(jpeg_ref.anchor_picture(16, 16), 75, 420))
    assert sorted(pil) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    mine = dht_tables(lib_header(16, 16, 75, 420, 8))
    for key, (bits, vals) in pil.items():
        assert (bits, vals) == tuple(jpeg_ref.HUFF[key]) == mine[key]
        assert len(vals) == (162 if key[0] else 12)


@pytest.mark.parametrize("sub", (420, 444))
def test_header_equals_reference(sub):
    for (w, h, quality, ri) in ((50, 37, 75, 8), (1, 1, 1, 1), (65535, 9, 100, 16), (1242, 750, 90, 3)):
        got = lib_header(w, h, quality, sub, ri)
        assert got == jpeg_ref.header(w, h, quality, sub, ri) and len(got) == 629
    assert [m for m, _ in segments(lib_header(8, 8, 75, sub, 8))] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4,
                                                                      0xDD]
    assert lib_header(8, 8, 75, sub, 8, cap=629) == jpeg_ref.header(8, 8, 75, sub, 8)


@pytest.mark.parametrize("sub", (420, 444))
def test_reference_files_open_with_pil(sub):
    for (h, w) in ((1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (40, 56)):
        for quality, ri in ((50, 1), (75, 3), (95, 16)):
            got = pil_open(jpeg_ref.encode(jpeg_ref.smooth_noise_picture(h, w), quality, sub, ri))
            assert got.shape == (h, w, 3)


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("sub", (420, 444))
@pytest.mark.parametrize("quality", (50, 75, 95))
@pytest.mark.parametrize("size", ((17, 33), (40, 56), (37, 50)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_psnr_against_pil(size, quality, sub):
    a = jpeg_ref.smooth_noise_picture(*size)
    ours = psnr(pil_open(jpeg_ref.encode(a, quality, sub, 8)), a)
    pils = psnr(pil_open(pil_save(a, quality, sub)), a)
    print(f"{size} q{quality} {sub}: ours {ours:.3f} dB, PIL {pils:.3f} dB, difference {ours - pils:+.3f}")
    assert ours >= pils - 0.25


def test_argument_errors_without_gpu():
    out = (ctypes.c_uint8 * 64)()
    buf = (ctypes.c_uint8 * 1024)()
    assert lib.esm_jpeg_quant_table(75, 0, None) == E and b"null" in lib.esm_last_error()
    for quality in (0, 101, -5):
        assert lib.esm_jpeg_quant_table(quality, 0, out) == E and b"quality" in lib.esm_last_error()
    for which in (-1, 2):
        assert lib.esm_jpeg_quant_table(75, which, out) == E

    def header(b=buf, cap=1024, w=50, h=37, quality=75, sub=420, ri=8):
        return lib.esm_jpeg_header(b, cap, w, h, quality, sub, ri)

    def bound(h=37, w=50, sub=420, ri=8):
        return lib.esm_jpeg_stream_bound(h, w, sub, ri)

    def workspace(B=1, h=37, w=50, sub=420, ri=8):
        return lib.esm_jpeg_workspace_bytes(B, h, w, sub, ri)

    def encode(src=P, B=1, h=37, w=50, bgr=0, quality=75, sub=420, ri=8, work=P, out=P, slot=4096, lengths=P):
        return lib.esm_jpeg_encode_rgb8(src, B, h, w, bgr, quality, sub, ri, work, out, slot, lengths, None)

    assert header() == 629 and bound() > 0 and workspace() > 0
    assert header(b=None) == E and b"null" in lib.esm_last_error()
    assert header(cap=628) == E and b"629" in lib.esm_last_error()
    assert header(quality=0) == E and header(quality=101) == E
    for name in ("src", "work", "out", "lengths"):
        assert encode(**{name: None}) == E and b"null" in lib.esm_last_error()
    assert encode(quality=0) == E and encode(quality=101) == E and b"quality" in lib.esm_last_error()
    assert encode(slot=1) == E and b"slot" in lib.esm_last_error()
    assert encode(work=P + 4) == E and b"aligned" in lib.esm_last_error()
    assert encode(B=0) == E and encode(B=65536) == E and workspace(B=0) == E and workspace(B=65536) == E
    for call in (header, bound, workspace, encode):  # the limits every call shares
        for bad in (dict(h=0), dict(w=0), dict(h=65536), dict(w=65536), dict(h=-1), dict(sub=422), dict(sub=0),
                    dict(ri=0), dict(ri=17), dict(h=65535, w=65535)):
            assert call(**bad) == E, (call.__name__, bad)
    assert bound(h=65535, w=10922) > 0 and bound(h=65535, w=10923) == E and b"2^31" in lib.esm_last_error()


def test_stream_bound_formula_and_noise_at_quality_100():
    """2 ceil(n * blocks * 1658 / 8) + 2 per interval of n MCUs; the reference scan of noise at quality 100 (the longest
    scans there are: 1.4 x raw at 444) stays below it."""
    assert lib.esm_jpeg_stream_bound(1, 1, 444, 16) == 2 * ((3 * 1658 + 7) // 8) + 2
    full, tail = 2 * ((48 * 1658 + 7) // 8) + 2, 2 * ((18 * 1658 + 7) // 8) + 2  # 27 MCUs: 8 + 8 + 8 + 3
    assert lib.esm_jpeg_stream_bound(33, 129, 420, 8) == 3 * full + tail
    assert lib.esm_jpeg_workspace_bytes(3, 33, 129, 420, 8) == 3 * 4 * 12
    rng = np.random.default_rng(3)
    for (h, w, sub, ri) in ((48, 64, 444, 8), (17, 33, 420, 1), (16, 24, 444, 16)):
        noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        scan = jpeg_ref.encode_scan(noise, 100, sub, ri)
        assert len(scan) <= lib.esm_jpeg_stream_bound(h, w, sub, ri)
        if (h, w) == (48, 64):
            assert len(scan) > 3 * h * w  # the overflow case of the GPU test: longer than the raw frame


def test_avi_of_three_frames(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    h, w = 17, 33
    pics = [jpeg_ref.smooth_noise_picture(h, w, seed) for seed in range(3)]
    files = [jpeg_ref.encode(p, 75, 420, 8) for p in pics]
    if all(len(f) % 2 == 0 for f in files):  # one odd-length frame, whatever the encoder gave
        files[1] = files[1][:-2] + b"\xff\xff\xd9"  # (a fill byte in front of EOI: still a valid file)
    assert any(len(f) % 2 for f in files)
    path = str(tmp_path / "three.avi")
    with MjpegWriter(path, fps=25, quality=75) as wr:
        for f in files:
            wr.write_jpeg(f)
        with pytest.raises(ValueError, match="frames"):
            wr.write_jpeg(jpeg_ref.encode(jpeg_ref.anchor_picture(8, 8), 75, 420, 8))
    data = open(path, "rb").read()
    tree = jpeg_ref.riff_walk(data)
    assert len(tree) == 1 and tree[0][0] == b"RIFF:AVI " and tree[0][2] == len(data) - 8
    assert [n[0] for n in tree[0][3]] == [b"LIST:hdrl", b"LIST:movi", b"idx1"]
    hdrl = tree[0][3][0][3]
    assert [n[0] for n in hdrl] == [b"avih", b"LIST:strl"] and [n[0] for n in hdrl[1][3]] == [b"strh", b"strf"]
    _, off, size, _ = jpeg_ref.riff_find(tree, b"avih")
    avih = struct.unpack_from("<14I", data, off)
    assert size == 56 and avih[0] == 40000 and avih[3] & 0x10 and avih[4] == 3 and avih[6] == 1
    assert avih[7] == max(len(f) for f in files) and (avih[8], avih[9]) == (w, h)
    _, off, size, _ = jpeg_ref.riff_find(tree, b"strh")
    assert size == 56 and data[off:off + 8] == b"vidsMJPG"
    scale, rate, start, length = struct.unpack_from("<4I", data, off + 20)
    assert rate / scale == 25 and start == 0 and length == 3
    assert struct.unpack_from("<4H", data, off + 48) == (0, 0, w, h)
    _, off, size, _ = jpeg_ref.riff_find(tree, b"strf")
    assert size == 40
    assert struct.unpack_from("<IiiHH4sI", data, off) == (40, w, h, 1, 24, b"MJPG", 3 * w * h)
    movi = jpeg_ref.riff_find(tree, b"LIST:movi")
    chunks = movi[3]
    assert [c[0] for c in chunks] == [b"00dc"] * 3 and [c[2] for c in chunks] == [len(f) for f in files]
    _, off, size, _ = jpeg_ref.riff_find(tree, b"idx1")
    assert size == 48
    for k in range(3):
        ckid, flags, rel, length = struct.unpack_from("<4sIII", data, off + 16 * k)
        at = movi[1] + rel  # movi[1] is the offset of the list's data: the 'movi' fourcc
        assert ckid == b"00dc" and flags & 0x10 and length == len(files[k])
        assert data[at:at + 4] == b"00dc" and struct.unpack_from("<I", data, at + 4)[0] == length
        assert data[at + 8:at + 8 + length] == files[k] and at % 2 == 0
        if length % 2:
            assert data[at + 8 + length] == 0  # the pad byte
        got = np.asarray(Image.open(_io.BytesIO(data[at + 8:at + 8 + length])).convert("RGB"))
        assert got.shape == (h, w, 3) and psnr(got, pics[k]) > 25


def test_avi_without_frames_and_closed_writer(tmp_path):
    path = str(tmp_path / "empty.avi")
    wr = MjpegWriter(path)
    wr.close()
    wr.close()
    data = open(path, "rb").read()
    tree = jpeg_ref.riff_walk(data)
    assert tree[0][2] == len(data) - 8
    assert struct.unpack_from("<14I", data, jpeg_ref.riff_find(tree, b"avih")[1])[4] == 0
    with pytest.raises(ValueError, match="closed"):
        wr.write_jpeg(jpeg_ref.encode(jpeg_ref.anchor_picture(8, 8)))
    with pytest.raises(ValueError, match="fps"):
        MjpegWriter(str(tmp_path / "x.avi"), fps=0)


def test_writer_refuses_cpu_tensors_and_files_past_2_gib(tmp_path, monkeypatch):
    import torch
    from esmstereo_amd import video

    with MjpegWriter(str(tmp_path / "a.avi")) as wr:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            wr.write(torch.zeros(8, 8, 3, dtype=torch.uint8))
        with pytest.raises(ValueError, match="uint8"):
            wr.write(torch.zeros(8, 8, 3))
        monkeypatch.setattr(video, "MAX_FILE", 1500)
        f = jpeg_ref.encode(jpeg_ref.anchor_picture(8, 8))
        wr.write_jpeg(f)
        with pytest.raises(ValueError, match="2 GiB"):
            wr.write_jpeg(f)
    assert len(jpeg_ref.riff_find(jpeg_ref.riff_walk(open(str(tmp_path / "a.avi"), "rb").read()), b"LIST:movi")[3]) == 1


def test_package_exports():
    import esmstereo_amd as pkg
    from esmstereo_amd import render

    assert pkg.MjpegWriter is MjpegWriter and pkg.JpegEncoder is render.JpegEncoder
    assert pkg.jpeg_encode_bgr8 is render.jpeg_encode_bgr8
    assert render.jpeg_header(50, 37, 75, "420", 8) == jpeg_ref.header(50, 37, 75, 420, 8)
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.jpeg_encode_bgr8(torch.zeros(8, 8, 3, dtype=torch.uint8))
