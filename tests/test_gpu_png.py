"""The device PNG encoder (csrc/png.hip) against tests/png_ref.py, zlib and PIL.

For every image: ``zlib.decompress(stream)`` is the reference's filtered scanlines (that alone checks the header, every
code, every chunk offset, the padding and the device Adler-32); the PNG opens with PIL and with png_ref's own parser
and equals the input exactly; the stream is bitwise png_ref's bit-at-a-time encoder run with the library's code lengths,
never longer than esm_png_stream_bound, and bitwise the same on a second call.  Shapes are the smallest that can go
wrong: raw sizes one below, at and one above the chunk, three chunks and a tail, rows whose length is no multiple of 4.

LDS, in tests/lds_poison.py's terms: png.hip is the first kernel in the tree to keep OFFSETS in LDS (the workgroup
scans' wave sums become each lane's bit offset, i.e. an index into the LDS staging buffer and, through the chunk's
start, a dword index into the output slot), so a leftover word there would not be a wrong value but a wild address.
The kernels write every such word before they read it and zero their own staging buffer, and every store into the
output and into the staging buffer is compared with its extent first; ``test_lds_leftovers`` runs a multi-chunk B = 2
encode behind both poison patterns and asserts the same bytes.
"""
import io as _io
import ctypes
import zlib

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

import lds_poison  # noqa: E402
import png_ref  # noqa: E402
from esmstereo_amd import _lib, io as EIO, render  # noqa: E402

lib = _lib.lib
DEV = torch.device("cuda")
C = lib.esm_png_chunk_bytes()
FILTERS = ("none", "sub", "up")


def shape_for(raw: int, bpp: int):
    """(h, w) with h * (1 + bpp * w) == raw and a row length 1 + bpp * w that is no multiple of 4: the shortest such
    row of at least 10 bytes (many rows, so that Up has a row above and chunk ends fall anywhere in a row)."""
    for row in range(10, raw + 1):
        if raw % row == 0 and (row - 1) % bpp == 0 and row % 4:
            return raw // row, (row - 1) // bpp
    raise AssertionError(f"no {bpp}-byte-per-pixel image has {raw} raw bytes")


def library_lengths(filtered: bytes):
    hist = np.concatenate([np.bincount(np.frombuffer(filtered, dtype=np.uint8), minlength=256), [1]])
    out = (ctypes.c_uint8 * 257)()
    assert lib.esm_deflate_code_lengths((ctypes.c_uint32 * 257)(*[int(v) for v in hist]), out) == 0
    return list(out)


def check_png(png: bytes, image: np.ndarray, filtered: bytes):
    """``image``: uint16 [h, w], or uint8 [h, w, 3] in R, G, B order."""
    Image = pytest.importorskip("PIL.Image")
    (w, h, depth, ctype, *_), stream = png_ref.split(png)
    assert (h, w) == image.shape[:2] and (depth, ctype) == ((16, 0) if image.ndim == 2 else (8, 2))
    assert stream[:2] == b"\x78\x01"
    assert zlib.decompress(stream) == filtered
    assert len(stream) <= lib.esm_png_stream_bound(len(filtered))
    expect = png_ref.encode(filtered, library_lengths(filtered))
    assert len(stream) == len(expect) and stream == expect
    assert np.array_equal(np.asarray(Image.open(_io.BytesIO(png))).astype(image.dtype), image)
    assert np.array_equal(png_ref.parse(png), image)
    return len(stream)


def check_u16(a: np.ndarray, filt: str):
    """a: uint16 [B, h, w]."""
    t = torch.from_numpy(a.view(np.int16)).to(DEV)
    pngs = EIO.png_encode_u16(t, filter=filt)
    assert len(pngs) == a.shape[0]
    for b, png in enumerate(pngs):
        check_png(png, a[b], png_ref.filtered_u16(a[b], png_ref.FILTERS[filt]))
    assert EIO.png_encode_u16(t, filter=filt) == pngs, "the bytes differ between two calls"
    return pngs


def check_rgb8(a: np.ndarray, order: str, filt: str):
    """a: uint8 [B, h, w, 3] with channels in ``order``."""
    t = torch.from_numpy(a).to(DEV)
    pngs = render.png_encode_bgr8(t, order=order, filter=filt)
    assert len(pngs) == a.shape[0]
    for b, png in enumerate(pngs):
        rgb = a[b, :, :, ::-1] if order == "bgr" else a[b]
        check_png(png, rgb, png_ref.filtered_rgb8(a[b], order, png_ref.FILTERS[filt]))
    assert render.png_encode_bgr8(t, order=order, filter=filt) == pngs, "the bytes differ between two calls"


def ramp_u16(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.round((20 + 0.11 * x + 0.07 * y + 2 * np.sin(x / 9.0)) * 256).astype(np.uint16)


def noise_u16(h, w, seed):
    return np.random.default_rng(seed).integers(0, 65536, (h, w), dtype=np.uint16)


RAW_SIZES = {"C-1": C - 1, "C": C, "C+1": C + 1, "3C+5": 3 * C + 5}


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("size", sorted(RAW_SIZES))
def test_u16_sizes_around_the_chunk(size, filt):
    h, w = shape_for(RAW_SIZES[size], 2)
    check_u16(np.stack([ramp_u16(h, w), noise_u16(h, w, 7)]), filt)  # B = 2: own table, offsets and slot each


@pytest.mark.parametrize("order", ("bgr", "rgb"))
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("size", sorted(RAW_SIZES))
def test_rgb8_sizes_around_the_chunk(size, filt, order):
    h, w = shape_for(RAW_SIZES[size], 3)
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.stack([(3 * x + y) % 256, (x + 2 * y) % 256, (x * y) % 256], axis=-1).astype(np.uint8)
    check_rgb8(np.stack([smooth, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)]), order, filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_one_pixel(filt):
    check_u16(np.array([[[0xA1B2]]], dtype=np.uint16), filt)
    check_rgb8(np.array([[[[1, 2, 3]]]], dtype=np.uint8), "bgr", filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_one_row_longer_than_a_chunk(filt):
    check_u16(np.stack([ramp_u16(1, C), noise_u16(1, C, 3)]), filt)  # raw = 1 + 2 C: the row crosses two chunk ends


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("content", ("zero", "all_bytes", "noise", "fibonacci", "ramp"))
def test_u16_contents(content, filt):
    h, w = shape_for(3 * C + 5, 2)
    if content == "zero":  # a two-symbol code: the filter byte (or the zero) and end-of-block
        a = np.zeros((2, h, w), dtype=np.uint16)
    elif content == "all_bytes":  # every byte value occurs, in both the high and the low byte
        v = (np.arange(h * w) % 256).astype(np.uint16)
        a = np.stack([(v << 8 | v[::-1]).reshape(h, w), (v * 257).reshape(h, w)])
    elif content == "noise":  # ~8 bits a byte: the stream is as long as it gets; check_png holds it to the bound
        a = np.stack([noise_u16(h, w, 1), noise_u16(h, w, 2)])
    elif content == "fibonacci":  # length limiting is active on the device (filter none; the others just differ)
        a = np.stack([png_ref.fibonacci_map(0), png_ref.fibonacci_map(1)])
        if filt == "none":
            assert max(library_lengths(png_ref.filtered_u16(a[0], 0))) == 15
    else:
        a = np.stack([ramp_u16(h, w), ramp_u16(h, w)[::-1, ::-1]])
    check_u16(np.ascontiguousarray(a), filt)


def check_prefilled_buffers_and_neighbouring_slot(h, w):
    """Slots, workspace and lengths hold 0xFF before the call: the encoder zeroes what it ORs into, writes nothing
    behind its stream but the rest of the last dword, and nothing into a slot it was not given."""
    a = np.stack([ramp_u16(h, w), noise_u16(h, w, 5)])
    enc = EIO.PngEncoder(2, h, 2 * w)
    t = torch.from_numpy(a.view(np.int16)).to(DEV)
    for n in (1, 2):
        enc.out.fill_(0xFF)
        enc.work.fill_(0xFF)
        enc.lengths.fill_(-1)
        pngs = enc.encode_u16(t[:n], filter="sub")
        out = enc.out.cpu().numpy()
        for b in range(n):
            size = check_png(pngs[b], a[b], png_ref.filtered_u16(a[b], 1))
            assert int(enc.host_lengths[b]) == size
            assert (out[b, size + 4:] == 0xFF).all(), "bytes behind the stream were written"
        for b in range(n, 2):
            assert (out[b] == 0xFF).all(), "a slot of an image that was not encoded was written"
            assert int(enc.lengths[b]) == -1


def test_prefilled_buffers_and_neighbouring_slot():
    check_prefilled_buffers_and_neighbouring_slot(*shape_for(3 * C + 5, 2))


def test_disparity_entry_matches_the_u16_path():
    """png_encode_disparity == png_encode_u16(disparity_to_u16(...)), byte for byte: exact .5/256 ties (round half to
    even) inside the window, NaN everywhere outside it."""
    Hp, Wp, top, left, h, w = 80, 70, 9, 6, 67, 59  # raw = 67 * 119 = 7973: three chunks
    g = torch.Generator().manual_seed(5)
    d = torch.full((2, Hp, Wp), float("nan"))
    d[:, top:top + h, left:left + w] = torch.rand(2, h, w, generator=g) * 200
    ties = torch.tensor([0.0, 1 / 512, 3 / 512, 5 / 512, 100.25, 7 / 512, 255.998, 2.5 / 256, 0.5 / 256, 1.5 / 256])
    d[0, top + 10, left:left + 10] = ties
    d[1, top + h - 1, left + w - 10:left + w] = ties + 17
    dev = d.to(DEV)
    u16 = EIO.disparity_to_u16(dev, top, left, h, w)
    for filt in FILTERS:
        got = EIO.png_encode_disparity(dev, top, left, h, w, filter=filt)
        assert got == EIO.png_encode_u16(u16, filter=filt)
        ref = u16.cpu().numpy().view(np.uint16)
        for b in range(2):
            check_png(got[b], ref[b], png_ref.filtered_u16(ref[b], png_ref.FILTERS[filt]))
    with pytest.raises(_lib.EsmError, match="window"):
        EIO.PngEncoder(2, h, 2 * w).encode_disparity(dev, top + 20, left, h, w)


def test_write_png_u16_device(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    a = np.stack([ramp_u16(30, 41), noise_u16(30, 41, 9)])
    paths = [str(tmp_path / f"{b}.png") for b in range(2)]
    EIO.write_png_u16_device(paths, torch.from_numpy(a.view(np.int16)).to(DEV))
    for b in range(2):
        assert np.array_equal(np.asarray(Image.open(paths[b])).astype(np.uint16), a[b])
    with pytest.raises(ValueError, match="paths"):
        EIO.write_png_u16_device(paths[:1], torch.from_numpy(a.view(np.int16)).to(DEV))


def check_lds_leftovers(h, w):
    """A full B = 2 encode behind poisoned LDS (see the module docstring): same lengths, same bytes."""
    a = np.stack([ramp_u16(h, w), noise_u16(h, w, 5)])
    t = torch.from_numpy(a.view(np.int16)).to(DEV)
    enc = EIO.PngEncoder(2, h, 2 * w)
    enc.out.fill_(0xFF)
    enc.lengths.fill_(-1)

    def launch():
        _lib.check(lib.esm_png_encode_u16(t.data_ptr(), 2, h, w, *enc._args("sub")), "png_encode_u16")

    def outputs():  # (after the synchronisation) the lengths and each stream up to its length; then spoil both again,
        n = enc.lengths.clone()  # so that a launch that stored nothing cannot leave "the same bytes"
        keep = torch.arange(enc.slot, device=DEV)[None, :] < n[:, None]
        streams = torch.where(keep, enc.out, torch.zeros_like(enc.out))
        enc.out.fill_(0xFF)
        enc.lengths.fill_(-1)
        return [n, streams]

    lds_poison.assert_leftover_free(launch, outputs, "png_encode_u16")
    launch()
    pngs = [EIO.png_wrap(s, w, h, 16, 0) for s in enc._streams(2)]
    for b in range(2):
        check_png(pngs[b], a[b], png_ref.filtered_u16(a[b], 1))


def test_lds_leftovers():
    check_lds_leftovers(*shape_for(3 * C + 5, 2))  # four chunks


def test_cpu_tensor_raises():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EIO.png_encode_u16(torch.zeros(1, 4, 5, dtype=torch.int16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EIO.png_encode_disparity(torch.zeros(1, 8, 8), 0, 0, 4, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.png_encode_bgr8(torch.zeros(4, 5, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EIO.PngEncoder(1, 4, 10, device="cuda").encode_u16(torch.zeros(1, 4, 5, dtype=torch.int16))
