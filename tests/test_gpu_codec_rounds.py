"""The device codecs past the first round of every loop that depends on the size of the picture.

tests/test_gpu_jpeg.py and tests/test_gpu_png.py take the smallest shapes that can go wrong in a block or a chunk; this
module takes the comparisons they make (bytes and lengths equal to jpeg_ref / png_ref, ``zlib.decompress`` equal to the
filtered scanlines, the same bytes on a second call) to the sizes at which the per-image loops go round again:

* jpeg_scan_kernel scans an image's interval lengths 256 at a time with a 64-bit carry between the rounds.  Cases at
  exactly 256 intervals (one full round), 257, 289, 525 (the carry added twice), 789 (four rounds, 4:2:0, a width with
  w % 16 == 8) and one 750 x 1242 node frame at the default restart interval (459).
* png_table_kernel has three loops over an image's chunks: a wave per chunk for the bit counts (four waves), the
  256-wide scan with its carry, and the Adler-32 fold in which each lane takes every 256th chunk and reduces
  modulo 65521.  Cases at 15, 18 and 19 chunks (the wave loop; raw sizes around 65,521 + one chunk, where the
  distance from a chunk's end to the end of the data is first reduced), 256, 257, 258 and 513 chunks, and a white
  16-bit map whose chunks of 0xFF bytes carry the largest sums a chunk can have.

Every case asserts the count it was chosen for (and the 256 threads both scans are as wide as), so that another chunk
size or block size cannot move it back into the first round without this module saying so.
"""
import io as _io
import os
import re

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

import png_ref  # noqa: E402
import test_gpu_jpeg as TJ  # noqa: E402
import test_gpu_png as TP  # noqa: E402
from esmstereo_amd import _lib, render  # noqa: E402

lib = _lib.lib
DEV = torch.device("cuda")
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
ROUND = 256  # intervals / chunks per round of either scan: the kernels' block size


def block_size(source: str) -> int:
    with open(os.path.join(CSRC, source)) as f:
        return int(re.search(r"^constexpr int kThreads = (\d+);", f.read(), re.M).group(1))


def rounds(count: int) -> int:
    return -(-count // ROUND)


# ---------------------------------------------------------------------------------------------------------------- JPEG

def intervals(h, w, sub, ri) -> int:
    """The restart intervals of one image, as the library sizes its workspace (12 bytes each) and as the header's
    definition counts them."""
    mcu = 16 if sub == 420 else 8
    n = -(-(-(-h // mcu) * -(-w // mcu)) // ri)
    assert lib.esm_jpeg_workspace_bytes(1, h, w, sub, ri) == 12 * n
    return n


BOTH = ("bgr", "rgb")
#              h, w, subsampling, Ri, intervals, rounds, channel orders
JPEG_CASES = ((128, 128, 444, 1, 256, 1, BOTH),      # exactly one full round: the loop ends at c0 == nint
              (8, 2056, 444, 1, 257, 2, BOTH),       # a second round of one lane
              (136, 136, 444, 1, 289, 2, BOTH),      # a partial second round
              (24, 1400, 444, 1, 525, 3, BOTH),      # the carry is added twice
              (40, 4200, 420, 1, 789, 4, ("bgr",)),  # 263 MCU columns, the last one half replicated (w % 16 == 8)
              (136, 136, 420, 3, 27, 1, BOTH))       # the contrast: the 289-interval picture in one round


def test_scans_are_256_wide():
    assert block_size("jpeg.hip") == ROUND and block_size("png.hip") == ROUND


@pytest.mark.parametrize("h,w,sub,ri,nint,nrounds,orders", JPEG_CASES,
                         ids=[f"{c[0]}x{c[1]}-{c[2]}-Ri{c[3]}-{c[4]}intervals" for c in JPEG_CASES])
def test_jpeg_interval_rounds(h, w, sub, ri, nint, nrounds, orders):
    assert intervals(h, w, sub, ri) == nint and rounds(nint) == nrounds
    for order in orders:
        TJ.check(("ramp", "noise"), h, w, sub=sub, ri=ri, order=order)


def pil_loads(data: bytes, h: int, w: int):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(_io.BytesIO(data))
    im.load()  # decodes the whole scan: every restart marker is where a decoder expects it
    assert im.size == (w, h)


def test_jpeg_one_node_frame():
    """750 x 1242 (StereoNode's two-panel frame at KITTI size), 4:2:0, Ri 8, quality 75: 459 intervals."""
    h, w = 750, 1242
    assert intervals(h, w, 420, 8) == 459 and rounds(459) == 2
    pil_loads(TJ.check(("noise",), h, w)[0], h, w)


def test_jpeg_marker_sequence_at_289_intervals():
    """Read back from the device's own bytes: RST0 .. RST7 thirty-six times, then EOI."""
    assert intervals(136, 136, 444, 1) == 289
    data = TJ.check(("noise",), 136, 136, sub=444, ri=1)[0][629:]
    marks = [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and data[i + 1] not in (0x00, 0xFF)]
    assert marks == [0xD0 + (k & 7) for k in range(288)] + [0xD9]


def test_jpeg_pil_loads_the_289_interval_files():
    for sub, ri in ((444, 1), (420, 3)):
        for data in TJ.check(("ramp", "noise"), 136, 136, sub=sub, ri=ri):
            pil_loads(data, 136, 136)


def test_jpeg_overflow_at_289_intervals():
    """A slot that ends inside the second round's intervals: the need is reported, the prefix is in place (offsets
    with the carry included), the neighbouring slot is untouched, and the encoder's retry gives the file."""
    h, w, sub, ri, slot = 136, 136, 444, 1, 22000
    assert intervals(h, w, sub, ri) == 289
    ref = TJ.scan_bytes("noise", h, w, 75, sub, ri)
    assert slot < len(ref)
    a = torch.from_numpy(TJ.picture("noise", h, w).copy()).to(DEV)
    out = torch.full((2, slot), 0xA5, dtype=torch.uint8, device=DEV)  # slot 1: the poisoned neighbour
    lengths = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    work = torch.empty(lib.esm_jpeg_workspace_bytes(1, h, w, sub, ri), dtype=torch.uint8, device=DEV)
    _lib.check(lib.esm_jpeg_encode_rgb8(a.data_ptr(), 1, h, w, 1, 75, sub, ri, work.data_ptr(), out.data_ptr(), slot,
                                        lengths.data_ptr(), None), "jpeg_encode_rgb8")
    torch.cuda.synchronize()
    assert lengths.tolist() == [-len(ref), -7]
    got = out.cpu().numpy()
    assert (got[1] == 0xA5).all(), "the neighbouring slot was written"
    assert got[0].tobytes() == ref[:slot]
    # the slot ends behind interval 256's start: the prefix holds bytes placed with the carry
    marks = [i for i in range(slot - 1) if ref[i] == 0xFF and 0xD0 <= ref[i + 1] <= 0xD7]
    assert len(marks) > ROUND
    enc = render.JpegEncoder(1, h, w, 75, str(sub), ri, slot_bytes=slot)
    assert enc.encode(a, "bgr") == [TJ.reference("noise", h, w, 75, sub, ri, "bgr")]
    assert enc.slot == lib.esm_jpeg_stream_bound(h, w, sub, ri) >= len(ref)


def test_jpeg_lds_leftovers_at_289_intervals():
    assert intervals(136, 136, 444, 1) == 289
    TJ.check_lds_leftovers(136, 136, 444, 1)


# ----------------------------------------------------------------------------------------------------------------- PNG

C = TP.C


def chunks(raw: int) -> int:
    return -(-raw // C)


def smooth_rgb8(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(3 * x + y) % 256, (x + 2 * y) % 256, (x * y) % 256], axis=-1).astype(np.uint8)


#             kind, h, w, raw bytes, chunks, rounds of the scan
PNG_CASES = (("u16", 27, 1000, 54027, 15, 1),      # the wave loop's 2nd to 4th iteration; Adler-32 without reduction
             ("u16", 17, 1927, 65535, 18, 1),      # the largest raw size of 16 bits: raw - end stays below 65521
             ("u16", 19, 1825, 69369, 19, 1),      # chunk 0's raw - end = 65,529: the first size at which it reduces
             ("rgb8", 240, 1365, 983040, 256, 1),  # exactly one full round
             ("u16", 3, 164000, 984003, 257, 2),   # a second round of one lane; rows far longer than a chunk
             ("u16", 257, 1921, 987651, 258, 2),   # a partial second round
             ("rgb8", 400, 1640, 1968400, 513, 3))  # three rounds; each Adler lane folds up to three chunks


def png_case(kind, h, w, raw, nchunks, nrounds):
    assert h * (1 + (2 if kind == "u16" else 3) * w) == raw and chunks(raw) == nchunks and rounds(nchunks) == nrounds
    if kind == "u16":
        return np.stack([TP.ramp_u16(h, w), TP.noise_u16(h, w, 7)])
    return np.stack([smooth_rgb8(h, w), np.random.default_rng(11).integers(0, 256, (h, w, 3), dtype=np.uint8)])


@pytest.mark.parametrize("filt", TP.FILTERS)
@pytest.mark.parametrize("kind,h,w,raw,nchunks,nrounds", PNG_CASES, ids=[f"{c[0]}-{c[4]}chunks" for c in PNG_CASES])
def test_png_chunk_rounds(kind, h, w, raw, nchunks, nrounds, filt):
    a = png_case(kind, h, w, raw, nchunks, nrounds)
    if kind == "u16":
        TP.check_u16(a, filt)
    else:
        TP.check_rgb8(a, "bgr" if nchunks == 256 else "rgb", filt)


@pytest.mark.parametrize("filt,depth", [("sub", 17), ("up", 16)])
def test_png_length_limit_is_active_at_258_chunks(filt, depth):
    """The 16-bit ramp at 257 x 1921 behind Sub / Up: a few residuals a million times, the others a handful of times,
    so its unrestricted Huffman tree is 17 / 16 deep (built here on the host) and the lengths the device computes in
    test_png_chunk_rounds are limited ones, at a real size."""
    filtered = png_ref.filtered_u16(TP.ramp_u16(257, 1921), png_ref.FILTERS[filt])
    counts = np.concatenate([np.bincount(np.frombuffer(filtered, dtype=np.uint8), minlength=256), [1]])
    assert huffman_depth(counts) == depth
    assert max(TP.library_lengths(filtered)) == 15


def huffman_depth(counts) -> int:
    """The depth of an unrestricted Huffman tree over the non-zero counts."""
    import heapq
    heap = [(int(c), 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (ca, da), (cb, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (ca + cb, max(da, db) + 1))
    return heap[0][1]


def test_png_white_map_has_the_largest_chunk_sums():
    """2 x 11520 of 0xFFFF, filter none: chunks 1 to 5 are 3840 bytes of 0xFF each, the largest sums a chunk can have
    (sum d = 979,200, above 65521, so ``a % 65521`` reduces; sum (n - i) d = 1,880,553,600 of 2^32)."""
    h, w = 2, 11520
    white = np.full((h, w), 0xFFFF, dtype=np.uint16)
    d = np.frombuffer(png_ref.filtered_u16(white, 0), dtype=np.uint8).astype(np.int64)
    assert d.size == 46082 and chunks(d.size) == 13
    full = d[:d.size // C * C].reshape(-1, C)
    assert (full[1:6] == 0xFF).all()
    assert int(full.sum(axis=1).max()) == 979200 == C * 255
    assert int((full * (C - np.arange(C))).sum(axis=1).max()) == 1880553600 < 2 ** 32
    TP.check_u16(np.stack([white, TP.noise_u16(h, w, 3)]), "none")
    TP.check_u16(white[None], "none")


def test_png_prefilled_buffers_and_neighbouring_slot_at_258_chunks():
    assert chunks(257 * (1 + 2 * 1921)) == 258
    TP.check_prefilled_buffers_and_neighbouring_slot(257, 1921)


def test_png_lds_leftovers_at_258_chunks():
    assert chunks(257 * (1 + 2 * 1921)) == 258
    TP.check_lds_leftovers(257, 1921)
