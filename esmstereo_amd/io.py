"""The steps on either side of the hot path, on device-resident data.

Input side — the reference turns an 8-bit RGB image into the network input two ways:

* ``kitti_test_transform`` — test_kitti.py:93-106 (and test_mid / save_vid / latest): PIL
  ``crop((w - wi, h - hi, w, h))`` pads the uint8 image with zeros at the TOP-LEFT to
  ``wi, hi = (w // 32 + 1) * 32, (h // 32 + 1) * 32``, then ``ToTensor`` + ``Normalize`` — so the
  padding holds ``(0 - mean) / std``; the prediction is cropped back with
  ``pred[:, hi - h:, wi - w:]`` (test_kitti.py:115).
* ``kitti_dataset_transform`` — datasets/kitti_dataset.py:151-170 (the loader of save_disp.py):
  ``ToTensor`` + ``Normalize`` first, then ``np.pad`` with 0.0 at the TOP and RIGHT to 384 x 1248;
  the prediction is cropped back with ``disp[top_pad:, :-right_pad]`` (save_disp.py:81).

Output side — ``disparity_to_u16``: ``np.round(disp * 256).astype(np.uint16)`` of the cropped map
(save_disp.py:85), and ``write_png_u16`` writes it as the 16-bit grayscale PNG that
``skimage.io.imsave`` produces there (save_disp.py:86; skimage is not a dependency here).

Both transforms and the rounding are one HIP launch each (``csrc/io.hip``), bit-exact with the
torchvision / numpy arithmetic; there is no CPU fallback.

The reference's resizing ROS nodes (``virtual_kitti_publisher``, ``kitti_publisher_ess``) do not pad: they
``cv::resize`` every frame to the engine's one size.  ``resize_u8`` and ``resize_preprocess`` are that step
(``csrc/resize.hip``): the 8-bit INTER_LINEAR rule restated in include/esmstereo_amd.h, bit-exact against its numpy
restatement (tests/resize_ref.py); parity with OpenCV's own bytes is UNPINNED.

``png_encode_u16`` / ``png_encode_disparity`` / ``write_png_u16_device`` (and ``render.png_encode_bgr8``) write the
same PNGs without the raw map leaving the device: ``csrc/png.hip`` builds the zlib stream (PNG filter, one
Huffman-only deflate block, Adler-32) in three launches, and the host adds the chunk framing and the CRC-32.
``png_u16_bytes`` / ``write_png_u16`` stay as the host encoders (zlib level 6) for CPU arrays and as the baseline.
"""
from __future__ import annotations

import ctypes
import os
import struct
import zlib
from typing import Sequence, Tuple

import numpy as np
import torch

from ._lib import check, lib, _stream

IMAGENET_MEAN = (0.485, 0.456, 0.406)  # datasets/data_io.py:8
IMAGENET_STD = (0.229, 0.224, 0.225)   # datasets/data_io.py:9


def _as_batch_u8(img: torch.Tensor) -> torch.Tensor:
    if img.dtype != torch.uint8:
        raise TypeError(f"expected a uint8 RGB image, got {img.dtype}")
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[-1] != 3:
        raise ValueError(f"expected [H, W, 3] or [B, H, W, 3] uint8, got {tuple(img.shape)}")
    if not img.is_cuda:
        raise RuntimeError("esmstereo_amd.io: the image must be on the GPU (no CPU fallback)")
    return img.contiguous()


def _pad_normalize(img: torch.Tensor, Hp: int, Wp: int, top: int, left: int, pad_normalized: bool) -> torch.Tensor:
    B, H, W, _ = img.shape
    out = torch.empty(B, 3, Hp, Wp, device=img.device, dtype=torch.float32)
    check(lib.esm_preprocess_u8(img.data_ptr(), out.data_ptr(), B, H, W, Hp, Wp, top, left, int(pad_normalized),
                                _stream(img)), "preprocess")
    return out


def kitti_test_size(h: int, w: int, m: int = 32) -> Tuple[int, int]:
    """Padded extent of test_kitti.py:94-95: ``(x // m + 1) * m`` (always at least one pixel of pad)."""
    return (h // m + 1) * m, (w // m + 1) * m


def kitti_test_transform(img: torch.Tensor) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """uint8 RGB ``[H, W, 3]`` / ``[B, H, W, 3]`` on the GPU -> (input ``[B, 3, hi, wi]``, (top, left)).

    test_kitti.py:93-106; crop the prediction back with ``pred[:, top:, left:]``."""
    img = _as_batch_u8(img)
    h, w = int(img.shape[1]), int(img.shape[2])
    hi, wi = kitti_test_size(h, w)
    return _pad_normalize(img, hi, wi, hi - h, wi - w, True), (hi - h, wi - w)


def kitti_dataset_transform(img: torch.Tensor, size: Tuple[int, int] = (384, 1248)) -> Tuple[torch.Tensor, int, int]:
    """uint8 RGB on the GPU -> (input ``[B, 3, 384, 1248]``, top_pad, right_pad), as
    datasets/kitti_dataset.py:151-170 (which asserts both pads are positive)."""
    img = _as_batch_u8(img)
    h, w = int(img.shape[1]), int(img.shape[2])
    top_pad, right_pad = size[0] - h, size[1] - w
    if not (top_pad > 0 and right_pad > 0):
        raise AssertionError(f"kitti_dataset: image {h}x{w} does not fit {size[0]}x{size[1]} with a pad")
    return _pad_normalize(img, size[0], size[1], top_pad, 0, False), top_pad, right_pad


def _size(size) -> Tuple[int, int]:
    h, w = (int(v) for v in size)
    return h, w


def _constants(mean: Sequence[float], std: Sequence[float]):
    """``mean`` / ``std`` as the two host arrays of 3 floats ``esm_preprocess_resize_u8`` takes."""
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("resize_preprocess: mean and std take three values each")
    return (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])


def resize_u8(img: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """``cv2.resize(img, (width, height), interpolation=cv2.INTER_LINEAR)`` of an 8-bit image on the GPU, by the
    fixed-point rule include/esmstereo_amd.h states for ``esm_resize_u8`` (parity with OpenCV's own bytes is
    UNPINNED).  ``img``: uint8 ``[H, W]``, ``[H, W, 3]``, ``[B, H, W, 3]`` or ``[B, H, W]`` (a 3-D tensor whose last
    extent is 3 is one colour image); ``size = (height, width)``.  Returns the same rank at ``size``.  A
    non-contiguous input is made contiguous first."""
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() not in (2, 3, 4) or (
            img.dim() == 4 and img.shape[-1] != 3):
        raise ValueError("resize_u8: expected a uint8 [H, W], [H, W, 3], [B, H, W, 3] or [B, H, W] tensor")
    if not img.is_cuda:
        raise RuntimeError("esmstereo_amd.io: resize_u8: the image must be on the GPU (no CPU fallback)")
    H, W = _size(size)
    C = 3 if img.dim() == 4 or (img.dim() == 3 and img.shape[-1] == 3) else 1
    src = img.contiguous()
    batched = src.dim() == (4 if C == 3 else 3)
    B = int(src.shape[0]) if batched else 1
    Hs, Ws = (int(v) for v in (src.shape[1:3] if batched else src.shape[:2]))
    out = torch.empty(((B,) if batched else ()) + (H, W) + ((3,) if C == 3 else ()), device=src.device,
                      dtype=torch.uint8)
    with torch.cuda.device(src.device):
        check(lib.esm_resize_u8(src.data_ptr(), out.data_ptr(), B, Hs, Ws, H, W, C, _stream(src)), "resize_u8")
    return out


def resize_preprocess(img: torch.Tensor, size: Tuple[int, int], mean: Sequence[float] = IMAGENET_MEAN,
                      std: Sequence[float] = IMAGENET_STD, return_resized: bool = False):
    """``preprocess_image`` of the reference's resizing nodes (virtual_kitti_publisher_cuda_node.cpp:232-266,
    kitti_publisher_ess_cuda_node.cpp:241-275, the latter with ``mean = (0, 0, 0)``, ``std = (1, 1, 1)``) in one
    launch: uint8 ``[H, W, 3]`` / ``[B, H, W, 3]`` on the GPU -> the network input ``[B, 3, height, width]`` fp32,
    ``(resized / 255 - mean[c]) / std[c]`` of :func:`resize_u8`'s bytes, channel ``c`` as stored.  With
    ``return_resized`` the resized bytes ``[B, height, width, 3]`` come back too, from the same launch."""
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise ValueError("resize_preprocess: expected a uint8 [H, W, 3] or [B, H, W, 3] tensor")
    src = _as_batch_u8(img)
    H, W = _size(size)
    m, s = _constants(mean, std)
    B, Hs, Ws, _ = (int(v) for v in src.shape)
    out = torch.empty(B, 3, H, W, device=src.device, dtype=torch.float32)
    resized = torch.empty(B, H, W, 3, device=src.device, dtype=torch.uint8) if return_resized else None
    with torch.cuda.device(src.device):
        check(lib.esm_preprocess_resize_u8(src.data_ptr(), out.data_ptr(),
                                           resized.data_ptr() if return_resized else None, B, Hs, Ws, H, W, m, s,
                                           _stream(src)), "resize_preprocess")
    return (out, resized) if return_resized else out


def disparity_to_u16(disp: torch.Tensor, top: int, left: int, h: int, w: int) -> torch.Tensor:
    """``np.round(disp[:, top:top+h, left:left+w] * 256).astype(np.uint16)`` on the GPU
    (save_disp.py:81,85; test_kitti.py:115 crop) -> uint16 ``[B, h, w]``."""
    if disp.dim() == 4 and disp.shape[1] == 1:
        disp = disp[:, 0]
    if disp.dim() == 2:
        disp = disp.unsqueeze(0)
    if disp.dim() != 3 or disp.dtype != torch.float32 or not disp.is_cuda:
        raise ValueError("disparity_to_u16: expected a float32 [B, H, W] GPU tensor")
    disp = disp.contiguous()
    B, Hp, Wp = (int(v) for v in disp.shape)
    out = torch.empty(B, h, w, device=disp.device, dtype=torch.int16)
    check(lib.esm_disp_to_u16(disp.data_ptr(), out.data_ptr(), B, Hp, Wp, top, left, h, w, _stream(disp)),
          "disp_to_u16")
    return out.view(torch.uint16)


def png_u16_bytes(a: np.ndarray) -> bytes:
    """A 16-bit grayscale PNG (big-endian samples, zlib-deflated, filter 0 per row) of ``a``."""
    a = np.ascontiguousarray(a, dtype=np.uint16)
    if a.ndim != 2:
        raise ValueError("png_u16_bytes: expected a 2-D array")
    h, w = a.shape
    raw = np.empty((h, 1 + 2 * w), dtype=np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = a.astype(">u2").view(np.uint8).reshape(h, 2 * w)
    return png_wrap(zlib.compress(raw.tobytes(), 6), w, h, 16, 0)


def write_png_u16(path: str, a) -> None:
    """``skimage.io.imsave(fn, disp_est_uint)`` of save_disp.py:86 for a uint16 map."""
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    with open(path, "wb") as f:
        f.write(png_u16_bytes(a))


# ---- the same files, encoded on the device (csrc/png.hip): PNG filter + Huffman-only deflate, no LZ77 ----
PNG_FILTERS = {"none": 0, "sub": 1, "up": 2}


def _png_filter(filter) -> int:
    if filter not in PNG_FILTERS:
        raise ValueError(f"png: filter must be one of {sorted(PNG_FILTERS)}, got {filter!r}")
    return PNG_FILTERS[filter]


def png_wrap(stream: bytes, width: int, height: int, bit_depth: int, color_type: int) -> bytes:
    """The PNG file around one zlib ``stream``: signature, IHDR, one IDAT with its CRC-32 (host ``zlib.crc32``), IEND."""
    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(tag)))

    ihdr = struct.pack(">IIBBBBB", width, height, bit_depth, color_type, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")


class _DeviceEncoder:
    """What the two device encoders (:class:`PngEncoder`, :class:`esmstereo_amd.render.JpegEncoder`) share: the
    buffers for batches of up to ``B`` images of one ``shape`` (the workspace, one output slot per image, the device
    length array and a pinned host mirror of both, allocated once so that repeated frames allocate nothing), the
    input checks, the read-back and the cache of encoders.

    A call enqueues the codec's three launches and the copy of the lengths, synchronises ONCE to read them
    (:meth:`_lengths`), then copies ``length`` bytes per image into the pinned mirror (:meth:`_copy`)."""

    _module, _codec, _noun, _unit, _least = "esmstereo_amd.io", "png", "image", "stream", 1
    _size = "{} rows of {} bytes"
    _cache = {}  # one for both codecs: (class, constructor arguments, device) -> encoder, at most 8

    def __init__(self, B: int, shape, device) -> None:
        self.B, self.shape = int(B), tuple(int(v) for v in shape)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{self._module}: {type(self).__name__} runs on the GPU (no CPU fallback)")

    def _allocate(self, nwork: int, slot: int) -> None:
        self.work = torch.empty(nwork, device=self.device, dtype=torch.uint8)
        self.lengths = torch.empty(self.B, device=self.device, dtype=torch.int32)
        self.host_lengths = torch.empty(self.B, dtype=torch.int32, pin_memory=True)
        self._slots(slot)

    def _slots(self, slot: int) -> None:
        self.slot = slot
        self.out = torch.empty(self.B, slot, device=self.device, dtype=torch.uint8)
        self.host = torch.empty(self.B, slot, dtype=torch.uint8, pin_memory=True)

    @classmethod
    def cached(cls, *args, device):
        """The cached encoder ``cls(*args, device=device)`` (a per-frame loop reuses one set of buffers)."""
        key = (cls, args, str(torch.device(device)))
        if key not in cls._cache:
            if len(cls._cache) >= 8:
                cls._cache.pop(next(iter(cls._cache)))
            cls._cache[key] = cls(*args, device=device)
        return cls._cache[key]

    @classmethod
    def _on_gpu(cls, what: str, t) -> None:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: expected a torch tensor on the GPU")
        if not t.is_cuda:
            raise RuntimeError(f"{cls._module}: {what}: the {cls._noun} must be on the GPU (no CPU fallback)")

    @classmethod
    def _frames(cls, what: str, frames, order: str) -> torch.Tensor:
        """uint8 ``[B, h, w, 3]`` / ``[h, w, 3]`` on the GPU, channels in ``order`` -> contiguous ``[B, h, w, 3]``."""
        if order not in ("bgr", "rgb"):
            raise ValueError(f"{what}: order must be 'bgr' or 'rgb', got {order!r}")
        cls._on_gpu(what, frames)
        if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
            raise ValueError(f"{what}: expected a uint8 [B, h, w, 3] or [h, w, 3] tensor")
        return (frames.unsqueeze(0) if frames.dim() == 3 else frames).contiguous()

    def _fits(self, what: str, t: torch.Tensor, shape) -> int:
        """The number of images in the batch ``t`` of ``shape``, which must be this encoder's, on its device."""
        if t.device != self.work.device:
            raise RuntimeError(f"{self._module}: {what}: the {self._noun} is on {t.device}, the encoder on "
                               f"{self.work.device}")
        n = int(t.shape[0])
        if n < 1 or n > self.B or tuple(shape) != self.shape:
            raise ValueError(f"{what}: this encoder takes 1..{self.B} {self._noun}s of "
                             f"{self._size.format(*self.shape)}, got {n} of {self._size.format(*shape)}")
        return n

    def _lengths(self, n: int) -> list:
        self.host_lengths[:n].copy_(self.lengths[:n], non_blocking=True)
        torch.cuda.current_stream(self.work.device).synchronize()  # the one synchronisation: the lengths
        return self.host_lengths[:n].tolist()

    def _copy(self, lengths) -> list:
        streams = []
        for b, length in enumerate(lengths):
            if not self._least <= length <= self.slot:
                raise RuntimeError(f"{self._codec}: {self._noun} {b}: {self._unit} length {length} outside the slot of "
                                   f"{self.slot} bytes")
            self.host[b, :length].copy_(self.out[b, :length])
            streams.append(self.host[b, :length].numpy().tobytes())
        return streams


class PngEncoder(_DeviceEncoder):
    """The device PNG encoder for batches of up to ``B`` images of ``rows`` rows of ``row_bytes`` sample bytes
    (``2 * w`` for a 16-bit map, ``3 * w`` for a colour frame): :class:`_DeviceEncoder`'s buffers with slots of
    ``esm_png_stream_bound`` bytes; the streams read back are wrapped on the host (:func:`png_wrap`)."""

    def __init__(self, B: int, rows: int, row_bytes: int, device="cuda"):
        super().__init__(B, (rows, row_bytes), device)
        self.rows, self.row_bytes = self.shape
        nwork = check(lib.esm_png_workspace_bytes(self.B, self.rows, self.row_bytes), "png_workspace_bytes")
        self._allocate(nwork, check(lib.esm_png_stream_bound(self.rows * (1 + self.row_bytes)), "png_stream_bound"))

    def _args(self, filter):
        return (self.work.data_ptr(), self.out.data_ptr(), self.slot, self.lengths.data_ptr(), _png_filter(filter),
                _stream(self.work))

    def _streams(self, n: int) -> list:
        return self._copy(self._lengths(n))

    @classmethod
    def _maps(cls, a) -> torch.Tensor:
        cls._on_gpu("png_encode_u16", a)
        if a.dtype not in (torch.uint16, torch.int16) or a.dim() not in (2, 3):
            raise ValueError("png_encode_u16: expected a uint16 [B, h, w] or [h, w] tensor")
        return (a.unsqueeze(0) if a.dim() == 2 else a).contiguous()

    @classmethod
    def _disp(cls, disp) -> torch.Tensor:
        cls._on_gpu("png_encode_disparity", disp)
        if disp.dim() == 4 and disp.shape[1] == 1:
            disp = disp[:, 0]
        if disp.dim() == 2:
            disp = disp.unsqueeze(0)
        if disp.dim() != 3 or disp.dtype != torch.float32:
            raise ValueError("png_encode_disparity: expected a float32 [B, H, W] tensor")
        return disp.contiguous()

    def _encode(self, what: str, entry, a: torch.Tensor, args, h: int, w: int, bpp: int, filter) -> list:
        """``entry`` on the checked batch ``a`` of ``h`` x ``w`` images of ``bpp`` bytes a pixel -> one PNG each."""
        n = self._fits(what, a, (h, bpp * w))
        with torch.cuda.device(self.work.device):
            check(entry(a.data_ptr(), n, *args, *self._args(filter)), what)
            return [png_wrap(s, w, h, *((16, 0) if bpp == 2 else (8, 2))) for s in self._streams(n)]

    def encode_u16(self, a: torch.Tensor, filter="sub") -> list:
        """uint16 (or int16 bit patterns) ``[B, h, w]`` / ``[h, w]`` on the GPU -> one 16-bit grayscale PNG each."""
        return self._u16(self._maps(a), filter)

    def _u16(self, a: torch.Tensor, filter) -> list:
        h, w = int(a.shape[1]), int(a.shape[2])
        return self._encode("png_encode_u16", lib.esm_png_encode_u16, a, (h, w), h, w, 2, filter)

    def encode_disparity(self, disp: torch.Tensor, top: int, left: int, h: int, w: int, filter="sub") -> list:
        """float32 ``[B, Hp, Wp]`` on the GPU -> the PNGs of ``disparity_to_u16(disp, top, left, h, w)``, rounded
        inside the encoder: the uint16 map is never stored."""
        return self._disparity(self._disp(disp), top, left, h, w, filter)

    def _disparity(self, disp: torch.Tensor, top: int, left: int, h: int, w: int, filter) -> list:
        args = (int(disp.shape[1]), int(disp.shape[2]), int(top), int(left), int(h), int(w))
        return self._encode("png_encode_disparity", lib.esm_png_encode_disp_f32, disp, args, int(h), int(w), 2, filter)

    def encode_rgb8(self, frames: torch.Tensor, order: str = "bgr", filter="sub") -> list:
        """uint8 ``[B, h, w, 3]`` / ``[h, w, 3]`` on the GPU, channels in ``order`` -> one 8-bit colour PNG each."""
        return self._rgb8(self._frames("png_encode_bgr8", frames, order), order, filter)

    def _rgb8(self, a: torch.Tensor, order: str, filter) -> list:
        h, w = int(a.shape[1]), int(a.shape[2])
        return self._encode("png_encode_bgr8", lib.esm_png_encode_rgb8, a, (h, w, int(order == "bgr")), h, w, 3, filter)


def png_encoder(B: int, rows: int, row_bytes: int, device) -> PngEncoder:
    """The cached :class:`PngEncoder` of this batch, shape and device (a per-frame loop reuses one set of buffers)."""
    return PngEncoder.cached(int(B), int(rows), int(row_bytes), device=device)


def png_encode_u16(a: torch.Tensor, filter="sub") -> list:
    """One 16-bit grayscale PNG (``bytes``) per map of uint16 ``[B, h, w]`` / ``[h, w]`` on the GPU, encoded there:
    PNG filter ``filter`` (``"none"``, ``"sub"``, ``"up"``) and a Huffman-only deflate block, no LZ77.  Any PNG reader
    opens it; the pixels are exact.  Only the compressed bytes cross to the host."""
    a = PngEncoder._maps(a)
    return png_encoder(a.shape[0], a.shape[1], 2 * a.shape[2], a.device)._u16(a, filter)


def png_encode_disparity(disp: torch.Tensor, top: int, left: int, h: int, w: int, filter="sub") -> list:
    """``png_encode_u16(disparity_to_u16(disp, top, left, h, w))``, byte for byte, with the rounding done inside the
    encoder's launches (save_disp.py:81-86 in one call)."""
    disp = PngEncoder._disp(disp)
    return png_encoder(disp.shape[0], h, 2 * int(w), disp.device)._disparity(disp, top, left, h, w, filter)


def write_png_u16_device(paths, a: torch.Tensor, filter="sub") -> None:
    """``write_png_u16`` for a device-resident batch: ``paths[b]`` receives map ``b`` of :func:`png_encode_u16`."""
    paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
    files = png_encode_u16(a, filter)
    if len(paths) != len(files):
        raise ValueError(f"write_png_u16_device: {len(paths)} paths for {len(files)} maps")
    for path, data in zip(paths, files):
        with open(path, "wb") as f:
            f.write(data)
