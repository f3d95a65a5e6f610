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
"""
from __future__ import annotations

import ctypes
import struct
import zlib
from typing import Sequence, Tuple

import numpy as np
import torch

from ._lib import check, lib

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


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


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

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) +
            chunk(b"IEND", b""))


def write_png_u16(path: str, a) -> None:
    """``skimage.io.imsave(fn, disp_est_uint)`` of save_disp.py:86 for a uint16 map."""
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    with open(path, "wb") as f:
        f.write(png_u16_bytes(a))
