"""Rendering a disparity on the device: the colour-mapped 8-bit frame and the depth map.

Every reference script that produces a disparity ends in scoring (:mod:`esmstereo_amd.metrics`), the 16-bit PNG
(:func:`esmstereo_amd.io.disparity_to_u16`) or the picture; this module is the picture.  One launch
(``csrc/render.hip``) turns a device-resident fp32 disparity into a ``uint8 [B, H, W, 3]`` frame through a
256-entry colour table, optionally stacked under the left image, so 3 bytes a pixel come back to the host instead
of 4 and nothing is colourised on the CPU:

* :func:`colorize_disparity` — save_vid.py:118-125, save_disp.py:87-97, test_mid.py:118-121, test_eth3d.py:102-105:
  ``cv2.applyColorMap(cv2.convertScaleAbs(np.round(d * 256).astype(np.uint16), alpha=0.01), cv2.COLORMAP_JET)``;
  ``stack=left`` is save_vid.py:125 ``np.concatenate((left_img, disp_np), 0)``.
* :func:`colorize_range` — kitti_publisher_cuda_node.cpp:81-86,117-118: ``minMaxLoc`` over the valid mask,
  ``convertTo(CV_8UC1, -255 / (max - min), 255 * max / (max - min))``, ``COLORMAP_MAGMA``, ``vconcat``.  The range
  is found on the device and never leaves it.  Defined here: an image with no valid pixel or with max == min (the
  reference divides by zero) maps every pixel to index 0.
* :func:`disparity_to_depth`, :func:`colorize_depth` — latest.py:56-63, fp32 throughout, bit-exact with the numpy
  lines.  Defined here: a NaN depth takes index 255 (``uint8`` 0).  latest.py:55 (``np.where(d <= 0, 1e-6, d)``)
  is the caller's step.

The index definitions are in ``include/esmstereo_amd.h``.  The arithmetic in front of the table restates OpenCV's
documented semantics (``saturate_cast``: round half to even, then clamp), as ``esm_node_filter_u16`` does for
``medianBlur`` and ``convertTo``.  Parity against OpenCV's own output is UNPINNED: cv2 is importable nowhere this
package is built or tested.  The table is an argument for that reason: :func:`colormap_lut` ships matplotlib's
``jet`` and ``magma``; a caller with cv2 passes cv2's own table.

:func:`png_rgb8_bytes` / :func:`write_png_bgr8` write such a frame as an 8-bit colour PNG, which is what
``cv2.imwrite`` does with it.  :class:`JpegEncoder` / :func:`jpeg_encode_bgr8` compress such a frame as a baseline
JPEG on the device (``csrc/jpeg.hip``), which is what the nodes' MJPG ``cv::VideoWriter`` does with it per frame;
:mod:`esmstereo_amd.video` puts those files into an AVI.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import json
import os
import zlib
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import COLORIZE_DEPTH, COLORIZE_RANGE, COLORIZE_SCALE, PKG, check, lib, _stream
from .io import PngEncoder, _DeviceEncoder, png_encoder, png_wrap

__all__ = ["colormap_lut", "colorize_disparity", "colorize_range", "range_workspace_bytes", "disparity_to_depth",
           "colorize_depth", "png_rgb8_bytes", "write_png_bgr8", "png_encode_bgr8", "JpegEncoder", "jpeg_encode_bgr8",
           "jpeg_header"]

COLORMAPS_PATH = os.path.join(PKG, "colormaps.json")
_tables = {}


def colormap_lut(name: str, device="cuda", order: str = "bgr") -> torch.Tensor:
    """The shipped table ``name`` (``"jet"`` or ``"magma"``) as uint8 ``[256, 3]`` on ``device``, in channel order
    ``"bgr"`` (OpenCV frames, the default) or ``"rgb"``.

    The tables are matplotlib's (3.10.8: ``rint(cmap(arange(256))[:, :3] * 255)``, scripts/make_colormaps.py), read
    from ``esmstereo_amd/colormaps.json`` (text: 256 ``rrggbb`` entries per table); matplotlib is not imported.
    OpenCV's ``COLORMAP_JET`` differs from matplotlib's ``jet``: for OpenCV's bytes pass cv2's own table,
    ``torch.from_numpy(cv2.applyColorMap(np.arange(256, dtype=np.uint8), code)[:, 0].copy()).to(device)``."""
    if order not in ("bgr", "rgb"):
        raise ValueError(f"colormap_lut: order must be 'bgr' or 'rgb', got {order!r}")
    if not _tables:
        with open(COLORMAPS_PATH) as f:
            doc = json.load(f)
        for k, rows in doc.items():
            if isinstance(rows, list):
                t = np.frombuffer(bytes.fromhex("".join(rows).replace(" ", "")), dtype=np.uint8).reshape(256, 3)
                _tables[k] = t.copy()
    if name not in _tables:
        raise KeyError(f"colormap_lut: no table {name!r}; shipped: {sorted(_tables)}")
    t = _tables[name]
    return torch.from_numpy(np.ascontiguousarray(t[:, ::-1] if order == "bgr" else t)).to(device)


def _disp_view(disp: torch.Tensor, what: str) -> Tuple[torch.Tensor, bool]:
    """``[B, H, W]`` view of ``[B, H, W]`` / ``[B, 1, H, W]`` / ``[H, W]`` where it lies (copied only when W is
    strided), and whether the input was a single ``[H, W]`` map."""
    single = disp.dim() == 2
    if disp.dim() == 4 and disp.shape[1] == 1:
        disp = disp[:, 0]
    elif single:
        disp = disp.unsqueeze(0)
    if disp.dim() != 3 or disp.dtype != torch.float32:
        raise ValueError(f"{what}: expected a float32 [B, H, W], [B, 1, H, W] or [H, W] tensor, got "
                         f"{disp.dtype} {tuple(disp.shape)}")
    if not disp.is_cuda:
        raise RuntimeError(f"esmstereo_amd.render: {what} must be on the GPU (no CPU fallback)")
    if disp.shape[2] > 1 and disp.stride(2) != 1:
        disp = disp.contiguous()
    return disp, single


def _check_lut(lut: torch.Tensor, dev: torch.device) -> torch.Tensor:
    if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise ValueError("esmstereo_amd.render: lut must be a uint8 [256, 3] tensor (see colormap_lut)")
    if lut.device != dev:
        raise RuntimeError("esmstereo_amd.render: lut must be on the disparity's device (no CPU fallback)")
    return lut.contiguous()


def _colorize(disp: torch.Tensor, lut: torch.Tensor, mode: int, stack: Optional[torch.Tensor], what: str,
              alpha: float = 0.0, num: float = 0.0, max_depth: float = 0.0,
              out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    disp, single = _disp_view(disp, what)
    B, H, W = (int(v) for v in disp.shape)
    dev = disp.device
    lut = _check_lut(lut, dev)
    top = None
    if stack is not None:
        top = stack.unsqueeze(0) if stack.dim() == 3 else stack
        if top.dtype != torch.uint8 or tuple(top.shape) != (B, H, W, 3):
            raise ValueError(f"{what}: stack must be uint8 {(B, H, W, 3)}, got {top.dtype} {tuple(top.shape)}")
        if top.device != dev:
            raise RuntimeError(f"esmstereo_amd.render: {what}: stack must be on the disparity's device")
        top = top.contiguous()
    hout = 2 * H if top is not None else H
    if out is None:
        out = torch.empty(B, hout, W, 3, device=dev, dtype=torch.uint8)
    elif (out.dtype != torch.uint8 or out.device != dev or out.numel() != B * hout * W * 3
          or not out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous uint8 tensor of {B * hout * W * 3} elements on {dev}")
    work = None
    if mode == COLORIZE_RANGE:
        nbytes = check(lib.esm_disp_colorize_workspace(B, H, W), "disp_colorize_workspace")
        work = workspace if workspace is not None else torch.empty(nbytes, device=dev, dtype=torch.uint8)
        if (work.dtype != torch.uint8 or work.device != dev or work.numel() < nbytes or not work.is_contiguous()
                or work.data_ptr() % 8):
            raise ValueError(f"{what}: workspace must be a contiguous, 8-byte aligned uint8 tensor of >= {nbytes} "
                             f"elements on {dev}")
    with torch.cuda.device(dev):
        check(lib.esm_disp_colorize_u8(disp.data_ptr(), disp.stride(0), disp.stride(1), B, H, W, mode, float(alpha),
                                       float(num), float(max_depth), lut.data_ptr(),
                                       top.data_ptr() if top is not None else None, out.data_ptr(),
                                       work.data_ptr() if work is not None else None, _stream(disp)), what)
    out = out.view(B, hout, W, 3)
    return out[0] if single else out


def colorize_disparity(disp: torch.Tensor, lut: torch.Tensor, alpha: float = 0.01,
                       stack: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``cv2.applyColorMap(cv2.convertScaleAbs(np.round(disp * 256).astype(np.uint16), alpha=alpha), table)`` on
    the device (save_vid.py:119-122, save_disp.py:87-97, test_mid.py:118-121, test_eth3d.py:102-105).

    ``disp``: float32 ``[B, H, W]``, ``[B, 1, H, W]`` or ``[H, W]``; a crop such as ``pred[:, top:, left:]`` is
    read where it lies.  ``lut``: uint8 ``[256, 3]`` in the output's channel order.  ``stack``: uint8
    ``[B, H, W, 3]`` (``[H, W, 3]`` for a single map) to put on top (save_vid.py:125).  Returns uint8
    ``[B, H or 2H, W, 3]`` (``[H or 2H, W, 3]`` for ``[H, W]``)."""
    return _colorize(disp, lut, COLORIZE_SCALE, stack, "colorize_disparity", alpha=alpha)


def colorize_range(filtered: torch.Tensor, lut: torch.Tensor, stack: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The node's picture (kitti_publisher_cuda_node.cpp:81-86,117-118) of the masked median map ``filtered`` that
    ``esm_node_filter_u16`` writes (invalid pixels exactly 0): each image's own min and max over ``filtered > 0``
    map to indices 255 and 0.  Shapes as :func:`colorize_disparity`.  A per-frame loop passes its own buffers:
    ``out`` receives the frame, ``workspace`` (uint8, :func:`range_workspace_bytes` elements) holds the partial
    ranges; both are allocated per call when absent."""
    return _colorize(filtered, lut, COLORIZE_RANGE, stack, "colorize_range", out=out, workspace=workspace)


def range_workspace_bytes(B: int, H: int, W: int) -> int:
    """Bytes of the ``workspace`` :func:`colorize_range` takes for a ``[B, H, W]`` batch."""
    return check(lib.esm_disp_colorize_workspace(int(B), int(H), int(W)), "disp_colorize_workspace")


def _num(baseline: float, focal: float) -> float:
    return float(np.float32(float(baseline) * float(focal)))  # the double product, rounded once


def disparity_to_depth(disp: torch.Tensor, baseline: float, focal: float, max_depth: float) -> torch.Tensor:
    """``np.clip((baseline * focal) / disp, 0, max_depth)`` for a float32 map (latest.py:56-57), bit-exact:
    ``disp == 0`` gives ``max_depth``, a negative disparity 0, NaN stays.  Same shape as ``disp``."""
    d, _ = _disp_view(disp, "disparity_to_depth")
    B, H, W = (int(v) for v in d.shape)
    out = torch.empty(B, H, W, device=d.device, dtype=torch.float32)
    with torch.cuda.device(d.device):
        check(lib.esm_disp_to_depth_f32(d.data_ptr(), d.stride(0), d.stride(1), out.data_ptr(), B, H, W,
                                        _num(baseline, focal), float(max_depth), _stream(d)),
              "disparity_to_depth")
    return out.view(disp.shape)


def colorize_depth(disp: torch.Tensor, baseline: float, focal: float, max_depth: float, lut: torch.Tensor,
                   stack: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``create_depth_colormap(disparity_to_depth_map(disp, ...))`` of latest.py:56-63 in one launch: index
    ``255 - uint8(clip(depth / max_depth, 0, 1) * 255)`` through ``lut``.  Shapes as :func:`colorize_disparity`."""
    return _colorize(disp, lut, COLORIZE_DEPTH, stack, "colorize_depth", num=_num(baseline, focal),
                     max_depth=max_depth)


def png_rgb8_bytes(a: np.ndarray, order: str = "bgr") -> bytes:
    """An 8-bit truecolour PNG (colour type 2, zlib-deflated, filter 0 per row) of ``a`` ``[H, W, 3]`` uint8 whose
    channels are in ``order``: the colour twin of :func:`esmstereo_amd.io.png_u16_bytes`."""
    if order not in ("bgr", "rgb"):
        raise ValueError(f"png_rgb8_bytes: order must be 'bgr' or 'rgb', got {order!r}")
    a = np.asarray(a)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError("png_rgb8_bytes: expected a uint8 [H, W, 3] array")
    h, w, _ = a.shape
    raw = np.empty((h, 1 + 3 * w), dtype=np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = (a[:, :, ::-1] if order == "bgr" else a).reshape(h, 3 * w)
    return png_wrap(zlib.compress(raw.tobytes(), 6), w, h, 8, 2)


def png_encode_bgr8(frames: torch.Tensor, order: str = "bgr", filter="sub") -> list:
    """One 8-bit colour PNG (``bytes``) per frame of uint8 ``[B, H, W, 3]`` / ``[H, W, 3]`` on the GPU whose channels
    are in ``order``, encoded on the device (``csrc/png.hip``: PNG filter ``filter`` and a Huffman-only deflate
    block): the device twin of :func:`png_rgb8_bytes`; see :func:`esmstereo_amd.io.png_encode_u16`."""
    a = PngEncoder._frames("png_encode_bgr8", frames, order)
    return png_encoder(a.shape[0], a.shape[1], 3 * a.shape[2], a.device)._rgb8(a, order, filter)


JPEG_SUBSAMPLINGS = {"420": 420, "444": 444, 420: 420, 444: 444}


def _jpeg_params(what: str, quality, subsampling, restart_mcus):
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"{what}: subsampling must be '420' or '444', got {subsampling!r}")
    quality, restart_mcus = int(quality), int(restart_mcus)
    if not 1 <= quality <= 100:
        raise ValueError(f"{what}: quality must be 1..100, got {quality}")
    if not 1 <= restart_mcus <= 16:
        raise ValueError(f"{what}: restart_mcus must be 1..16, got {restart_mcus}")
    return quality, JPEG_SUBSAMPLINGS[subsampling], restart_mcus


def jpeg_header(w: int, h: int, quality: int = 75, subsampling="420", restart_mcus: int = 8) -> bytes:
    """The JFIF header (SOI .. SOS, 629 bytes) that goes in front of a scan of :class:`JpegEncoder`: a host-only call
    of ``esm_jpeg_header`` (``include/esmstereo_amd.h`` lists the segments)."""
    quality, sub, ri = _jpeg_params("jpeg_header", quality, subsampling, restart_mcus)
    buf = (ctypes.c_uint8 * 1024)()
    n = check(lib.esm_jpeg_header(buf, 1024, int(w), int(h), quality, sub, ri), "jpeg_header")
    return bytes(buf[:n])


class JpegEncoder(_DeviceEncoder):
    """The device JPEG encoder (``csrc/jpeg.hip``) for batches of up to ``B`` frames of ``h`` x ``w``: the
    :class:`esmstereo_amd.io.PngEncoder` of the nodes' MJPG writer (``kitti_publisher_cuda_node.cpp:122-132`` and its
    three siblings), on the same buffers and read-back (:class:`esmstereo_amd.io._DeviceEncoder`).

    The host-built header goes in front of each scan read back.  The default slot is the raw size ``3 * h * w``; a
    frame whose scan is longer (noise at quality 100) is reported by the library as a negative length, and the
    encoder then re-encodes once into slots of ``esm_jpeg_stream_bound`` bytes, which it keeps."""

    _module, _codec, _noun, _unit, _least, _size = "esmstereo_amd.render", "jpeg", "frame", "scan", 2, "{} x {}"

    def __init__(self, B: int, h: int, w: int, quality: int = 75, subsampling="420", restart_mcus: int = 8,
                 slot_bytes: Optional[int] = None, device="cuda"):
        self.quality, self.sub, self.ri = _jpeg_params("JpegEncoder", quality, subsampling, restart_mcus)
        super().__init__(B, (h, w), device)
        self.h, self.w = self.shape
        slot = 3 * self.h * self.w if slot_bytes is None else int(slot_bytes)
        if slot < 2:
            raise ValueError(f"JpegEncoder: slot_bytes must be at least 2, got {slot}")
        nwork = check(lib.esm_jpeg_workspace_bytes(self.B, self.h, self.w, self.sub, self.ri), "jpeg_workspace_bytes")
        self.bound = check(lib.esm_jpeg_stream_bound(self.h, self.w, self.sub, self.ri), "jpeg_stream_bound")
        self.header = jpeg_header(self.w, self.h, self.quality, self.sub, self.ri)
        self._allocate(nwork, slot)

    def _launch(self, a: torch.Tensor, n: int, bgr: bool) -> list:
        """The three launches and the one synchronisation: the lengths of the ``n`` scans."""
        check(lib.esm_jpeg_encode_rgb8(a.data_ptr(), n, self.h, self.w, int(bgr), self.quality, self.sub, self.ri,
                                       self.work.data_ptr(), self.out.data_ptr(), self.slot, self.lengths.data_ptr(),
                                       _stream(self.work)), "jpeg_encode_rgb8")
        return self._lengths(n)

    def encode(self, frames: torch.Tensor, order: str = "bgr") -> list:
        """uint8 ``[B, h, w, 3]`` / ``[h, w, 3]`` on the GPU, channels in ``order`` -> one JFIF file (``bytes``)
        each."""
        return self._encode(self._frames("jpeg_encode_bgr8", frames, order), order)

    def _encode(self, a: torch.Tensor, order: str) -> list:
        n = self._fits("jpeg_encode_bgr8", a, a.shape[1:3])
        with torch.cuda.device(self.work.device):
            lengths = self._launch(a, n, order == "bgr")
            if min(lengths) < 0:  # a scan longer than its slot: once more, into slots that hold any scan
                self._slots(self.bound)
                lengths = self._launch(a, n, order == "bgr")
            return [self.header + s for s in self._copy(lengths)]


def jpeg_encode_bgr8(frames: torch.Tensor, quality: int = 75, subsampling="420", order: str = "bgr") -> list:
    """One complete baseline JFIF file (``bytes``) per frame of uint8 ``[B, H, W, 3]`` / ``[H, W, 3]`` on the GPU whose
    channels are in ``order``, encoded on the device (``csrc/jpeg.hip``): what ``cv::VideoWriter`` with
    ``fourcc('M','J','P','G')`` compresses per ``write`` (``kitti_publisher_cuda_node.cpp:122-132``).  The encoder of
    each batch, shape and setting is cached (:class:`JpegEncoder`, restart interval 8).  There is no CPU fallback."""
    a = JpegEncoder._frames("jpeg_encode_bgr8", frames, order)
    enc = JpegEncoder.cached(*(int(v) for v in a.shape[:3]), int(quality), str(subsampling), device=a.device)
    return enc._encode(a, order)


def write_png_bgr8(path: str, a) -> None:
    """``cv2.imwrite(path, frame)`` for a BGR uint8 ``[H, W, 3]`` frame (save_disp.py:91-97, test_mid.py:119)."""
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    with open(path, "wb") as f:
        f.write(png_rgb8_bytes(a, "bgr"))
