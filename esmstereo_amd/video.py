"""The nodes' video file: Motion-JPEG in an AVI, with the frames compressed on the device.

All four reference nodes open ``cv::VideoWriter`` with ``fourcc('M','J','P','G')`` and call
``video_writer.write(combined)`` once per frame on the stacked picture (kitti_publisher_cuda_node.cpp:122-132,
kitti_publisher_conf_cuda_node.cpp:265-275, virtual_kitti_publisher_cuda_node.cpp:218-228,
kitti_publisher_ess_cuda_node.cpp:227-237).  That picture is ``node.dev_frame`` here (``dev_panels`` for the
confidence node's four panels) and never needs to leave the device raw: :class:`MjpegWriter` compresses it with
:class:`esmstereo_amd.render.JpegEncoder` (``csrc/jpeg.hip``) and appends the JFIF file to a plain RIFF AVI:

    RIFF 'AVI '
      LIST 'hdrl'   'avih' (56 bytes)   LIST 'strl'   'strh' (56 bytes: 'vids' / 'MJPG')   'strf' (40 bytes:
                                                       BITMAPINFOHEADER, 24 bit, 'MJPG')
      LIST 'movi'   one '00dc' chunk per frame, padded to an even length
      'idx1'        per frame: '00dc', AVIIF_KEYFRAME, the chunk's offset from the 'movi' fourcc, its length

The sizes and frame counts are patched when the file is closed.  This is the AVI 1.0 layout, below 2 GiB; a file that
would pass that raises (OpenDML is out of scope).  UNPINNED: no player and no cv2 is importable where this package is
built or tested, so what is tested is the layout (tests/jpeg_ref.py's RIFF walker) and that every frame decodes with
PIL, not playback in a given player.
"""
from __future__ import annotations

import struct
from typing import Optional

import torch

from .render import JpegEncoder

__all__ = ["MjpegWriter"]

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
MAX_FILE = (1 << 31) - 1
_HEADER_BYTES = 12 + 12 + 8 + 56 + 12 + 8 + 56 + 8 + 40 + 12  # up to and including LIST size 'movi'


def jpeg_size(data: bytes):
    """(width, height) from the frame header (SOF0-SOF2) of a JPEG file."""
    if data[:2] != b"\xff\xd8":
        raise ValueError("MjpegWriter: not a JPEG file (no SOI)")
    pos = 2
    while pos + 4 <= len(data):
        if data[pos] != 0xFF:
            raise ValueError(f"MjpegWriter: no marker at byte {pos}")
        marker, size = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
        if marker in (0xC0, 0xC1, 0xC2):
            h, w = struct.unpack_from(">HH", data, pos + 5)
            return w, h
        if marker == 0xDA:
            break
        pos += 2 + size
    raise ValueError("MjpegWriter: no frame header before the scan")


class MjpegWriter:
    """``cv::VideoWriter(path, fourcc('M','J','P','G'), fps, size)`` for device-resident frames.

    ``write(frame)`` takes a uint8 ``[H, W, 3]`` BGR tensor on the GPU (``node.dev_frame`` after
    ``process_rendered`` / ``dev_panels`` after ``process_scored``) and compresses it there at ``quality`` /
    ``subsampling``; the first frame fixes the size and a frame of another size raises.  ``write_jpeg(data)`` appends
    a ready JPEG file.  ``close()`` (or leaving the ``with`` block) writes the index and patches the headers."""

    def __init__(self, path: str, fps: float = 30, quality: int = 75, subsampling="420"):
        if not fps > 0:
            raise ValueError(f"MjpegWriter: fps must be positive, got {fps}")
        self.path, self.fps, self.quality, self.subsampling = path, float(fps), int(quality), subsampling
        self.size = None  # (w, h)
        self.encoder: Optional[JpegEncoder] = None
        self.index = []   # (offset from the 'movi' fourcc, length)
        self.max_chunk = 0
        self.f = open(path, "wb")
        self.closed = False

    # -- frames
    def write(self, frame: torch.Tensor) -> None:
        if not isinstance(frame, torch.Tensor) or frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise ValueError("MjpegWriter.write: expected a uint8 [H, W, 3] tensor")
        if not frame.is_cuda:
            raise RuntimeError("esmstereo_amd.video: MjpegWriter.write: the frame must be on the GPU (no CPU fallback; "
                               "write_jpeg appends ready bytes)")
        h, w = int(frame.shape[0]), int(frame.shape[1])
        if self.size is not None and (w, h) != self.size:
            raise ValueError(f"MjpegWriter.write: this file holds {self.size[1]} x {self.size[0]} frames, got "
                             f"{h} x {w}")
        if self.encoder is None:
            self.encoder = JpegEncoder(1, h, w, self.quality, self.subsampling, device=frame.device)
        self.write_jpeg(self.encoder.encode(frame, "bgr")[0])

    def write_jpeg(self, data: bytes) -> None:
        if self.closed:
            raise ValueError("MjpegWriter: the file is closed")
        data = bytes(data)
        size = jpeg_size(data)
        if self.size is None:
            self.size = size
            self.f.write(b"\0" * _HEADER_BYTES)  # patched by close()
        elif size != self.size:
            raise ValueError(f"MjpegWriter.write_jpeg: this file holds {self.size[1]} x {self.size[0]} frames, got "
                             f"{size[1]} x {size[0]}")
        pos = self.f.tell()
        padded = len(data) + (len(data) & 1)
        if pos + 8 + padded + 8 + 16 * (len(self.index) + 1) > MAX_FILE:
            raise ValueError("MjpegWriter: the file would pass 2 GiB (AVI 1.0; OpenDML is not written)")
        self.index.append((pos - (_HEADER_BYTES - 4), len(data)))
        self.f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1))
        self.max_chunk = max(self.max_chunk, len(data))

    # -- the file
    def _headers(self, movi_bytes: int) -> bytes:
        w, h = self.size or (0, 0)
        n = len(self.index)
        usec = int(round(1e6 / self.fps))
        rate, scale = int(round(self.fps * 1000)), 1000
        total = sum(length for _, length in self.index)
        avih = struct.pack("<14I", usec, int(total * self.fps / n) if n else 0, 0, AVIF_HASINDEX, n, 0, 1,
                           self.max_chunk, w, h, 0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, n, self.max_chunk, 0xFFFFFFFF,
                                         0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", 3 * w * h, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        riff_size = _HEADER_BYTES - 8 + movi_bytes + 8 + 16 * n
        out = (b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
               b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi")
        assert len(out) == _HEADER_BYTES and len(avih) == 56 and len(strh) == 56
        return out

    def close(self) -> None:
        if self.closed:
            return
        self.closed = True
        try:
            if self.size is None:
                self.f.write(b"\0" * _HEADER_BYTES)
            movi_bytes = self.f.tell() - _HEADER_BYTES
            idx = b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, off, length) for off, length in self.index)
            self.f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
            self.f.seek(0)
            self.f.write(self._headers(movi_bytes))
        finally:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
