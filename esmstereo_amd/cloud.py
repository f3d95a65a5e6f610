"""Point clouds on the device: a disparity map reprojected to XYZ(RGB), compacted and coloured (``csrc/cloud.hip``).

The reference node has the camera (``fx``, ``baseline``: ``kitti_publisher_cuda_node.cpp:60-78,277-278``) and
``latest.py:54-58`` turns the disparity into depth; the 3-D points are the step a consumer runs next, and on the host
it is a download of the full fp32 map and the frame, a reprojection and a boolean mask in numpy.  Here it is one plan
op (``esm_plan_add_cloud``; the definition is ``esm_cloud_desc``'s comment in include/esmstereo_amd.h): per candidate
pixel ``Z = num / d``, ``X = (x - cx) * Z / fx``, ``Y = (y - cy) * Z / fy`` in fp32, kept when ``d > 0``, ``z_min <= Z
<= z_max`` and the optional ``valid`` byte is set, written densely in raster order.  Only the kept points cross to the
host.  Rectified pinhole only: no 4 x 4 Q matrix, no filtering, no normals.

:class:`CloudBuilder` owns the plan, the workspace, one slot of records per image, the device counts and pinned
mirrors (:class:`esmstereo_amd.io._DeviceEncoder`'s buffers and read-back), so repeated frames allocate nothing;
:func:`disparity_to_points` is the cached convenience call; :func:`ply_bytes` / :func:`write_ply` put the records of
the ``"ply"`` packing behind a ``binary_little_endian 1.0`` header verbatim.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional

import numpy as np
import torch

from ._lib import CLOUD_PACK_PCL, CLOUD_PACK_PLY, EsmCloudDesc, c_void_p, check, lib, _stream
from .io import _DeviceEncoder
from .render import _num

__all__ = ["Camera", "CloudBuilder", "disparity_to_points", "ply_bytes", "write_ply", "point_dtype"]

PACKINGS = {"ply": CLOUD_PACK_PLY, "pcl": CLOUD_PACK_PCL}
_XYZ = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
_DTYPES = {None: np.dtype(_XYZ),
           "ply": np.dtype(_XYZ + [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]),
           "pcl": np.dtype(_XYZ + [("rgb", "<u4")])}


def point_dtype(color: bool, packing: str = "ply") -> np.dtype:
    """The structured dtype of one record: ``x, y, z`` float32, then ``red, green, blue, alpha`` uint8 (``"ply"``) or
    ``rgb`` uint32 ``0x00RRGGBB`` (``"pcl"``, the ``rgb`` field of a ROS ``PointCloud2``) when coloured."""
    if packing not in PACKINGS:
        raise ValueError(f"cloud: packing must be one of {sorted(PACKINGS)}, got {packing!r}")
    return _DTYPES[packing if color else None]


class Camera:
    """A rectified pinhole camera: focal lengths ``fx``, ``fy`` and principal point ``cx``, ``cy`` in pixels,
    ``baseline`` in the unit the points come out in.  DEFINED HERE: ``fy`` defaults to ``fx``, and ``cx`` / ``cy`` to
    the image centre ``(W - 1) / 2`` / ``(H - 1) / 2`` of the map the camera is used on."""

    def __init__(self, fx: float, baseline: float, fy: Optional[float] = None, cx: Optional[float] = None,
                 cy: Optional[float] = None) -> None:
        self.fx, self.baseline = float(fx), float(baseline)
        self.fy = self.fx if fy is None else float(fy)
        self.cx = None if cx is None else float(cx)
        self.cy = None if cy is None else float(cy)

    def values(self, H: int, W: int) -> tuple:
        """``(num, fx, fy, cx, cy)`` for an ``H`` x ``W`` map; ``num = float32(fx * baseline)``, rounded once."""
        cx = (W - 1) / 2 if self.cx is None else self.cx
        cy = (H - 1) / 2 if self.cy is None else self.cy
        return _num(self.baseline, self.fx), self.fx, self.fy, cx, cy


def _span_bytes(t: torch.Tensor) -> int:
    """Bytes from ``t``'s first element to behind its last."""
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


class _Bound:
    """One plan with one cloud op, and the input tensors its pointers are bound to."""

    def __init__(self, desc: EsmCloudDesc, inputs: dict) -> None:
        self.plan = lib.esm_plan_create()
        self.inputs = {}
        try:
            check(lib.esm_plan_add_cloud(self.plan, ctypes.byref(desc)), "plan_add_cloud")
        except Exception:
            self.close()
            raise
        self.inputs = {k: (t.data_ptr(), _span_bytes(t)) for k, t in inputs.items()}

    def bind(self, inputs: dict) -> None:
        """Move the op's input pointers to ``inputs`` (the same keys) where they changed: ``esm_plan_rebind``."""
        moved = [(self.inputs[k], t) for k, t in inputs.items() if self.inputs[k][0] != t.data_ptr()]
        if moved:
            n = len(moved)
            old = (c_void_p * n)(*[m[0][0] for m in moved])
            size = (ctypes.c_uint64 * n)(*[m[0][1] for m in moved])
            new = (c_void_p * n)(*[m[1].data_ptr() for m in moved])
            check(lib.esm_plan_rebind(self.plan, n, old, size, new), "plan_rebind")
        self.inputs = {k: (t.data_ptr(), _span_bytes(t)) for k, t in inputs.items()}

    def close(self) -> None:
        if self.plan:
            lib.esm_plan_destroy(self.plan)
            self.plan = None

    def __del__(self) -> None:
        self.close()


class CloudBuilder(_DeviceEncoder):
    """The point cloud op for batches of up to ``B`` maps of ``H`` x ``W``, sampled every ``step`` pixels, with
    (``color=True``, 16-byte records) or without (12-byte records) a colour per point: the workspace, one slot of
    ``esm_cloud_max_points`` records per image, the device counts and the pinned mirrors, allocated once.  A plan of
    one op is kept per combination of camera, limits, packing, inputs present and strides of ``disp`` (at most 4); a
    frame whose tensors moved goes through ``esm_plan_rebind``, not a new plan."""

    _module, _codec, _noun, _unit, _least = "esmstereo_amd.cloud", "cloud", "map", "record", 0
    _size = "{} x {} pixels, step {}"

    def __init__(self, B: int, H: int, W: int, step: int = 1, color: bool = True, device="cuda") -> None:
        super().__init__(B, (H, W, step), device)
        self.H, self.W, self.step = self.shape
        self.color = bool(color)
        self.record_bytes = 16 if self.color else 12
        self.max_points = check(lib.esm_cloud_max_points(self.H, self.W, self.step), "cloud_max_points")
        nwork = check(lib.esm_cloud_workspace_bytes(self.B, self.H, self.W, self.step), "cloud_workspace_bytes")
        self._allocate(nwork, self.max_points * self.record_bytes)
        self._plans = {}

    def build(self, disp: torch.Tensor, camera: Camera, color: Optional[torch.Tensor] = None,
              valid: Optional[torch.Tensor] = None, z_min: float = 0.0, z_max: float = math.inf,
              packing: str = "ply", order: str = "bgr") -> List[np.ndarray]:
        """``disp``: float32 ``[B, H, W]``, ``[B, 1, H, W]`` or ``[H, W]`` on the GPU.  A crop is read where it lies;
        only a tensor whose W stride is not 1 is copied first, which costs a temporary and a rebind on every call
        (the one case in which a repeated frame allocates);
        ``color``: uint8 ``[B, H, W, 3]`` / ``[H, W, 3]`` in ``order`` (required by a ``color=True`` builder, refused
        by the other); ``valid``: uint8 or bool ``[B, H, W]`` / ``[H, W]``, non-zero = usable.  Enqueues the op on the
        current stream, synchronises once for the counts, copies ``count * record_bytes`` per image and returns one
        structured array (:func:`point_dtype`) per image, the kept points in raster order."""
        what = "cloud.build"
        self._on_gpu(what, disp)
        if disp.dim() == 4 and disp.shape[1] == 1:
            disp = disp[:, 0]
        elif disp.dim() == 2:
            disp = disp.unsqueeze(0)
        if disp.dim() != 3 or disp.dtype != torch.float32:
            raise ValueError(f"{what}: expected a float32 [B, H, W], [B, 1, H, W] or [H, W] tensor")
        if disp.shape[2] > 1 and disp.stride(2) != 1:
            disp = disp.contiguous()
        n = self._fits(what, disp, (int(disp.shape[1]), int(disp.shape[2]), self.step))
        dtype = point_dtype(self.color, packing)
        if (color is not None) != self.color:
            raise ValueError(f"{what}: this builder was made with color={self.color}")
        inputs = {"disp": disp}
        if color is not None:
            inputs["color"] = self._frames(what, color, order)
            if tuple(inputs["color"].shape) != (n, self.H, self.W, 3) or inputs["color"].device != disp.device:
                raise ValueError(f"{what}: color must be uint8 {(n, self.H, self.W, 3)} on {disp.device}")
        if valid is not None:
            self._on_gpu(what, valid)
            v = valid.unsqueeze(0) if valid.dim() == 2 else valid
            if v.dtype not in (torch.uint8, torch.bool) or tuple(v.shape) != (n, self.H, self.W) or v.device != disp.device:
                raise ValueError(f"{what}: valid must be uint8 or bool {(n, self.H, self.W)} on {disp.device}")
            inputs["valid"] = v.contiguous()
        # everything the descriptor holds beside the pointers: a frame that differs in any of it takes another plan.
        # The strides are part of it (a crop and a contiguous map of one shape are addressed differently); the batch
        # stride of one image and the row stride of one row address nothing, so they do not split plans
        strides = (disp.stride(0) if n > 1 else 0, disp.stride(1) if self.H > 1 else 0)
        key = (n, camera.values(self.H, self.W), float(z_min), float(z_max), packing, order if self.color else None,
               valid is not None, strides)
        with torch.cuda.device(self.device):
            bound = self._plans.get(key)
            if bound is None:
                if len(self._plans) >= 4:
                    self._plans.pop(next(iter(self._plans))).close()
                bound = self._plans[key] = _Bound(self._desc(n, inputs, key), inputs)
            else:
                bound.bind(inputs)
            check(lib.esm_plan_run(bound.plan, _stream(self.work)), what)
            counts = self._lengths(n)
            data = self._copy([c * self.record_bytes for c in counts])
        return [np.frombuffer(d, dtype=dtype) for d in data]

    def _desc(self, n: int, inputs: dict, key) -> EsmCloudDesc:
        _, (num, fx, fy, cx, cy), z_min, z_max, packing, order, _, (sb, sh) = key
        disp = inputs["disp"]
        d = EsmCloudDesc()
        d.disp, d.disp_sb, d.disp_sh = disp.data_ptr(), sb, sh
        d.color = inputs["color"].data_ptr() if "color" in inputs else None
        d.valid = inputs["valid"].data_ptr() if "valid" in inputs else None
        d.out, d.slot_points = self.out.data_ptr(), self.max_points
        d.counts, d.work = self.lengths.data_ptr(), self.work.data_ptr()
        d.B, d.H, d.W, d.step = n, self.H, self.W, self.step
        d.bgr, d.packing = int(order == "bgr"), PACKINGS[packing]
        d.num, d.fx, d.fy, d.cx, d.cy, d.z_min, d.z_max = num, fx, fy, cx, cy, z_min, z_max
        return d


def disparity_to_points(disp: torch.Tensor, camera: Camera, color: Optional[torch.Tensor] = None,
                        valid: Optional[torch.Tensor] = None, step: int = 1, z_min: float = 0.0,
                        z_max: float = math.inf, packing: str = "ply", order: str = "bgr") -> List[np.ndarray]:
    """:meth:`CloudBuilder.build` with the cached builder of this batch, size, step and device (at most 4 are kept,
    so a per-frame loop reuses one set of buffers)."""
    CloudBuilder._on_gpu("disparity_to_points", disp)
    shape = disp.shape if disp.dim() != 2 else (1,) + tuple(disp.shape)
    key = (int(shape[0]), int(shape[-2]), int(shape[-1]), int(step), color is not None, str(disp.device))
    if key not in _builders:
        if len(_builders) >= 4:
            _builders.pop(next(iter(_builders)))
        _builders[key] = CloudBuilder(*key[:5], device=disp.device)
    return _builders[key].build(disp, camera, color, valid, z_min, z_max, packing, order)


_builders = {}


def ply_bytes(points: np.ndarray) -> bytes:
    """A ``binary_little_endian 1.0`` PLY file of one image's points: the header, then the records verbatim (which is
    why the ``"ply"`` packing is R, G, B, A).  ``points``: an array of :func:`point_dtype` ``(False)`` or
    ``(True, "ply")``."""
    points = np.ascontiguousarray(points)
    if points.dtype not in (_DTYPES[None], _DTYPES["ply"]) or points.ndim != 1:
        raise ValueError("ply_bytes: expected a 1-D array of the xyz or the 'ply' record dtype")
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {len(points)}"]
    lines += [f"property float {n}" for n in "xyz"]
    if points.dtype == _DTYPES["ply"]:
        lines += [f"property uchar {n}" for n in ("red", "green", "blue", "alpha")]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii") + points.tobytes()


def write_ply(path, points: np.ndarray) -> None:
    """:func:`ply_bytes` of ``points`` into the file ``path``."""
    with open(path, "wb") as f:
        f.write(ply_bytes(points))
