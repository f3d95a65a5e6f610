"""HIP-runtime analogue of the reference's ROS2 stereo node loop
(``kitti_publisher/src/kitti_publisher_cuda_node.cpp:323-430``, ``preprocess_image`` ``:136-175``).

The reference node, per timer tick: reads a stereo pair (OpenCV, BGR), pads it right / bottom to
``(w // 32 + 1) * 32`` x ``(h // 32 + 1) * 32`` and normalises it on the CPU, copies it to the
device, runs the TensorRT engine of ``ESMStereo_trt`` (``enqueueV3``), copies the disparity back,
crops it, median-blurs it (5x5), masks it to ``(0, max_disp)``, converts it to 16-bit (x256) and
publishes it.  :class:`StereoNode` does the same work with the device doing all of it:

* the uint8 frames go host -> device as bytes (a quarter of the reference's fp32 copy) from pinned
  staging buffers on the node's own stream;
* pad + normalise: ``esm_preprocess_u8`` (pad right / bottom with normalised zeros, as
  ``copyMakeBorder`` before ``convertTo`` / normalise);
* inference: ``ESMStereo_trt.forward`` (backbone on PyTorch/MIOpen, hot path as one hipGraph);
* crop + medianBlur(5) + valid mask + ``convertTo(CV_16UC1, 256)``: ``esm_node_filter_u16``;
* only the uint16 disparity comes back to the host;
* the node's picture (``visualize_and_record_disparity``, ``:81-86,117-118``: ``minMaxLoc`` over the valid mask,
  ``convertTo(CV_8UC1, ...)``, ``COLORMAP_MAGMA``, ``vconcat`` under the left image):
  :meth:`StereoNode.process_rendered` builds it on the device from the masked median map
  (``esm_disp_colorize_u8``, RANGE mode, the range found on the device) and returns it as 8-bit
  bytes beside the disparity.

``elapsed_ms`` is measured as the node measures it (``:357-376``): from the input copy to the end
of inference.  The first frame also builds the hot path's launch plan and hipGraph, so
:meth:`StereoNode.warmup` runs one frame untimed (:meth:`run` calls it first).  Publishing (ROS
topics), what the node draws on the picture (the centre circle and the ``putText`` overlays,
``:100-115``), ``imshow`` and the video writer are outside this package; :meth:`StereoNode.run`
yields the per-frame results to whatever publishes them.

The reference ships three more nodes, and their per-frame device work is here too (what they draw on the frame stays
outside, as above):

* ``kitti_publisher_conf`` (``kitti_publisher_conf/src/kitti_publisher_conf_cuda_node.cpp:484-605``) runs
  ``ESMStereo_confidence``, adds ``conf >= threshold`` to the valid mask (``:571-575``), scores the result against the
  KITTI 16-bit ground truth (``computeEPE``, ``:55-67``) and shows a four-panel frame (``:183-257``): left image and
  colour-mapped disparity beside the node's own error map (``:69-151``) and the confidence map.
  :class:`ConfidenceNode` does that with ``esm_node_filter_conf_u16`` (the median selected from an LDS tile),
  ``esm_node_panels_u8`` (range pass + one pass over the pixels) and ``esm_disp_metrics_f32``; the uint16 map, the
  frame and one 12-double record come back.
* ``virtual_kitti_publisher`` (``virtual_kitti_publisher/src/virtual_kitti_publisher_cuda_node.cpp:413-523,131-213``)
  does not pad: it resizes every camera frame to the one size its engine was built for (``cv::resize(...,
  INTER_LINEAR)``, then /255, mean and std, ``:232-266``) and publishes, draws and scores at that size.
  :class:`ResizeNode` does that: ``esm_preprocess_resize_u8`` (resize and network input in one launch, the resized
  left image for the picture from the same launch), the model, ``esm_node_filter_u16`` over the whole map, the
  picture stacked and squeezed back to one network-sized frame with ``esm_resize_u8`` (``:211-213``), the ground
  truth from the 16-bit depth image (:func:`depth16_to_disparity`, ``esm_depth16_to_disp_f32``, ``:55-77,146-147``)
  and ``computeEPE`` / ``computeD1`` (``:80-126``) from one ``esm_disp_metrics_f32`` call; its running mean of the
  per-frame EPE is :attr:`ResizeNode.epe_mean`.  One tuned, captured shape then serves every camera.
* ``kitti_publisher_ess`` (``kitti_publisher_ess/src/kitti_publisher_ess_cuda_node.cpp:241-275``) is the same loop
  around another engine with mean 0 and std 1: ``ResizeNode(model, ..., mean=(0, 0, 0), std=(1, 1, 1))``.

Parity: the post-filter is bit-exact against ``oracle/io_oracle.py``, whose median restatement
matches ``scipy.ndimage.median_filter(mode="nearest")``.  Parity with OpenCV itself is UNPINNED: cv2
is not importable here and the reference holds no node outputs.  That ``cv::medianBlur`` on the
cropped ROI replicates the ROI's own border (rather than reading the padded image around it) is an
assumption of this restatement.  The picture's arithmetic restates ``convertTo``'s documented
rounding (:mod:`esmstereo_amd.render`); its parity with OpenCV is UNPINNED for the same reason, and
the default table is matplotlib's magma, not cv2's bytes.  The same holds for ``cv::resize(..., INTER_LINEAR)`` in
:func:`depth16_to_disparity`: the header restates OpenCV's float rule (coordinate in fp64, rounded to fp32, two
separately rounded lerps), tests/node_ref.py checks the restatement against ``torch.nn.functional.interpolate`` and an
fp64 evaluation, and parity with OpenCV's own bytes is UNPINNED.
"""
from __future__ import annotations

import ctypes
import time
from typing import Iterable, Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import METRICS_RECORD_DOUBLES, METRICS_VALUES, check, lib, _stream
from .cloud import CloudBuilder
from .io import IMAGENET_MEAN, IMAGENET_STD
from .render import colorize_range, colormap_lut, range_workspace_bytes

__all__ = ["StereoNode", "ConfidenceNode", "ResizeNode", "depth16_to_disparity", "node_pads"]

EPE_MAX_DISP = 192.0  # computeEPE's bound (:59), hard-coded there and independent of max_disp
D1_THRES = (ctypes.c_float * 1)(3.0)  # computeD1's absolute bound (virtual_kitti_publisher_cuda_node.cpp:120)


def node_pads(h: int, w: int, m: int = 32) -> Tuple[int, int]:
    """(pad_bottom, pad_right) of ``preprocess_image`` (:141-146): always up to the NEXT multiple
    of 32, so an already divisible size still gains 32 rows / columns."""
    return (h // m + 1) * m - h, (w // m + 1) * m - w


class StereoNode:
    """The node's per-frame work on one device stream (see the module docstring).

    ``model``: an ``ESMStereo_trt`` (or any module whose ``forward(left, right)`` returns
    ``[B, H, W]`` disparities); ``height`` x ``width``: the camera frame size.  ``lut``: the colour
    table of :meth:`process_rendered`, a uint8 ``[256, 3]`` tensor in the frames' channel order or
    the name of a shipped table (``"magma"``, ``"jet"``; BGR); when given, the frame's device and
    pinned staging buffers are allocated here.

    :meth:`_frame` is the one frame loop of the three nodes; a subclass overrides its steps (:meth:`_preprocess`,
    :meth:`_filter`, :meth:`_picture`, ``_score``), never their sequence."""

    outputs = 1  # the maps the model returns

    def __init__(self, model: torch.nn.Module, height: int, width: int, max_disp: float = 192.0,
                 device: torch.device = torch.device("cuda"), lut=None) -> None:
        pb, pr = node_pads(int(height), int(width))
        self.hp, self.wp = int(height) + pb, int(width) + pr
        self._allocate(model, height, width, (self.hp, self.wp), (int(height), int(width)), max_disp, device, lut)

    def _allocate(self, model, height, width, net: Tuple[int, int], window: Tuple[int, int], max_disp, device,
                  lut) -> None:
        """The stream and the buffers every frame uses: ``height`` x ``width`` camera frames in, the network's input
        (and its map) at ``net``, the disparity that comes back at ``window``, the part of that map the filter keeps."""
        self.model = model
        self.device = torch.device(device)
        self.h, self.w = int(height), int(width)
        self.net, self.window = net, window
        self.max_disp = float(max_disp)
        self.stream = torch.cuda.Stream(self.device)
        self.host_u8 = torch.empty(2, self.h, self.w, 3, dtype=torch.uint8).pin_memory()
        self.host_u16 = torch.empty(*window, dtype=torch.int16).pin_memory()
        self.dev_u8 = torch.empty(2, self.h, self.w, 3, dtype=torch.uint8, device=self.device)
        self.net_in = torch.empty(2, 1, 3, *net, device=self.device)
        self.dev_u16 = torch.empty(*window, dtype=torch.int16, device=self.device)
        self.filtered = torch.empty(*window, device=self.device)
        self.lut = None
        if lut is not None:
            self._render_buffers(lut)

    def _render_buffers(self, lut) -> None:
        """The colour table (a uint8 ``[256, 3]`` device tensor or a shipped table's name, BGR), the range workspace
        and the picture's buffers."""
        self.lut = colormap_lut(lut, self.device) if isinstance(lut, str) else lut.to(self.device)
        self.range_work = torch.empty(range_workspace_bytes(1, *self.window), dtype=torch.uint8, device=self.device)
        self._picture_buffers()

    def _picture_buffers(self) -> None:
        """The frame's device and pinned staging buffers."""
        self.dev_frame = torch.empty(2 * self.h, self.w, 3, dtype=torch.uint8, device=self.device)
        self.host_frame = torch.empty(2 * self.h, self.w, 3, dtype=torch.uint8).pin_memory()

    def process(self, left: np.ndarray, right: np.ndarray) -> Tuple[np.ndarray, float]:
        """One frame pair ``[H, W, 3] uint8`` (channel order as read: the reference feeds OpenCV's
        BGR) -> (disparity ``[H, W] uint16``, elapsed ms of copy-in + inference)."""
        return self._frame(left, right, False)

    def process_rendered(self, left: np.ndarray, right: np.ndarray) -> Tuple[np.ndarray, np.ndarray, float]:
        """:meth:`process` plus the node's picture (``:81-86,117-118``): -> (disparity ``[H, W] uint16``, frame
        ``[2H, W, 3] uint8``, elapsed ms).  The frame is the left image over the colour-mapped disparity
        (``cv::vconcat``): ``self.filtered`` through :func:`esmstereo_amd.render.colorize_range` (each frame's own
        min / max over the valid pixels -> indices 255 / 0) and the node's table, stacked under ``self.dev_u8[0]``
        on the node's stream; 6 bytes a pixel come back through a pinned buffer.  Without ``lut`` in the
        constructor the first call takes the shipped MAGMA table and allocates the buffers."""
        if self.lut is None:
            self._render_buffers("magma")
        u16, ms = self._frame(left, right, True)
        return u16, self.host_frame.numpy().copy(), ms

    def process_points(self, left: np.ndarray, right: np.ndarray, camera, step: int = 1, z_min: float = 0.0,
                       z_max: float = float("inf"), packing: str = "ply",
                       order: str = "bgr") -> Tuple[np.ndarray, np.ndarray, float]:
        """:meth:`process` plus the frame's point cloud: -> (disparity ``[H, W] uint16``, points, elapsed ms).
        ``camera``: an :class:`esmstereo_amd.cloud.Camera`.  After the frame, ``self.filtered`` (invalid pixels are
        exactly 0 there, whatever gate the node applies, so the op's ``d > 0`` rule drops them) is reprojected and
        coloured from the left image ``self.dev_u8[0]`` (channels in ``order``, as the frames were given) by one
        :class:`esmstereo_amd.cloud.CloudBuilder` kept by the node, on the node's stream; only the kept points come
        back, as one structured array (:func:`esmstereo_amd.cloud.point_dtype`) in raster order.  The builder is made
        at the first call and again whenever ``step`` differs from the last call's (fresh device and pinned buffers:
        alternating steps reallocates every frame; keep one step per node)."""
        u16, ms = self._frame(left, right, False)
        if getattr(self, "_cloud", None) is None or self._cloud.step != int(step):
            self._cloud = CloudBuilder(1, self.h, self.w, int(step), True, self.device)
        with torch.cuda.stream(self.stream):
            points = self._cloud.build(self.filtered, camera, self.dev_u8[0], None, z_min, z_max, packing, order)[0]
        return u16, points, ms

    def _frame(self, left: np.ndarray, right: np.ndarray, rendered: bool, score: Optional[tuple] = None,
               **gate) -> Tuple[np.ndarray, float]:
        """One frame on the node's stream.  ``score``: the 16-bit ground truth image and whatever else ``_score``
        takes (the scoring nodes); ``gate``: what :meth:`_filter` takes beside the maps."""
        if left.shape != (self.h, self.w, 3) or right.shape != (self.h, self.w, 3):
            raise ValueError(f"{type(self).__name__}: frames must be {(self.h, self.w, 3)} uint8")
        self.host_u8[0].numpy()[...] = left
        self.host_u8[1].numpy()[...] = right
        if score is not None:
            self.host_gt.numpy().view(np.uint16)[...] = score[0]
        s = self.stream
        sp = _stream(s)
        with torch.cuda.stream(s):
            t0 = time.perf_counter()
            self.dev_u8.copy_(self.host_u8, non_blocking=True)
            for k in range(2):
                self._preprocess(k, rendered, sp)
            with torch.no_grad():
                out = self.model(self.net_in[0], self.net_in[1])
            s.synchronize()
            elapsed_ms = (time.perf_counter() - t0) * 1e3
            maps = [m.contiguous() for m in (out if self.outputs > 1 else (out,))]
            want = (1,) + self.net  # checked before any pointer goes to the filter
            if [tuple(m.shape) for m in maps] != [want] * self.outputs:
                what = f"two {want} maps" if self.outputs == 2 else f"a {want} map"
                raise ValueError(f"{type(self).__name__}: the model must return {what}, got "
                                 + " and ".join(str(tuple(m.shape)) for m in maps))
            self._filter(maps, sp, **gate)
            self.host_u16.copy_(self.dev_u16, non_blocking=True)
            if rendered:
                self._picture(sp)
                self.host_frame.copy_(self.dev_frame, non_blocking=True)
            if score is not None:
                self.dev_gt.copy_(self.host_gt, non_blocking=True)
                self._score(maps, sp, *score[1:])
                self.host_records.copy_(self.records, non_blocking=True)
            s.synchronize()
        return self.host_u16.numpy().view(np.uint16).copy(), elapsed_ms

    def _preprocess(self, k: int, rendered: bool, sp) -> None:
        """Image ``k`` of the pair -> its network input: pad right / bottom and normalise."""
        check(lib.esm_preprocess_u8(self.dev_u8[k].data_ptr(), self.net_in[k].data_ptr(), 1, self.h, self.w,
                                    *self.net, 0, 0, 1, sp), "node preprocess")

    def _filter(self, maps, sp) -> None:
        """The model's map -> ``dev_u16`` and ``filtered`` over the window."""
        check(lib.esm_node_filter_u16(maps[0].data_ptr(), self.dev_u16.data_ptr(), self.filtered.data_ptr(), 1,
                                      *self.net, 0, 0, *self.window, self.max_disp, sp), "node filter")

    def _picture(self, sp) -> None:
        """``filtered`` -> ``dev_frame``: the colour-mapped map stacked under the left image."""
        colorize_range(self.filtered, self.lut, stack=self.dev_u8[0], out=self.dev_frame, workspace=self.range_work)

    def warmup(self, left: np.ndarray, right: np.ndarray) -> None:
        """One untimed frame: builds the plan / hipGraph so later frames' elapsed_ms is steady state."""
        self.process(left, right)
        self._warm = True

    def run(self, pairs: Iterable[Tuple[np.ndarray, np.ndarray]]) -> Iterator[Tuple[np.ndarray, float]]:
        """The timer loop's body over a frame source (the node cycles its image list, :325-327); the
        first pair is also run once untimed (warmup) before its timed frame."""
        for left, right in pairs:
            if not getattr(self, "_warm", False):
                self.warmup(left, right)
            yield self.process(left, right)


class _Scored:
    """The score state of the two nodes that have a ground truth: the staged 16-bit image, the fp32 ground truth at
    the window, the buffers of ``esm_disp_metrics_f32``, and the running mean of the per-frame EPE
    (``total_epe / frame_count``, ``virtual_kitti_publisher_cuda_node.cpp:149-153``) over the frames
    ``process_scored`` has seen."""

    total_epe, frame_count, records = 0.0, 0, None

    @property
    def epe_mean(self) -> float:
        return self.total_epe / self.frame_count if self.frame_count else 0.0

    def _score_buffers(self) -> None:
        """Allocated once: what ``process_scored`` touches per frame beside the picture's buffers."""
        dev = self.device
        self.host_gt = torch.empty(self.h, self.w, dtype=torch.int16).pin_memory()
        self.dev_gt = torch.empty(self.h, self.w, dtype=torch.int16, device=dev)
        self.gt_f32 = torch.empty(*self.window, device=dev)
        nbytes = check(lib.esm_disp_metrics_workspace(1, *self.window), "disp_metrics_workspace")
        self.metrics_work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.records = torch.empty(1, METRICS_RECORD_DOUBLES, dtype=torch.float64, device=dev)
        self.values = torch.empty(1, METRICS_VALUES, device=dev)
        self.batch_values = torch.empty(METRICS_VALUES, device=dev)
        self.host_records = torch.empty(1, METRICS_RECORD_DOUBLES, dtype=torch.float64).pin_memory()

    def _metrics(self, sp, thres=None) -> None:
        """``filtered`` against ``gt_f32`` over ``(gt > 0) & (gt < 192)`` -> ``records`` (``thres``: D1's bound)."""
        H, W = self.window
        check(lib.esm_disp_metrics_f32(self.filtered.data_ptr(), H * W, W, self.gt_f32.data_ptr(), H * W, W, None, 0, 0,
                                       1, H, W, 0.0, EPE_MAX_DISP, 1, thres, int(thres is not None), 0.05,
                                       self.metrics_work.data_ptr(), self.records.data_ptr(), self.values.data_ptr(),
                                       self.batch_values.data_ptr(), sp), "node score")

    def _scored(self):
        """The record read back -> (record, epe); the EPE enters :attr:`epe_mean`."""
        rec = self.host_records.numpy()[0]
        epe = float(rec[2] / rec[0]) if rec[0] > 0 else 0.0
        self.total_epe += epe
        self.frame_count += 1
        return rec, epe


class ConfidenceNode(_Scored, StereoNode):
    """The confidence-gated node (``kitti_publisher_conf_cuda_node.cpp:484-605``) on one device stream.

    ``model``: an ``ESMStereo_confidence`` (or any module whose ``forward(left, right)`` returns ``(disp, conf)``,
    both ``[B, H, W]``).  Other arguments as :class:`StereoNode`; ``lut`` defaults to the shipped MAGMA table when
    :meth:`process_scored` is first called.  ``epe_mean`` is the node's running mean over the frames
    :meth:`process_scored` has seen (:class:`_Scored`)."""

    outputs = 2
    dev_panels = None

    def __init__(self, model: torch.nn.Module, height: int, width: int, max_disp: float = 192.0,
                 device: torch.device = torch.device("cuda"), lut=None) -> None:
        super().__init__(model, height, width, max_disp, device, lut)
        if lut is not None:
            self._panel_buffers()

    def _panel_buffers(self) -> None:
        """Allocated once: everything :meth:`process_scored` touches per frame (the colour table and the range
        workspace are :meth:`StereoNode._render_buffers`')."""
        if self.lut is None:
            self._render_buffers("magma")
        self._score_buffers()
        self.dev_panels = torch.empty(2 * self.h, 2 * self.w, 3, dtype=torch.uint8, device=self.device)
        self.host_panels = torch.empty(2 * self.h, 2 * self.w, 3, dtype=torch.uint8).pin_memory()

    def process(self, left: np.ndarray, right: np.ndarray, threshold: float = 0.5) -> Tuple[np.ndarray, float]:
        """One frame pair -> (disparity ``[H, W] uint16``, elapsed ms): :meth:`StereoNode.process` with
        ``conf >= threshold`` in the valid mask (``:571-575``), the comparison in fp64 as the node's is."""
        return self._frame(left, right, False, threshold=float(threshold))

    def process_scored(self, left: np.ndarray, right: np.ndarray, gt_u16: np.ndarray,
                       threshold: float = 0.5) -> Tuple[np.ndarray, np.ndarray, float, float]:
        """:meth:`process` plus the node's frame and score against the KITTI 16-bit ground truth ``gt_u16``
        ``[H, W] uint16`` (disparity x 256, 0 = none): -> (disparity ``[H, W] uint16``, frame ``[2H, 2W, 3] uint8``,
        epe, elapsed ms).  The frame (``:183-257`` without the overlays) is left image | error map over colour-mapped
        disparity | confidence; ``epe`` is ``computeEPE`` (``:55-67``): the fp64 mean of ``|gt - disp|`` over
        ``(gt > 0) & (gt < 192)`` with gt zeroed where the disparity is invalid, 0 over no pixel (``cv::mean``).  It
        also enters :attr:`epe_mean`."""
        gt_u16 = np.asarray(gt_u16)
        if gt_u16.shape != (self.h, self.w) or gt_u16.dtype != np.uint16:
            raise ValueError(f"ConfidenceNode: gt_u16 must be {(self.h, self.w)} uint16")
        if self.dev_panels is None:
            self._panel_buffers()
        u16, ms = self._frame(left, right, False, (gt_u16,), threshold=float(threshold))
        _, epe = self._scored()
        return u16, self.host_panels.numpy().copy(), epe, ms

    def _filter(self, maps, sp, threshold: float = 0.5) -> None:
        """:meth:`StereoNode._filter` with ``conf >= threshold`` in the valid mask."""
        check(lib.esm_node_filter_conf_u16(maps[0].data_ptr(), maps[1].data_ptr(), self.dev_u16.data_ptr(),
                                           self.filtered.data_ptr(), None, 1, self.hp, self.wp, 0, 0, self.h, self.w,
                                           self.max_disp, threshold, sp), "node filter (confidence)")

    def _score(self, maps, sp) -> None:
        """The four panels and the record of the frame against ``dev_gt``."""
        check(lib.esm_node_panels_u8(self.filtered.data_ptr(), maps[1].data_ptr(), self.hp, self.wp, 0, 0,
                                     self.dev_gt.data_ptr(), self.dev_u8[0].data_ptr(), self.lut.data_ptr(),
                                     self.dev_panels.data_ptr(), self.gt_f32.data_ptr(), self.range_work.data_ptr(), 1,
                                     self.h, self.w, sp), "node panels")
        self._metrics(sp)
        self.host_panels.copy_(self.dev_panels, non_blocking=True)


class ResizeNode(_Scored, StereoNode):
    """The resizing nodes (``virtual_kitti_publisher_cuda_node.cpp:413-523,131-213``; ``kitti_publisher_ess`` with
    ``mean = (0, 0, 0)``, ``std = (1, 1, 1)``) on one device stream: every ``height`` x ``width`` camera frame is
    resized to the one ``net_height`` x ``net_width`` the model runs at (multiples of 32: the model's rule, enforced
    there), so one launch plan and one captured graph serve any camera.  The disparity, the picture and the score are
    all at the network size, as the nodes publish them.  ``mean`` / ``std`` apply to the channels as stored (the
    nodes feed OpenCV's BGR and never swap it).  Other arguments and conventions as :class:`StereoNode`; ``lut``
    defaults to the shipped MAGMA table when a picture is first asked for.  :attr:`epe_mean` is the node's running
    ``total_epe / frame_count`` (``:149-153``) over :meth:`process_scored`'s frames."""

    def __init__(self, model: torch.nn.Module, height: int, width: int, net_height: int, net_width: int,
                 max_disp: float = 192.0, mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD,
                 device: torch.device = torch.device("cuda"), lut=None) -> None:
        self.hn, self.wn = int(net_height), int(net_width)
        if min(int(height), int(width), self.hn, self.wn) <= 0:
            raise ValueError("ResizeNode: sizes must be positive")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("ResizeNode: mean and std take three values each")
        self.mean = (ctypes.c_float * 3)(*[float(v) for v in mean])
        self.std = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._allocate(model, height, width, (self.hn, self.wn), (self.hn, self.wn), max_disp, device, lut)

    def _picture_buffers(self) -> None:
        """The resized left image, the stacked picture and the squeezed frame with its pinned staging buffer."""
        dev, hn, wn = self.device, self.hn, self.wn
        self.dev_left = torch.empty(hn, wn, 3, dtype=torch.uint8, device=dev)
        self.dev_stack = torch.empty(2 * hn, wn, 3, dtype=torch.uint8, device=dev)
        self.dev_frame = torch.empty(hn, wn, 3, dtype=torch.uint8, device=dev)
        self.host_frame = torch.empty(hn, wn, 3, dtype=torch.uint8).pin_memory()

    def process(self, left: np.ndarray, right: np.ndarray) -> Tuple[np.ndarray, float]:
        """One camera-sized pair ``[h, w, 3] uint8`` -> (disparity ``[Hn, Wn] uint16`` at the network size, elapsed
        ms of copy-in + resize + inference): ``esm_preprocess_resize_u8`` twice, the model, ``esm_node_filter_u16``
        over the whole map (the node's pads are 0, so it crops nothing)."""
        return self._frame(left, right, False)

    def process_points(self, left: np.ndarray, right: np.ndarray, camera, **limits):
        """Not available: this node's map is at the network size, so the intrinsics have to be scaled and the colour
        taken from the resized frame, which is a decision this class does not make."""
        raise NotImplementedError("ResizeNode.process_points: points at the network size need scaled intrinsics and "
                                  "the resized frame as the colour source; not provided")

    def process_scored(self, left: np.ndarray, right: np.ndarray, depth_u16: np.ndarray, focal: float,
                       baseline: float) -> Tuple[np.ndarray, np.ndarray, float, float, float]:
        """:meth:`process_rendered` plus the node's score against the camera-sized 16-bit depth image ``depth_u16``
        ``[h, w] uint16``: -> (disparity, frame, epe, d1, elapsed ms).  The ground truth is
        :func:`depth16_to_disparity` at the network size (``:55-77,146-147``, written into the node's own buffer);
        ``epe`` is ``computeEPE`` (``:80-92``), the fp64 mean of ``|filtered - gt|`` over ``(gt > 0) & (gt < 192)``,
        0 over no pixel, and ``d1`` ``computeD1`` (``:95-126``), the percent of those pixels with ``err > 3 &&
        err / gt > 0.05``.  ``filtered`` is the masked median map with its zeros: unlike the confidence node, this
        one does not zero the ground truth where the disparity is invalid.  Both come from one
        ``esm_disp_metrics_f32`` call and one record read back; ``epe`` also enters :attr:`epe_mean`."""
        depth_u16 = np.asarray(depth_u16)
        if depth_u16.shape != (self.h, self.w) or depth_u16.dtype != np.uint16:
            raise ValueError(f"ResizeNode: depth_u16 must be {(self.h, self.w)} uint16")
        if self.lut is None:
            self._render_buffers("magma")
        if self.records is None:
            self._score_buffers()
        num = float(np.float32(focal) * np.float32(baseline))  # as depth16_to_disparity
        u16, ms = self._frame(left, right, True, (depth_u16, num))
        rec, epe = self._scored()
        d1 = float(100.0 * rec[8] / rec[0]) if rec[0] > 0 else 0.0
        return u16, self.host_frame.numpy().copy(), epe, d1, ms

    def _preprocess(self, k: int, rendered: bool, sp) -> None:
        """Image ``k`` of the pair -> its network input, resized; the left image's launch also leaves the picture's
        top panel."""
        resized = self.dev_left.data_ptr() if rendered and k == 0 else None
        check(lib.esm_preprocess_resize_u8(self.dev_u8[k].data_ptr(), self.net_in[k].data_ptr(), resized, 1, self.h,
                                           self.w, self.hn, self.wn, self.mean, self.std, sp),
              "node resize + preprocess")

    def _picture(self, sp) -> None:
        """:meth:`process_rendered`'s picture here (``:131-213`` without the overlays), ``[Hn, Wn, 3]``: the left image
        at the network size (``:186-188``, the ``resized`` output of its preprocess launch) stacked over the auto-range
        colour-mapped disparity, and the ``[2Hn, Wn, 3]`` stack squeezed back to one network-sized frame with
        ``esm_resize_u8`` (``:211-213``); 3 bytes a pixel come back."""
        hn, wn = self.hn, self.wn
        colorize_range(self.filtered, self.lut, stack=self.dev_left, out=self.dev_stack, workspace=self.range_work)
        check(lib.esm_resize_u8(self.dev_stack.data_ptr(), self.dev_frame.data_ptr(), 1, 2 * hn, wn, hn, wn, 3, sp),
              "node squeeze")

    def _score(self, maps, sp, num: float) -> None:
        """The ground truth from the depth image in ``dev_gt`` and the record of the frame against it."""
        check(lib.esm_depth16_to_disp_f32(self.dev_gt.data_ptr(), self.gt_f32.data_ptr(), 1, self.h, self.w, self.hn,
                                          self.wn, num, 0.01, sp), "node ground truth")
        self._metrics(sp, D1_THRES)


def depth16_to_disparity(depth: torch.Tensor, focal: float, baseline: float, size: Optional[Tuple[int, int]] = None,
                         depth_scale: float = 0.01) -> torch.Tensor:
    """``depthToDisparity`` + ``cv::resize(..., INTER_LINEAR)`` (``virtual_kitti_publisher_cuda_node.cpp:55-77,
    146-147``) in one launch: a 16-bit depth image (``torch.uint16`` or the same bits as ``torch.int16``, ``[H, W]``
    or ``[B, H, W]``, on the GPU) -> the fp32 disparity ``focal * baseline / (d16 * depth_scale)`` (0 where the depth
    is 0), resized to ``size = (height, width)`` (the source size when ``None``).  ``focal`` and ``baseline`` are
    taken as floats and multiplied in fp32, as the reference does.  With the source size the result is the
    conversion itself, bit for bit.  Parity with OpenCV's own resize is UNPINNED (module docstring)."""
    if (not isinstance(depth, torch.Tensor) or depth.dtype not in (torch.uint16, torch.int16)
            or depth.dim() not in (2, 3)):
        raise ValueError("depth16_to_disparity: expected a uint16 / int16 [H, W] or [B, H, W] tensor")
    if not depth.is_cuda:
        raise RuntimeError("esmstereo_amd.node: depth16_to_disparity: depth must be on the GPU (no CPU fallback)")
    d = (depth.unsqueeze(0) if depth.dim() == 2 else depth).contiguous()
    B, Hs, Ws = (int(v) for v in d.shape)
    H, W = (Hs, Ws) if size is None else (int(size[0]), int(size[1]))
    num = float(np.float32(focal) * np.float32(baseline))
    out = torch.empty(B, H, W, device=d.device, dtype=torch.float32)
    with torch.cuda.device(d.device):
        check(lib.esm_depth16_to_disp_f32(d.data_ptr(), out.data_ptr(), B, Hs, Ws, H, W, num, float(depth_scale),
                                          _stream(d)), "depth16_to_disparity")
    return out[0] if depth.dim() == 2 else out
