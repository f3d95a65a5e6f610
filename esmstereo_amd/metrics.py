"""Scoring a disparity against ground truth on the device: drop-ins for ``utils/metrics.py`` and
``utils/visualization.py:vis``.

    from esmstereo_amd.metrics import D1_metric, EPE_metric, Thres_metric   # instead of `from utils.metrics import ...`
    from esmstereo_amd.metrics import vis                                    # instead of `from utils.visualization import vis`

The reference scores one image and one metric at a time: two boolean-index compactions (``D_est[mask]``,
``D_gt[mask]``) with a host sync each, and two more syncs for the skip rule (utils/metrics.py:17-74).  Here one
pass over ``est``, ``gt`` and ``mask`` (``csrc/metrics.hip``, two launches, no sync) gives every number that
train_kitti.py:221-232, train_sceneflow.py:239-250, test_kitti.py:117-125, test_eth3d.py:93-98 and
test_mid.py:106-114 print:

* the named functions keep the reference's signatures and return a 0-dim fp32 tensor on the inputs' device;
* :func:`disparity_metrics` returns everything at once, per image and for the batch;
* :class:`DisparityEvaluator` collects a dataset loop's records on the device and reads them back once;
* :func:`vis` / :func:`error_image` is the KITTI error map, bit-exact with the numpy original.

Rates are ``float(count) / float(n_mask)`` of exact integer counts, the bits of torch's fp32 mean of a 0/1 tensor
(below 2^24 pixels); EPE is an fp64 sum divided by the count and rounded once to fp32 (the reference's fp32 sum has
no specified order).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import METRICS_MAX_THRES, METRICS_RECORD_DOUBLES, METRICS_VALUES, check, lib, _stream

D1_REL = 0.05  # utils/metrics.py:47,56


class DisparityMetrics:
    """What one pass gives.  Per-image tensors are ``[B]`` (``thres`` / ``d1``: ``[B, K]``), batch tensors 0-dim
    (``[K]``): the mean over the images the reference keeps, 0 when it keeps none (utils/metrics.py:31-37).  All
    are views of the three buffers the kernels wrote; ``n_valid`` and ``skipped`` are formed when asked for (one
    small launch each), so a caller who wants the means pays for nothing else."""
    FIELDS = ("epe", "thres", "d1", "n_valid", "skipped", "batch_epe", "batch_thres", "batch_d1", "records")
    __slots__ = ("records", "values", "batch", "_k")

    def __init__(self, records: torch.Tensor, values: torch.Tensor, batch: torch.Tensor, k: int):
        self.records = records  # [B, 12] fp64: n_mask, n_gt_pos, sum |gt - est|, 0, n_abs[4], n_both[4]
        self.values = values    # [B, 10] fp32: epe, thres[4], d1[4], skipped (0 / 1)
        self.batch = batch      # [10] fp32: the nine means, then the number of images kept
        self._k = k

    epe = property(lambda s: s.values[:, 0])
    thres = property(lambda s: s.values[:, 1:1 + s._k])
    d1 = property(lambda s: s.values[:, 1 + METRICS_MAX_THRES:1 + METRICS_MAX_THRES + s._k])
    n_valid = property(lambda s: s.records[:, 0].long())                   # pixels in the mask
    skipped = property(lambda s: s.values[:, METRICS_VALUES - 1] != 0)     # mean(mask) / mean(gt > 0) < 0.1
    batch_epe = property(lambda s: s.batch[0])
    batch_thres = property(lambda s: s.batch[1:1 + s._k])
    batch_d1 = property(lambda s: s.batch[1 + METRICS_MAX_THRES:1 + METRICS_MAX_THRES + s._k])


def _check_shape(*ts) -> None:
    """The reference's precondition (utils/metrics.py:10-14), an assertion there too: [B, H, W], all alike."""
    assert all(t.dim() == 3 and t.shape == ts[0].shape for t in ts), [tuple(t.shape) for t in ts]


def _view(t: torch.Tensor, dtype, what: str):
    """(tensor kept alive, pointer, batch stride, row stride): the tensor where it lies when W is contiguous."""
    if not t.is_cuda:
        raise RuntimeError(f"esmstereo_amd.metrics: {what} must be on the GPU (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"esmstereo_amd.metrics: {what} must be {dtype}, got {t.dtype}")
    if t.shape[2] > 1 and t.stride(2) != 1:
        t = t.contiguous()
    return t, t.data_ptr(), t.stride(0), t.stride(1)


def _launch(est, gt, mask, maxdisp, thres: Sequence[float], records, values, batch) -> None:
    B, H, W = (int(v) for v in gt.shape)
    est, pe, eb, eh = _view(est, torch.float32, "D_est")
    gt, pg, gb, gh = _view(gt, torch.float32, "D_gt")
    if est.device != gt.device or (mask is not None and mask.device != gt.device):
        raise RuntimeError("esmstereo_amd.metrics: inputs on different devices")
    pm, mb, mh = None, 0, 0
    if mask is not None:
        mask, pm, mb, mh = _view(mask, torch.bool, "mask")
    if len(thres) > METRICS_MAX_THRES:
        raise ValueError(f"at most {METRICS_MAX_THRES} thresholds per call, got {len(thres)}")
    nbytes = check(lib.esm_disp_metrics_workspace(B, H, W), "disp_metrics_workspace")
    work = torch.empty(nbytes, device=gt.device, dtype=torch.uint8)
    th = (ctypes.c_float * max(len(thres), 1))(*[float(t) for t in thres])
    with torch.cuda.device(gt.device):
        check(lib.esm_disp_metrics_f32(pe, eb, eh, pg, gb, gh, pm, mb, mh, B, H, W, 0.0,
                                       float(maxdisp) if maxdisp is not None else 0.0, int(maxdisp is not None),
                                       th, len(thres), D1_REL, work.data_ptr(), records.data_ptr(), values.data_ptr(),
                                       batch.data_ptr(), _stream(gt)), "disp_metrics")


def disparity_metrics(D_est: torch.Tensor, D_gt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                      maxdisp: Optional[float] = None, thres: Sequence[float] = (1., 2., 3.)) -> DisparityMetrics:
    """Every metric of utils/metrics.py for ``[B, H, W]`` device tensors in one pass, without a host sync.

    ``mask``: bool, ``None`` = every pixel; ``maxdisp`` ANDs it with ``(gt > 0) & (gt < maxdisp)``
    (train_kitti.py:221, test_kitti.py:120) without building a mask tensor.  Crops such as
    ``pred[:, hi-h:, wi-w:]`` are read in place; a tensor whose innermost stride is not 1 is copied."""
    _check_shape(*((D_est, D_gt) if mask is None else (D_est, D_gt, mask)))
    B, K = int(D_gt.shape[0]), len(thres)
    dev = D_gt.device
    if not dev.type == "cuda":
        raise RuntimeError("esmstereo_amd.metrics: the inputs must be on the GPU (no CPU fallback)")
    records = torch.empty(B, METRICS_RECORD_DOUBLES, device=dev, dtype=torch.float64)
    values = torch.empty(B, METRICS_VALUES, device=dev, dtype=torch.float32)
    batch = torch.empty(METRICS_VALUES, device=dev, dtype=torch.float32)
    _launch(D_est, D_gt, mask, maxdisp, thres, records, values, batch)
    return DisparityMetrics(records, values, batch, K)


def EPE_metric(D_est, D_gt, mask):
    """utils/metrics.py:70-74."""
    _check_shape(D_est, D_gt, mask)
    return disparity_metrics(D_est, D_gt, mask, thres=()).batch_epe


def D1_metric(D_est, D_gt, mask):
    """utils/metrics.py:42-48."""
    return D1_metric_thres(D_est, D_gt, mask, 3)


def D1_metric_thres(D_est, D_gt, mask, thres):
    """utils/metrics.py:51-57."""
    _check_shape(D_est, D_gt, mask)
    return disparity_metrics(D_est, D_gt, mask, thres=(thres,)).batch_d1[0]


def Thres_metric(D_est, D_gt, mask, thres):
    """utils/metrics.py:60-67."""
    _check_shape(D_est, D_gt, mask)
    assert isinstance(thres, (int, float))
    return disparity_metrics(D_est, D_gt, mask, thres=(thres,)).batch_thres[0]


def vis(D_est: torch.Tensor, D_gt: torch.Tensor, abs_thres: float = 3., rel_thres: float = .05,
        dilate_radius: int = 1) -> torch.Tensor:
    """utils/visualization.py:20-37 on device tensors: fp32 ``[B, 3, H, W]``, bit-exact with the numpy original.
    ``dilate_radius`` is accepted and ignored, as there."""
    _check_shape(D_est, D_gt)
    B, H, W = (int(v) for v in D_gt.shape)
    est, pe, eb, eh = _view(D_est, torch.float32, "D_est")
    gt, pg, gb, gh = _view(D_gt, torch.float32, "D_gt")
    if est.device != gt.device:
        raise RuntimeError("esmstereo_amd.metrics: inputs on different devices")
    out = torch.empty(B, 3, H, W, device=gt.device, dtype=torch.float32)
    with torch.cuda.device(gt.device):
        check(lib.esm_disp_error_map_f32(pe, eb, eh, pg, gb, gh, out.data_ptr(), B, H, W, float(abs_thres),
                                         float(rel_thres), _stream(gt)), "disp_error_map")
    return out


error_image = vis


class DisparityEvaluator:
    """A dataset loop's scores: ``update`` enqueues the kernels and keeps the per-image records on the device
    (no sync), ``summary`` reads them back once.

        ev = DisparityEvaluator()
        for left, right, gt in loader:
            ev.update(model(left, right)[-1][:, top:, left_pad:], gt, maxdisp=192)
        print(ev.summary())
    """
    THRES: Tuple[float, float, float] = (1., 2., 3.)  # Thres1 / Thres2 / Thres3 of train_kitti.py:230-232; D1 is d1[2]

    def __init__(self, capacity: int = 256):
        self._cap = max(1, int(capacity))
        self._n = 0
        self._rec: Optional[torch.Tensor] = None  # [cap, 12] fp64
        self._val: Optional[torch.Tensor] = None  # [cap, 10] fp32
        self._batch: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return self._n

    def _reserve(self, dev: torch.device, more: int) -> None:
        if self._rec is None:
            while self._cap < more:
                self._cap *= 2
            self._rec = torch.empty(self._cap, METRICS_RECORD_DOUBLES, device=dev, dtype=torch.float64)
            self._val = torch.empty(self._cap, METRICS_VALUES, device=dev, dtype=torch.float32)
            self._batch = torch.empty(METRICS_VALUES, device=dev, dtype=torch.float32)
        if self._rec.device != dev:
            raise RuntimeError("DisparityEvaluator: every update must be on the same device")
        if self._n + more > self._cap:
            while self._cap < self._n + more:
                self._cap *= 2
            for name in ("_rec", "_val"):
                old = getattr(self, name)
                new = torch.empty(self._cap, old.shape[1], device=dev, dtype=old.dtype)
                new[:self._n].copy_(old[:self._n])  # stream-ordered device copy
                setattr(self, name, new)

    def update(self, D_est: torch.Tensor, D_gt: torch.Tensor, mask: Optional[torch.Tensor] = None,
               maxdisp: Optional[float] = None) -> None:
        _check_shape(*((D_est, D_gt) if mask is None else (D_est, D_gt, mask)))
        if not D_gt.is_cuda:
            raise RuntimeError("esmstereo_amd.metrics: the inputs must be on the GPU (no CPU fallback)")
        B = int(D_gt.shape[0])
        self._reserve(D_gt.device, B)
        _launch(D_est, D_gt, mask, maxdisp, self.THRES, self._rec[self._n:self._n + B],
                self._val[self._n:self._n + B], self._batch)
        self._n += B

    def summary(self) -> Dict[str, float]:
        """Means over the images the reference keeps (its skip rule) of the per-image fp32 EPE, D1, Thres1-3, and
        the two numbers test_kitti.py:141-142 prints: ``kitti_epe`` = mean over all images of sum |E| / n_mask,
        ``kitti_gt3`` (">3.0") = mean over all images of n_abs(3) / n_mask.  One readback."""
        if self._n == 0:
            return {"images": 0, "kept": 0}
        host = torch.cat([self._rec[:self._n], self._val[:self._n].double()], dim=1).cpu().numpy()
        rec, val = host[:, :METRICS_RECORD_DOUBLES], host[:, METRICS_RECORD_DOUBLES:]
        kept = val[:, METRICS_VALUES - 1] == 0
        M = METRICS_MAX_THRES
        out: Dict[str, float] = {"images": int(self._n), "kept": int(kept.sum())}
        cols = {"EPE": 0, "D1": 1 + M + 2, "Thres1": 1, "Thres2": 2, "Thres3": 3}
        for name, c in cols.items():
            out[name] = float(val[kept, c].mean()) if kept.any() else 0.0
        with np.errstate(divide="ignore", invalid="ignore"):  # an empty mask: NaN, as np.mean of nothing
            out["kitti_epe"] = float((rec[:, 2] / rec[:, 0]).mean())
            out["kitti_gt3"] = float((rec[:, 4 + 2] / rec[:, 0]).mean())
        return out
