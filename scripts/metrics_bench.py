"""Time esmstereo_amd.metrics.disparity_metrics (and vis) against the torch-on-GPU formulation of the same
definitions, which is what scoring on the GPU costs without the op.

    python scripts/metrics_bench.py [--reps 200] [--json out.json]

Shapes: KITTI, 1 x 375 x 1242, and 8 x 544 x 960.  Both sides are timed in the same loop, alternating, each
repetition between its own pair of device events; the medians are reported.  The torch side ends in host syncs of
its own (boolean indexing, the skip rule's `if`), so its event pair spans them, as a user's loop would.
Reported per shape: median time of each side, the achieved fraction of 8 TB/s on the algorithmic bytes
((4 + 4 + 1) H W per image for the metrics, 8 H W + 12 H W for the error image), launches and host syncs per call
(counted with the profiler and torch's sync debug mode; null where the runtime does not report them).
Fails without a GPU."""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esmstereo_amd import metrics as EM  # noqa: E402

HBM_BYTES_PER_S = 8e12
THRES = (1.0, 2.0, 3.0)


def torch_formulation(est, gt, mask):
    """EPE, D1, Thres1-3 as utils/metrics.py defines them, one image and one metric at a time."""
    def per_image(fn):
        kept = []
        for e, g, m in zip(est, gt, mask):
            if m.float().mean() / (g > 0).float().mean() < 0.1:
                continue
            kept.append(fn(e[m], g[m]))
        return torch.stack(kept).mean() if kept else torch.zeros((), device=gt.device)

    out = [per_image(lambda e, g: (g - e).abs().mean())]
    out.append(per_image(lambda e, g: (((g - e).abs() > 3) & ((g - e).abs() / g.abs() > 0.05)).float().mean()))
    out += [per_image(lambda e, g, t=t: ((g - e).abs() > t).float().mean()) for t in THRES]
    return out


def ours(est, gt, mask):
    return EM.disparity_metrics(est, gt, mask, thres=THRES)


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name
                and "emset" not in e.name)
        return n or None
    except Exception:
        return None


def count_syncs(fn):
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
        return sum("synchroniz" in str(x.message) for x in w)
    except Exception:
        return None
    finally:
        torch.cuda.set_sync_debug_mode("default")


def paired_medians(fns, reps, warmup=20):
    """Median ms of each callable, alternating them, each call between its own pair of events."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
          for _ in fns]
    for r in range(reps):
        for k, f in enumerate(fns):
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return [float(np.median([a.elapsed_time(b) for a, b in row])) for row in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench: needs a ROCm GPU")
    dev = torch.device("cuda")
    rows = []
    for B, H, W in ((1, 375, 1242), (8, 544, 960)):
        g = torch.Generator().manual_seed(B * H)
        gt = torch.rand(B, H, W, generator=g) * 200
        gt[torch.rand(B, H, W, generator=g) < 0.3] = 0
        est = gt + torch.randn(B, H, W, generator=g)
        est, gt = est.to(dev), gt.to(dev)
        mask = (gt > 0) & (gt < 192)
        a, b = ours(est, gt, mask), torch_formulation(est, gt, mask)
        mine = [a.batch_epe.item(), a.batch_d1[2].item()] + a.batch_thres.tolist()
        theirs = [x.item() for x in b]
        assert np.allclose(mine, theirs, rtol=1e-5, atol=0), (mine, theirs)  # the same numbers are being timed
        t_ours, t_gate, t_torch, t_vis = paired_medians(
            [lambda: ours(est, gt, mask), lambda: EM.disparity_metrics(est, gt, maxdisp=192, thres=THRES),
             lambda: torch_formulation(est, gt, mask), lambda: EM.vis(est, gt)], args.reps)
        px = B * H * W
        rows.append({
            "shape": [B, H, W], "metrics_ms": t_ours, "metrics_range_gate_ms": t_gate, "torch_ms": t_torch,
            "error_map_ms": t_vis, "speedup": t_torch / t_ours,
            "metrics_frac_of_8TBs": 9 * px / (t_ours * 1e-3) / HBM_BYTES_PER_S,
            "metrics_range_gate_frac_of_8TBs": 8 * px / (t_gate * 1e-3) / HBM_BYTES_PER_S,
            "error_map_frac_of_8TBs": 20 * px / (t_vis * 1e-3) / HBM_BYTES_PER_S,
            "launches": {"ours": count_launches(lambda: ours(est, gt, mask)),
                         "torch": count_launches(lambda: torch_formulation(est, gt, mask))},
            "host_syncs": {"ours": count_syncs(lambda: ours(est, gt, mask)),
                           "torch": count_syncs(lambda: torch_formulation(est, gt, mask))},
        })
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
