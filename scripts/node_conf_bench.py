"""Time the confidence-gated node's two entry points (csrc/node_conf.hip) against what a user has without them.

    python scripts/node_conf_bench.py [--reps 200] [--rounds 5] [--json out.json]

Shape: KITTI, a 375 x 1242 image in a 384 x 1248 map, B = 1.
  filter  esm_node_filter_conf_u16 with conf = NULL (the LDS-tiled median, selection network) against
          esm_node_filter_u16 (25 global loads and a full sort per pixel) on the same input, and with the gate on;
  panels  esm_node_panels_u8 against the same frame from the existing calls plus torch ops: colorize_range with the
          left image stacked, the error map, the confidence map and the two concatenations in torch.
The sides of a comparison are timed in the same loop, alternating, each call between its own pair of device events;
the median is reported.  The whole measurement is repeated `rounds` times: the spread of the medians is the
run-to-run noise a difference has to exceed.  Bytes are the algorithmic ones (each input read once, each output
written once), the fraction of 8 TB/s is theirs over the median time.  Both sides are checked to give the same bytes
before anything is timed.  Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import esmstereo_amd as E  # noqa: E402
from esmstereo_amd._lib import check, lib  # noqa: E402

HBM_BYTES_PER_S = 8e12
H, W, HP, WP = 375, 1242, 384, 1248
MAX_DISP = 192.0
# the node's error table as the bytes land in the frame (kitti_publisher_conf_cuda_node.cpp:69-92, RGB -> BGR)
ERR_BGR = [[149, 54, 49], [180, 117, 69], [209, 173, 116], [233, 217, 171], [248, 243, 224], [144, 224, 254],
           [97, 174, 253], [67, 109, 244], [39, 48, 215], [38, 0, 165]]
ERR_EDGES = [2.0 ** k for k in range(-4, 5)]  # 1/16 .. 16: the inner bounds of the ten rows


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


def summary(rounds):
    """Per side: the median of the rounds' medians and their spread (max - min)."""
    a = np.asarray(rounds)
    return [{"median_ms": float(np.median(col)), "spread_ms": float(col.max() - col.min())} for col in a.T]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("node_conf_bench: needs a ROCm GPU")
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    # a smooth disparity with noise and holes, like a network's output, in the padded map
    yy, xx = torch.meshgrid(torch.arange(HP), torch.arange(WP), indexing="ij")
    disp = (40 + 30 * torch.sin(xx / 97.0) + 20 * torch.cos(yy / 53.0) + torch.randn(HP, WP, generator=g)).float()
    disp[torch.rand(HP, WP, generator=g) < 0.02] = -1.0
    disp = disp.unsqueeze(0).contiguous().to(dev)
    conf = torch.rand(1, HP, WP, generator=g).to(dev)
    gt = (disp[:, :H, :W].cpu() + torch.randn(1, H, W, generator=g) * 2).clamp(0, 250)
    gt[torch.rand(1, H, W, generator=g) < 0.3] = 0
    gt16 = (gt * 256).round().to(torch.int32).to(torch.int16).to(dev)  # the bits of the uint16 map
    left = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    lut = E.colormap_lut("magma", dev)
    u_new = torch.empty(1, H, W, dtype=torch.int16, device=dev)
    u_old = torch.empty_like(u_new)
    f_new = torch.empty(1, H, W, device=dev)
    f_old = torch.empty_like(f_new)
    frame = torch.empty(1, 2 * H, 2 * W, 3, dtype=torch.uint8, device=dev)
    gt_f32 = torch.empty(1, H, W, device=dev)
    work = torch.empty(E.range_workspace_bytes(1, H, W), dtype=torch.uint8, device=dev)
    err_table = torch.tensor(ERR_BGR + [[0, 0, 0]], dtype=torch.uint8, device=dev)
    err_edges = torch.tensor(ERR_EDGES, device=dev)
    stream = None  # the default stream, as torch's ops use it

    def filter_new(c=None, thr=0.5):
        check(lib.esm_node_filter_conf_u16(disp.data_ptr(), c.data_ptr() if c is not None else None, u_new.data_ptr(),
                                           f_new.data_ptr(), None, 1, HP, WP, 0, 0, H, W, MAX_DISP, thr, stream),
              "node_filter_conf")

    def filter_old():
        check(lib.esm_node_filter_u16(disp.data_ptr(), u_old.data_ptr(), f_old.data_ptr(), 1, HP, WP, 0, 0, H, W,
                                      MAX_DISP, stream), "node_filter")

    def panels_new():
        check(lib.esm_node_panels_u8(f_new.data_ptr(), conf.data_ptr(), HP, WP, 0, 0, gt16.data_ptr(), left.data_ptr(),
                                     lut.data_ptr(), frame.data_ptr(), gt_f32.data_ptr(), work.data_ptr(), 1, H, W,
                                     stream), "node_panels")
        return frame

    def panels_separate():
        left_col = E.colorize_range(f_new, lut, stack=left, workspace=work)
        gtf = (gt16.to(torch.int32) & 0xFFFF).float() * (1.0 / 256.0)
        gtf = torch.where(f_new > 0, gtf, torch.zeros_like(gtf))
        err = (gtf - f_new).abs()
        rel = err / gtf
        err = torch.where(rel < err, rel, err)
        row = torch.bucketize(err, err_edges, right=True)
        row = torch.where(gtf > 0, row, torch.full_like(row, 10))
        c = torch.nan_to_num(conf[:, :H, :W] * 256.0, nan=0.0).round().clamp(0, 255).to(torch.uint8)
        right_col = torch.cat((err_table[row], c.unsqueeze(-1).expand(-1, -1, -1, 3)), dim=1)
        return torch.cat((left_col, right_col), dim=2)

    filter_new()
    filter_old()
    assert torch.equal(u_new, u_old) and torch.equal(f_new.view(torch.int32), f_old.view(torch.int32))
    assert torch.equal(panels_new(), panels_separate())  # the same frame is being timed
    filter_rounds, panel_rounds = [], []
    for _ in range(args.rounds):
        filter_rounds.append(paired_medians([filter_new, filter_old, lambda: filter_new(conf)], args.reps))
    filter_new()
    for _ in range(args.rounds):
        panel_rounds.append(paired_medians([panels_new, panels_separate], args.reps))
    px = H * W
    f_sum, p_sum = summary(filter_rounds), summary(panel_rounds)
    filter_bytes = 4 * px + 2 * px + 4 * px            # the window read once, u16 and filtered written
    # filtered (read twice: the range pass), conf, gt16, left; the frame and gt_f32 written
    panel_bytes = (4 + 4 + 2 + 3) * px + 4 * px + 12 * px + 4 * px
    out = {
        "device": torch.cuda.get_device_name(0), "shape": [1, H, W], "map": [HP, WP], "reps": args.reps,
        "rounds": args.rounds,
        "filter": {"lds_median_no_conf": f_sum[0], "node_filter_u16": f_sum[1], "lds_median_with_conf": f_sum[2],
                   "speedup": f_sum[1]["median_ms"] / f_sum[0]["median_ms"], "bytes": filter_bytes,
                   "bytes_with_conf": filter_bytes + 4 * px,
                   "frac_of_8TBs": filter_bytes / (f_sum[0]["median_ms"] * 1e-3) / HBM_BYTES_PER_S,
                   "rounds_ms": filter_rounds},
        "panels": {"node_panels_u8": p_sum[0], "separate_calls_and_torch": p_sum[1],
                   "speedup": p_sum[1]["median_ms"] / p_sum[0]["median_ms"], "bytes": panel_bytes,
                   "frac_of_8TBs": panel_bytes / (p_sum[0]["median_ms"] * 1e-3) / HBM_BYTES_PER_S,
                   "rounds_ms": panel_rounds},
    }
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
