"""Time esmstereo_amd.render against what a user does without it.

    python scripts/render_bench.py [--reps 100] [--json out.json]

Shapes: KITTI, 1 x 375 x 1242, and 8 x 544 x 960.  Two renderings: SCALE (save_vid.py:119-122) and RANGE stacked
under the left frame (the ROS node's picture).  Three sides produce the same frame on the host's side of the
event pair they are timed with, in the same loop, alternating, each repetition between its own pair of device events:

  ours   the op (one launch, RANGE two), the frame left on the device
  torch  the same definitions written with torch ops on the GPU (what rendering on the GPU costs without the op)
  host   the reference's route: the fp32 map copied to the host, then numpy on the CPU (its event pair spans the
         copy and the CPU work, as a user's loop would)

Reported per shape and rendering: the median, the 5th and 95th percentile of each side, and the speed-ups.  The three
sides' frames are compared before anything is timed.  The host route keeps the GPU idle for milliseconds per
repetition and `ours` is the launch that follows it, so the two device sides are also timed a second time alternating
with each other only (`*_back_to_back`).

Kernel time comes from a kernel trace taken in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python scripts/render_bench.py --trace-run
    python scripts/render_bench.py --trace-dir DIR [--json out.json]

--trace-run launches each configuration TRACE_REPS times in a fixed order and nothing else of this library; --trace-dir
splits the trace's dispatches of each kernel into those runs and reports the median kernel time per configuration and
its fraction of 8 TB/s on the algorithmic bytes (4 H W read + 3 H W written per image; RANGE reads the map twice and
the stack moves 6 H W more).  Fails without a GPU."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12
SHAPES = ((1, 375, 1242), (8, 544, 960))
RENDERINGS = ("scale", "range_stacked")
TRACE_REPS = 40


def algorithmic_bytes(rendering, B, H, W):
    px = B * H * W
    return px * (4 + 3) if rendering == "scale" else px * (4 + 4 + 3 + 6)


def make_inputs(B, H, W, dev):
    g = torch.Generator().manual_seed(B * H)
    d = torch.rand(B, H, W, generator=g) * 190 + 1
    d[torch.rand(B, H, W, generator=g) < 0.2] = 0  # the node's invalid pixels
    left = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    lut = torch.randint(0, 256, (256, 3), generator=g, dtype=torch.uint8)
    return d.to(dev), left.to(dev), lut.to(dev)


def ours(rendering, d, left, lut):
    from esmstereo_amd import render as R
    return R.colorize_disparity(d, lut) if rendering == "scale" else R.colorize_range(d, lut, stack=left)


def torch_formulation(rendering, d, left, lut):
    """The definitions of include/esmstereo_amd.h with torch ops (round = half to even, as rint)."""
    if rendering == "scale":
        u = (torch.round(d * 256).to(torch.int32) & 0xFFFF).float()
        idx = torch.round(u * 0.01).clamp_(0, 255).long()
        return lut[idx]
    valid = d > 0
    u = torch.where(valid, torch.round(d * 256).clamp_max(65535), torch.zeros((), device=d.device))
    big = torch.full((), 1e9, device=d.device)
    mn = torch.where(valid, u, big).amin(dim=(1, 2), keepdim=True).double()
    mx = torch.where(valid, u, -big).amax(dim=(1, 2), keepdim=True).double()
    span = mx - mn
    a, b = (-255.0 / span).float(), (255.0 * mx / span).float()
    idx = torch.round(u * a + b).clamp_(0, 255)
    idx = torch.where(span > 0, idx, torch.zeros((), device=d.device)).long()
    return torch.cat((left, lut[idx]), dim=1)


def host_route(rendering, d, left_host, lut_host):
    """fp32 device-to-host, then numpy on the CPU, as the reference's scripts do with cv2."""
    x = d.cpu().numpy()
    if rendering == "scale":
        u = (np.rint(x * np.float32(256)).astype(np.int32) & 0xFFFF).astype(np.float32)
        return lut_host[np.clip(np.rint(u * np.float32(0.01)), 0, 255).astype(np.intp)]
    out = np.empty((x.shape[0], 2 * x.shape[1], x.shape[2], 3), np.uint8)
    for i, m in enumerate(x):
        valid = m > 0
        u = np.where(valid, np.minimum(np.rint(m * np.float32(256)), np.float32(65535)), np.float32(0))
        idx = np.zeros(m.shape, np.intp)
        if valid.any():
            mn, mx = float(u[valid].min()), float(u[valid].max())
            if mx > mn:
                a, b = np.float32(-255.0 / (mx - mn)), np.float32(255.0 * mx / (mx - mn))
                idx = np.clip(np.rint(u * a + b), 0, 255).astype(np.intp)
        out[i, :m.shape[0]] = left_host[i]
        out[i, m.shape[0]:] = lut_host[idx]
    return out


def paired_times(fns, reps, warmup=10):
    """ms of each callable per repetition, alternating them, each call between its own pair of events."""
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
    return [np.array([a.elapsed_time(b) for a, b in row]) for row in ev]


def spread(t, unit="ms"):
    return {f"median_{unit}": float(np.median(t)), f"p05_{unit}": float(np.percentile(t, 5)),
            f"p95_{unit}": float(np.percentile(t, 95))}


def bench(reps):
    dev = torch.device("cuda")
    rows = []
    for B, H, W in SHAPES:
        d, left, lut = make_inputs(B, H, W, dev)
        left_host, lut_host = left.cpu().numpy(), lut.cpu().numpy()
        for rendering in RENDERINGS:
            a = ours(rendering, d, left, lut).cpu().numpy()
            assert np.array_equal(a, torch_formulation(rendering, d, left, lut).cpu().numpy())
            assert np.array_equal(a, host_route(rendering, d, left_host, lut_host))  # the same frame is being timed
            t = paired_times([lambda: ours(rendering, d, left, lut), lambda: torch_formulation(rendering, d, left, lut),
                              lambda: host_route(rendering, d, left_host, lut_host)], reps)
            # the two device sides again without the host route between them: its CPU work leaves the GPU idle for
            # milliseconds, and the first launch after such a gap (always `ours`, above) pays for the wake-up
            t2 = paired_times([lambda: ours(rendering, d, left, lut),
                               lambda: torch_formulation(rendering, d, left, lut)], reps)
            row = {"shape": [B, H, W], "rendering": rendering, "ours": spread(t[0]), "torch": spread(t[1]),
                   "host": spread(t[2]), "ours_back_to_back": spread(t2[0]), "torch_back_to_back": spread(t2[1])}
            row["speedup_vs_torch"] = row["torch"]["median_ms"] / row["ours"]["median_ms"]
            row["speedup_vs_host"] = row["host"]["median_ms"] / row["ours"]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def trace_run():
    dev = torch.device("cuda")
    for B, H, W in SHAPES:
        d, left, lut = make_inputs(B, H, W, dev)
        for rendering in RENDERINGS:
            for _ in range(TRACE_REPS):
                ours(rendering, d, left, lut)
            torch.cuda.synchronize()


def trace_summary(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {trace_dir}")
    disp = {"render_kernel": [], "range_partial_kernel": []}
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                for k in disp:
                    if k in r["Kernel_Name"]:
                        t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
                        disp[k].append((t0, (t1 - t0) * 1e-3))  # ns -> us
    configs = [(s, r) for s in SHAPES for r in RENDERINGS]
    us = {k: [t for _, t in sorted(v)] for k, v in disp.items()}
    if len(us["render_kernel"]) != TRACE_REPS * len(configs):
        raise SystemExit(f"expected {TRACE_REPS * len(configs)} render_kernel dispatches, "
                         f"found {len(us['render_kernel'])}")
    rows, n_range = [], 0
    for i, ((B, H, W), rendering) in enumerate(configs):
        t = np.array(us["render_kernel"][i * TRACE_REPS:(i + 1) * TRACE_REPS])
        row = {"shape": [B, H, W], "rendering": rendering, "render_kernel": spread(t, "us")}
        total = float(np.median(t))
        if rendering != "scale":
            p = np.array(us["range_partial_kernel"][n_range * TRACE_REPS:(n_range + 1) * TRACE_REPS])
            n_range += 1
            row["range_partial_kernel"] = spread(p, "us")
            total += float(np.median(p))
        row["kernel_us"] = total
        row["algorithmic_bytes"] = algorithmic_bytes(rendering, B, H, W)
        row["frac_of_8TBs"] = row["algorithmic_bytes"] / (total * 1e-6) / HBM_BYTES_PER_S
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-run", action="store_true", help="the launches alone, for rocprofv3 --kernel-trace")
    ap.add_argument("--trace-dir", default=None, help="summarise the kernel trace written under this directory")
    args = ap.parse_args()
    if args.trace_dir:
        rows, device = trace_summary(args.trace_dir), None
    else:
        if not torch.cuda.is_available():
            raise SystemExit("render_bench: needs a ROCm GPU")
        device = torch.cuda.get_device_name(0)
        if args.trace_run:
            trace_run()
            return
        rows = bench(args.reps)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": device, "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
