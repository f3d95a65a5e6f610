"""Time the device point cloud op (csrc/cloud.hip) against the host path it replaces.

    python scripts/cloud_bench.py [--reps 30] [--rounds 3] [--json profiles/cloud_bench.json]

Input: the S-K benchmark's own disparity (scripts/png_bench.py's: bench.py's seeded ESMStereo-S gwc 384 x 1248 step),
cropped to 375 x 1242, a camera-like left image of that size, the KITTI camera (fx 721.5377, baseline 0.54), points
kept for 0 <= Z <= 80.  Per frame, coloured (16-byte records) and not (12-byte):
  host path   WALL time of what a caller does without the op: download of the fp32 map and the frame, then the
              reprojection and the boolean mask in numpy on one core;
  device path WALL time of CloudBuilder.build: three launches, one synchronisation for the count, download of the kept
              records;
  launches    DEVICE time of each of the three kernels, from the profiler's kernel records (null when the profiler gives
              none: unmeasured), and of the three together between one pair of device events.
Method as scripts/png_bench.py: wall times are time.perf_counter around a call that ends synchronised; the two sides
alternate in one loop and the median of `reps` is reported; the measurement is repeated `rounds` times and the spread of
the medians is the noise a difference has to exceed.  Both sides' records are compared byte for byte before anything
is timed.  Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import png_bench  # noqa: E402

FX, BASELINE, Z_MIN, Z_MAX = 721.5377, 0.54, 0.0, 80.0
KERNELS = ("cloud_count_kernel", "cloud_scan_kernel", "cloud_emit_kernel")


def host_points(disp, frame, values, dtype):
    """The numpy path: fp32 throughout, one operation per line, the boolean mask."""
    num, fx, fy, cx, cy = (np.float32(v) for v in values)
    H, W = disp.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    with np.errstate(all="ignore"):
        Z = num / disp
        X = (x - cx) * Z / fx
        Y = (y - cy) * Z / fy
        keep = (disp > 0) & (Z >= np.float32(Z_MIN)) & (Z <= np.float32(Z_MAX))
    out = np.empty(int(keep.sum()), dtype=dtype)
    out["x"], out["y"], out["z"] = X[keep], Y[keep], Z[keep]
    if frame is not None:
        c = frame[keep]
        out["red"], out["green"], out["blue"], out["alpha"] = c[:, 2], c[:, 1], c[:, 0], 255
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cloud_bench: needs a ROCm GPU")
    dev = torch.device("cuda")
    T, L, H, W = png_bench.TOP, png_bench.LEFT, png_bench.H, png_bench.W
    disp = png_bench.benchmark_disparity(dev)[:, T:T + H, L:L + W]  # a crop, read where it lies
    from esmstereo_amd import cloud
    from esmstereo_amd._lib import check, lib, _stream

    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = 128 + 60 * torch.sin(xx / 41.0) + 50 * torch.cos(yy / 29.0)
    left = (base.unsqueeze(-1) + 10 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)
    left = left.unsqueeze(0).contiguous().to(dev)
    cam = cloud.Camera(FX, BASELINE)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
           "tile_points": lib.esm_cloud_tile_points(), "pixels": H * W, "z_range": [Z_MIN, Z_MAX],
           "times": "host_* and device_* are WALL ms per frame of the whole call; launches_* are DEVICE times"}
    for name, frame in (("xyzrgb_16_bytes", left), ("xyz_12_bytes", None)):
        builder = cloud.CloudBuilder(1, H, W, 1, frame is not None, dev)
        dtype = cloud.point_dtype(frame is not None, "ply")

        def device():
            return builder.build(disp, cam, frame, None, Z_MIN, Z_MAX)[0]

        def host():
            return host_points(disp[0].cpu().numpy(), None if frame is None else frame[0].cpu().numpy(),
                               cam.values(H, W), dtype)

        a, b = device(), host()
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name  # the same points, before anything is timed
        rounds = [png_bench.wall_medians([host, device], args.reps) for _ in range(args.rounds)]
        s = png_bench.summary(rounds)
        plan = next(iter(builder._plans.values())).plan

        def launch():
            check(lib.esm_plan_run(plan, _stream(builder.work)), "plan_run")

        out[name] = {"points_kept": len(a), "bytes_to_host": a.nbytes,
                     "host_bytes_downloaded": H * W * (4 + (3 if frame is not None else 0)),
                     "host_download_numpy": s[0], "device_build": s[1],
                     "speedup_wall": s[0]["median_ms"] / s[1]["median_ms"],
                     "launches_device_us": png_bench.kernel_times_us(launch, names=KERNELS),
                     "launches_device_ms_event_pair": png_bench.event_ms(launch), "rounds_ms": rounds}
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
