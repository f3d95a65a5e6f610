"""Time the resizing node's two launches (csrc/resize.hip) against what a user has without them.

    python scripts/node_resize_bench.py [--reps 200] [--rounds 5] [--json out.json]

Shape: virtual KITTI, a 375 x 1242 camera frame to the 576 x 960 network input, B = 1.
  preprocess  esm_preprocess_resize_u8 (resize + network input + the resized bytes, one launch) against the nearest
              stock composition: F.interpolate(bilinear, align_corners=False) on the float image followed by the
              normalisation in torch (another rounding, the same work);
  squeeze     esm_resize_u8 of the [2 * 576, 960, 3] stacked picture to [576, 960, 3] against the same in torch.
The sides of a comparison are timed in the same loop, alternating, each call between its own pair of device events;
the median is reported.  The whole measurement is repeated `rounds` times: the spread of the medians is the
run-to-run noise a difference has to exceed.  Bytes are the algorithmic ones (each source byte once, each output
once), the fraction of 8 TB/s is theirs over the median time.  The two sides round differently, so they are checked
to agree to within the resize rule's own bound (1.3 grey levels), not bit for bit.  Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esmstereo_amd._lib import c_float, check, lib  # noqa: E402
from esmstereo_amd.io import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402

HBM_BYTES_PER_S = 8e12
H, W, HN, WN = 375, 1242, 576, 960
GREY_LEVELS = 1.3  # the distance of the 8-bit rule to an exact bilinear interpolation (tests/test_resize_host.py)


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
        raise SystemExit("node_resize_bench: needs a ROCm GPU")
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    # a smooth image with noise: neighbouring bytes differ as a camera frame's do
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = 128 + 60 * torch.sin(xx / 41.0) + 50 * torch.cos(yy / 29.0)
    img = (base.unsqueeze(-1) + 10 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)
    img = img.unsqueeze(0).contiguous().to(dev)
    stack = torch.randint(0, 256, (1, 2 * HN, WN, 3), generator=g, dtype=torch.uint8).to(dev)
    net_in = torch.empty(1, 3, HN, WN, device=dev)
    resized = torch.empty(1, HN, WN, 3, dtype=torch.uint8, device=dev)
    frame = torch.empty(1, HN, WN, 3, dtype=torch.uint8, device=dev)
    mean_c, std_c = (c_float * 3)(*IMAGENET_MEAN), (c_float * 3)(*IMAGENET_STD)
    mean_t = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std_t = torch.tensor(IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    stream = None  # the default stream, as torch's ops use it

    def preprocess_new():
        check(lib.esm_preprocess_resize_u8(img.data_ptr(), net_in.data_ptr(), resized.data_ptr(), 1, H, W, HN, WN,
                                           mean_c, std_c, stream), "preprocess_resize_u8")
        return net_in

    def preprocess_torch():
        x = F.interpolate(img.permute(0, 3, 1, 2).float(), size=(HN, WN), mode="bilinear", align_corners=False)
        return (x / 255.0 - mean_t) / std_t

    def squeeze_new():
        check(lib.esm_resize_u8(stack.data_ptr(), frame.data_ptr(), 1, 2 * HN, WN, HN, WN, 3, stream), "resize_u8")
        return frame

    def squeeze_torch():
        x = F.interpolate(stack.permute(0, 3, 1, 2).float(), size=(HN, WN), mode="bilinear", align_corners=False)
        return x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    # the same work is being timed: the two sides agree to within the rule's own rounding
    tol = GREY_LEVELS / 255.0 / min(IMAGENET_STD) + 1e-5
    diff_pre = float((preprocess_new() - preprocess_torch()).abs().max())
    diff_sq = float((squeeze_new().float() - squeeze_torch().float()).abs().max())
    assert diff_pre <= tol and diff_sq <= GREY_LEVELS + 0.5, (diff_pre, diff_sq)
    pre_rounds, sq_rounds = [], []
    for _ in range(args.rounds):
        pre_rounds.append(paired_medians([preprocess_new, preprocess_torch], args.reps))
    for _ in range(args.rounds):
        sq_rounds.append(paired_medians([squeeze_new, squeeze_torch], args.reps))
    p_sum, s_sum = summary(pre_rounds), summary(sq_rounds)
    pre_bytes = 3 * H * W + 12 * HN * WN + 3 * HN * WN  # the frame read; the fp32 input and the resized bytes written
    sq_bytes = 3 * 2 * HN * WN + 3 * HN * WN            # the stack read, the frame written
    out = {
        "device": torch.cuda.get_device_name(0), "camera": [H, W], "network": [HN, WN], "reps": args.reps,
        "rounds": args.rounds,
        "preprocess": {"preprocess_resize_u8": p_sum[0], "interpolate_and_normalise_in_torch": p_sum[1],
                       "speedup": p_sum[1]["median_ms"] / p_sum[0]["median_ms"], "bytes": pre_bytes,
                       "frac_of_8TBs": pre_bytes / (p_sum[0]["median_ms"] * 1e-3) / HBM_BYTES_PER_S,
                       "max_abs_diff": diff_pre, "rounds_ms": pre_rounds},
        "squeeze": {"resize_u8": s_sum[0], "interpolate_in_torch": s_sum[1],
                    "speedup": s_sum[1]["median_ms"] / s_sum[0]["median_ms"], "bytes": sq_bytes,
                    "frac_of_8TBs": sq_bytes / (s_sum[0]["median_ms"] * 1e-3) / HBM_BYTES_PER_S,
                    "max_abs_diff_grey_levels": diff_sq, "rounds_ms": sq_rounds},
    }
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
