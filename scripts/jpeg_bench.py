"""Time the device JPEG encoder (csrc/jpeg.hip) against the host path it replaces.

    python scripts/jpeg_bench.py [--part wall|device] [--reps 30] [--rounds 3] [--json profiles/jpeg_bench.json]

Inputs, at quality 75 / 4:2:0 / Ri = 8: the nodes' two-panel frame (scripts/png_bench.py's: a camera-like left image
over the colour-mapped S-K benchmark disparity, 750 x 1242 x 3) and a four-panel frame of the confidence node's size
(1500 x 2484 x 3: that frame beside a second colour map of it, over both mirrored).  Per frame:
  host path   WALL time of what cv::VideoWriter's MJPG path costs the nodes: download of the raw frame, then PIL's
              Image.save(..., "JPEG", quality=75, subsampling=2) (libjpeg on one core);
  device path WALL time of render.JpegEncoder.encode: three launches, one synchronisation, download of the compressed
              bytes, the header put in front;
  launches    (--part device, a run of its own) DEVICE time of each of the three kernels from the profiler's kernel
              records (null when the profiler gives none: unmeasured), and of the three together between one pair of
              device events;
  sizes       both files' bytes, and the raw frame's.
Wall times are time.perf_counter around a call that ends synchronised; the two sides alternate in one loop and the
median is reported; the measurement is repeated `rounds` times and the spread of the medians is the noise a
difference has to exceed.  Both files are decoded with PIL and compared with the input (PSNR) before anything is
timed.  --json merges the part's results into the file.  Fails without a GPU."""
import argparse
import io as _io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import png_bench  # noqa: E402

QUALITY, SUB, RI = 75, "420", 8


def launch_name(kernel: str) -> str:
    """The launch a profiler record belongs to (the record's name is the kernel's, mangled or not)."""
    if "jpeg_scan_kernel" in kernel:
        return "2 jpeg_scan_kernel"
    emit = "<true, true>" in kernel or "ILb1ELb1" in kernel
    return "3 jpeg_interval_kernel<420, emit>" if emit else "1 jpeg_interval_kernel<420, count>"


def frames(dev):
    """The two-panel frame [750, 1242, 3] and the four-panel frame [1500, 2484, 3], BGR uint8 on the device."""
    from esmstereo_amd import render
    T, L, H, W = png_bench.TOP, png_bench.LEFT, png_bench.H, png_bench.W
    disp = png_bench.benchmark_disparity(dev)
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = 128 + 60 * torch.sin(xx / 41.0) + 50 * torch.cos(yy / 29.0)
    left = (base.unsqueeze(-1) + 10 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)
    left = left.unsqueeze(0).contiguous().to(dev)
    crop = disp[:, T:T + H, L:L + W]
    two = render.colorize_disparity(crop, render.colormap_lut("jet", dev), stack=left)[0].contiguous()
    other = render.colorize_disparity(crop, render.colormap_lut("magma", dev), stack=left)[0]
    top = torch.cat([two, other], dim=1)
    four = torch.cat([top[:H], top[H:].flip(1), top[:H].flip(0), top[H:]], dim=0).contiguous()
    return two, four


def psnr(a, b):
    return float(10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def kernel_times_us(fn, reps=20):
    """{kernel: median device us} of the three launches over `reps` calls, from the profiler; None when it has none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        per = {}
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA and "jpeg_" in e.name:
                per.setdefault(launch_name(e.name), []).append(e.time_range.elapsed_us())
        return {k: float(np.median(v)) for k, v in per.items()} or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="wall", choices=["wall", "device"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench: needs a ROCm GPU")
    from PIL import Image
    from esmstereo_amd import render
    from esmstereo_amd._lib import check, lib
    dev = torch.device("cuda")
    out = {}
    if args.json and os.path.exists(args.json):
        with open(args.json) as f:
            out = json.load(f)
    out.update({"device": torch.cuda.get_device_name(0), "quality": QUALITY, "subsampling": SUB, "restart_mcus": RI,
                "times": "host_* and device_* are WALL ms per frame of the whole call; launches_* are DEVICE times",
                "launch_3": "recomputes the interval (the only form built; a parked segment was not tried)"})
    for name, frame in zip(("frame_750x1242_bgr8", "frame_1500x2484_bgr8"), frames(dev)):
        h, w = int(frame.shape[0]), int(frame.shape[1])
        enc = render.JpegEncoder(1, h, w, QUALITY, SUB, RI)
        rec = out.setdefault(name, {})

        def host():
            b = _io.BytesIO()
            Image.fromarray(frame.cpu().numpy()[:, :, ::-1]).save(b, "JPEG", quality=QUALITY, subsampling=2)
            return b.getvalue()

        def device():
            return enc.encode(frame, "bgr")[0]

        def launch():
            check(lib.esm_jpeg_encode_rgb8(frame.data_ptr(), 1, h, w, 1, QUALITY, 420, RI, enc.work.data_ptr(),
                                           enc.out.data_ptr(), enc.slot, enc.lengths.data_ptr(),
                                           render._stream(enc.work)), "jpeg")

        if args.part == "wall":
            files = {"host": host(), "device": device()}
            rgb = frame.cpu().numpy()[:, :, ::-1]
            quality = {k: psnr(np.asarray(Image.open(_io.BytesIO(v)).convert("RGB")), rgb) for k, v in files.items()}
            rounds = [png_bench.wall_medians([host, device], args.reps) for _ in range(args.rounds)]
            s = png_bench.summary(rounds)
            rec.update({"raw_bytes": 3 * h * w, "host_download_pil_save": s[0], "device_jpeg_encode": s[1],
                        "speedup_wall": s[0]["median_ms"] / s[1]["median_ms"],
                        "host_file_bytes": len(files["host"]), "device_file_bytes": len(files["device"]),
                        "device_over_host_bytes": len(files["device"]) / len(files["host"]),
                        "psnr_db": quality, "rounds_ms": rounds})
        else:
            rec.update({"launches_device_us": kernel_times_us(launch),
                        "launches_device_ms_event_pair": png_bench.event_ms(launch)})
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
