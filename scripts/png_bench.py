"""Time the device PNG encoder (csrc/png.hip) against the host writers it stands beside.

    python scripts/png_bench.py [--reps 30] [--rounds 3] [--json profiles/png_bench.json]

Inputs: the S-K benchmark's own disparity (bench.py configs[1]: ESMStereo-S gwc 384 x 1248, seeded weights and inputs,
one replay of the hot path), cropped as save_disp.py:81 does to 375 x 1242, and the stacked two-panel frame
(save_vid.py:125: a camera-like left image over the colour-mapped disparity, 750 x 1242 x 3).  Per image:
  host path   WALL time of what the parent does: download of the raw map / frame, then io.png_u16_bytes /
              render.png_rgb8_bytes (zlib level 6 on one core, filter 0);
  device path WALL time of io.png_encode_disparity (the rounding inside the encoder), io.png_encode_u16 and
              render.png_encode_bgr8: three launches, one synchronisation, download of the compressed bytes, CRC-32 and
              chunk framing on the host; and, inside it, the wall time of the host CRC-32 alone;
  launches    DEVICE time of each of the three kernels, from the profiler's kernel records (null when the profiler gives
              none: unmeasured), and of the three together between one pair of device events;
  sizes       both files' bytes, and the raw scanline bytes.
Wall times are time.perf_counter around a call that ends synchronised; the two sides alternate in one loop and the
median is reported; the measurement is repeated `rounds` times and the spread of the medians is the noise a difference
has to exceed.  Every file is decoded (with PIL, when it is installed) and compared with the input before anything is
timed.  Fails without a GPU."""
import argparse
import io as _io
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

TOP, LEFT, H, W = 9, 0, 375, 1242  # save_disp.py:81 disp[top_pad:, :-right_pad] of the 384 x 1248 map


def benchmark_disparity(dev):
    """The S-K step's output on bench.py's own inputs: fp32 [1, 384, 1248] on the device."""
    bench._load_package()
    E = bench.E
    cfg = dict(variant="S", cv="gwc", height=384, width=1248, maxdisp=192)
    backbone, cvs = bench.VARIANTS[cfg["variant"]]
    model = E.ESMStereo(cfg["maxdisp"], True, False, backbone, cvs)
    bench.seeded_init(model, 1234)
    bench.load_seeded_weights(model, cfg["variant"], cfg["cv"])
    model = model.eval().to(dev)
    ml, mr, att, up = bench.bench_inputs(cfg["variant"], cfg["cv"], 1, cfg["height"], cfg["width"], cfg["maxdisp"],
                                         bench.INPUT_SEED[1], dev)
    B, C, h, w = (int(v) for v in ml.shape)
    hp = E.HotPath(model, B, h, w, 0 if att is None else int(att.shape[1]), [tuple(u.shape) for u in up], dev,
                   channels=C)
    hp.load_inputs(ml, mr, att, up)
    hp.launch()
    torch.cuda.synchronize()
    d = hp.outputs[0].detach().clone().float()
    return d.reshape(1, cfg["height"], cfg["width"])


def wall_medians(fns, reps, warmup=3):
    """Median wall ms of each callable (each ends synchronised), alternating them."""
    for _ in range(warmup):
        for f in fns:
            f()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(v)) for v in t]


def summary(rounds):
    a = np.asarray(rounds)
    return [{"median_ms": float(np.median(col)), "spread_ms": float(col.max() - col.min())} for col in a.T]


PNG_KERNELS = ("png_count_kernel", "png_table_kernel", "png_emit_kernel")


def kernel_times_us(fn, reps=20, names=PNG_KERNELS):
    """{kernel: median device us} of the kernels `names` over `reps` calls, from the profiler; None when it has none
    (why is printed to stderr)."""
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
            key = next((k for k in names if k in e.name), None)
            if e.device_type == torch.autograd.DeviceType.CUDA and key is not None:
                per.setdefault(key, []).append(e.time_range.elapsed_us())
        if not per:
            print(f"kernel_times_us: the profiler recorded none of {names}: unmeasured", file=sys.stderr)
        return {k: float(np.median(v)) for k, v in per.items()} or None
    except Exception as e:  # noqa: BLE001  (no profiler, or one that fails: the times stay unmeasured, and say why)
        print(f"kernel_times_us: unmeasured: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def event_ms(fn, reps=50):
    """Median device ms between a pair of events around one un-synchronised call."""
    for _ in range(5):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def decoded(png: bytes):
    try:
        from PIL import Image
    except ImportError:
        return None
    return np.asarray(Image.open(_io.BytesIO(png)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_bench: needs a ROCm GPU")
    dev = torch.device("cuda")
    disp = benchmark_disparity(dev)
    from esmstereo_amd import io as EIO, render
    from esmstereo_amd._lib import check, lib

    u16 = EIO.disparity_to_u16(disp, TOP, LEFT, H, W)
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = 128 + 60 * torch.sin(xx / 41.0) + 50 * torch.cos(yy / 29.0)
    left = (base.unsqueeze(-1) + 10 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)
    left = left.unsqueeze(0).contiguous().to(dev)
    frame = render.colorize_disparity(disp[:, TOP:TOP + H, LEFT:LEFT + W], render.colormap_lut("jet", dev),
                                      stack=left).contiguous()  # [1, 750, 1242, 3] BGR

    def host_u16():
        return EIO.png_u16_bytes(u16[0].cpu().numpy())

    def dev_disp():
        return EIO.png_encode_disparity(disp, TOP, LEFT, H, W)[0]

    def dev_u16():
        return EIO.png_encode_u16(u16)[0]

    def host_frame():
        return render.png_rgb8_bytes(frame[0].cpu().numpy(), "bgr")

    def dev_frame():
        return render.png_encode_bgr8(frame)[0]

    # the same picture on both sides, before anything is timed
    ref16 = u16[0].cpu().numpy()
    files = {"host_u16": host_u16(), "device_disparity": dev_disp(), "device_u16": dev_u16(),
             "host_frame": host_frame(), "device_frame": dev_frame()}
    assert files["device_disparity"] == files["device_u16"]
    for k in ("host_u16", "device_u16"):
        got = decoded(files[k])
        assert got is None or np.array_equal(got.astype(np.uint16), ref16), k
    for k in ("host_frame", "device_frame"):
        got = decoded(files[k])
        assert got is None or np.array_equal(got, frame[0].cpu().numpy()[:, :, ::-1]), k

    map_rounds = [wall_medians([host_u16, dev_disp, dev_u16], args.reps) for _ in range(args.rounds)]
    frame_rounds = [wall_medians([host_frame, dev_frame], args.reps) for _ in range(args.rounds)]
    m_sum, f_sum = summary(map_rounds), summary(frame_rounds)

    def crc_ms(png):
        t0 = time.perf_counter()
        for _ in range(20):
            zlib.crc32(png)
        return (time.perf_counter() - t0) / 20 * 1e3

    enc16 = EIO.png_encoder(1, H, 2 * W, dev)
    enc24 = EIO.png_encoder(1, 2 * H, 3 * W, dev)

    def launch_disp():
        check(lib.esm_png_encode_disp_f32(disp.data_ptr(), 1, 384, 1248, TOP, LEFT, H, W, *enc16._args("sub")), "png")

    def launch_frame():
        check(lib.esm_png_encode_rgb8(frame.data_ptr(), 1, 2 * H, W, 1, *enc24._args("sub")), "png")

    out = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
        "chunk_bytes": lib.esm_png_chunk_bytes(),
        "times": "host_* and device_* are WALL ms per image of the whole call; launches_* are DEVICE times",
        "map_375x1242_u16": {
            "raw_bytes": H * (1 + 2 * W),
            "host_download_png_u16_bytes": m_sum[0], "device_png_encode_disparity": m_sum[1],
            "device_png_encode_u16": m_sum[2],
            "speedup_wall": m_sum[0]["median_ms"] / m_sum[1]["median_ms"],
            "host_file_bytes": len(files["host_u16"]), "device_file_bytes": len(files["device_u16"]),
            "host_crc32_ms": crc_ms(files["device_u16"]),
            "launches_device_us": kernel_times_us(launch_disp), "launches_device_ms_event_pair": event_ms(launch_disp),
            "rounds_ms": map_rounds},
        "frame_750x1242_bgr8": {
            "raw_bytes": 2 * H * (1 + 3 * W),
            "host_download_png_rgb8_bytes": f_sum[0], "device_png_encode_bgr8": f_sum[1],
            "speedup_wall": f_sum[0]["median_ms"] / f_sum[1]["median_ms"],
            "host_file_bytes": len(files["host_frame"]), "device_file_bytes": len(files["device_frame"]),
            "host_crc32_ms": crc_ms(files["device_frame"]),
            "launches_device_us": kernel_times_us(launch_frame), "launches_device_ms_event_pair": event_ms(launch_frame),
            "rounds_ms": frame_rounds},
    }
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
