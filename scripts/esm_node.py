"""Command-line form of the node loop (the reference's kitti_publisher node without ROS):

    python scripts/esm_node.py --left DIR --right DIR --out DIR [--variant S] [--max-disp 192]
        [--checkpoint ckpt.tar] [--frames N] [--picture DIR] [--net-size H W] [--confidence [--gt DIR]]
        [--record PATH [--record-quality Q]]

Reads the sorted PNG pairs of two directories (KITTI image_2 / image_3 layout), feeds them in
OpenCV's BGR channel order as the reference node does (cv::imread), runs esmstereo_amd.node.
StereoNode and writes each 16-bit disparity PNG (x256, KITTI convention) to --out, printing the
per-frame elapsed time the node prints (kitti_publisher_cuda_node.cpp:376).  With --picture it also
writes the node's "Left + Disparity" frame (the left image over the auto-ranged MAGMA disparity,
:81-86,117-118), built on the device by StereoNode.process_rendered.  Without a checkpoint
the model keeps its random initialisation (the pretrained backbone is not fetchable offline).
With --net-size H W the loop is the resizing nodes' (virtual_kitti_publisher, kitti_publisher_ess): every frame is
resized on the device to that one network size (multiples of 32) by esmstereo_amd.node.ResizeNode, and the disparity
and the picture (one network-sized frame: the stack squeezed, virtual_kitti_publisher_cuda_node.cpp:211-213) are
written at that size.  With --confidence the model is ESMStereo_confidence and the loop is the confidence-gated node's
(esmstereo_amd.node.ConfidenceNode, threshold 0.5); with --gt DIR (KITTI 16-bit ground truth of the same names) every
frame is also scored and the picture is the node's four-panel frame (process_scored).
With --record PATH the node's picture of every frame is also appended to an MJPG AVI, as the reference nodes do with
record_video (cv::VideoWriter 'MJPG' at 30 fps, video_writer.write(combined), kitti_publisher_cuda_node.cpp:122-132):
esmstereo_amd.video.MjpegWriter compresses node.dev_frame (dev_panels when scoring) on the device, so the raw frame
is not downloaded for it.  Without --record nothing of this runs and the output is unchanged.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import esmstereo_amd as E  # noqa: E402
from esmstereo_amd.node import ConfidenceNode, ResizeNode, StereoNode  # noqa: E402
from esmstereo_amd.render import write_png_bgr8  # noqa: E402
from esmstereo_amd.video import MjpegWriter  # noqa: E402

VARIANTS = {"S": ("mobilenetv2_100", 16), "M": ("efficientnet_b2", 8), "L": ("efficientnet_b2", 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--left", required=True)
    ap.add_argument("--right", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--variant", default="S", choices=sorted(VARIANTS))
    ap.add_argument("--cv", default="gwc", choices=["gwc", "nc"])
    ap.add_argument("--max-disp", type=float, default=192.0)
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--picture", default="", help="also write the left image over the MAGMA disparity here")
    ap.add_argument("--net-size", type=int, nargs=2, metavar=("H", "W"), default=None,
                    help="resize every frame to this network size (ResizeNode) instead of padding it")
    ap.add_argument("--confidence", action="store_true",
                    help="the confidence-gated node (ESMStereo_confidence, ConfidenceNode) instead of the plain one")
    ap.add_argument("--gt", default="", help="with --confidence: KITTI 16-bit ground truth; scores every frame and "
                                             "makes the picture the four-panel frame")
    ap.add_argument("--record", default="", metavar="PATH",
                    help="also append every frame's picture to this MJPG AVI, compressed on the device")
    ap.add_argument("--record-quality", type=int, default=75, help="JPEG quality of --record (1..100)")
    args = ap.parse_args()
    if args.confidence and args.net_size:
        ap.error("--confidence and --net-size are different nodes")
    if args.gt and not args.confidence:
        ap.error("--gt needs --confidence")
    backbone, cvs = VARIANTS[args.variant]
    model_cls = E.ESMStereo_confidence if args.confidence else E.ESMStereo_trt
    model = model_cls(192, args.cv == "gwc", args.cv == "nc", backbone, cvs)
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
        sd = sd.get("model", sd)
        model.load_state_dict({k.replace("module.", "", 1): v for k, v in sd.items()}, strict=False)
    model = model.eval().cuda()
    names = sorted(f for f in os.listdir(args.left) if f.endswith(".png"))
    if args.frames:
        names = names[:args.frames]
    os.makedirs(args.out, exist_ok=True)
    if args.picture:
        os.makedirs(args.picture, exist_ok=True)
    node = None
    writer = MjpegWriter(args.record, fps=30, quality=args.record_quality) if args.record else None
    for n in names:
        left = np.asarray(Image.open(os.path.join(args.left, n)).convert("RGB"))[..., ::-1]  # BGR, as cv::imread
        right = np.asarray(Image.open(os.path.join(args.right, n)).convert("RGB"))[..., ::-1]
        if node is None or left.shape[:2] != (node.h, node.w):
            if args.confidence:
                node = ConfidenceNode(model, left.shape[0], left.shape[1], args.max_disp)
            elif args.net_size:
                node = ResizeNode(model, left.shape[0], left.shape[1], args.net_size[0], args.net_size[1],
                                  args.max_disp)
            else:
                node = StereoNode(model, left.shape[0], left.shape[1], args.max_disp)
            node.warmup(np.ascontiguousarray(left), np.ascontiguousarray(right))  # plan + graph build, untimed
        if args.gt:  # the confidence node's four panels and score (kitti_publisher_conf_cuda_node.cpp:183-257)
            gt = np.asarray(Image.open(os.path.join(args.gt, n))).astype(np.uint16)
            disp, frame, epe, ms = node.process_scored(np.ascontiguousarray(left), np.ascontiguousarray(right), gt)
            if args.picture:
                write_png_bgr8(os.path.join(args.picture, n), frame)
            if writer:
                writer.write(node.dev_panels)
            print(f"{n}: EPE = {epe:.4f} (mean {node.epe_mean:.4f})", flush=True)
        elif args.picture or writer:  # the node's "Left + Disparity" frame (:81-86,117-118), built on the device
            disp, frame, ms = node.process_rendered(np.ascontiguousarray(left), np.ascontiguousarray(right))
            if args.picture:
                write_png_bgr8(os.path.join(args.picture, n), frame)
            if writer:  # video_writer.write(combined) (:130-132): the frame is compressed where it lies
                writer.write(node.dev_frame)
        else:
            disp, ms = node.process(np.ascontiguousarray(left), np.ascontiguousarray(right))
        Image.fromarray(disp).save(os.path.join(args.out, n))
        print(f"{n}: Elapsed time =: {ms:.3f} ms", flush=True)
    if writer:
        writer.close()
        print(f"{args.record}: {len(writer.index)} frames", flush=True)


if __name__ == "__main__":
    main()
