"""The point cloud op's definition (esm_cloud_desc, include/esmstereo_amd.h) in numpy, written from the definition:
fp32 arrays, one operation per line (numpy rounds each once), the boolean mask, raster order, both packings."""
import numpy as np

PLY, PCL = 0, 1
XYZ = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
XYZ_PLY = np.dtype(XYZ.descr + [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
XYZ_PCL = np.dtype(XYZ.descr + [("rgb", "<u4")])


def record_dtype(color: bool, packing: int = PLY) -> np.dtype:
    return XYZ if not color else (XYZ_PLY if packing == PLY else XYZ_PCL)


def max_points(H: int, W: int, step: int) -> int:
    return -(-H // step) * -(-W // step)


def cloud(disp, num, fx, fy, cx, cy, z_min=0.0, z_max=np.inf, step=1, color=None, bgr=True, valid=None, packing=PLY):
    """``disp`` fp32 [H, W]; ``color`` uint8 [H, W, 3] or None; ``valid`` uint8 / bool [H, W] or None -> the kept
    points of the image as a structured array of ``record_dtype``, in raster order of (y, x)."""
    f32 = np.float32
    d = np.asarray(disp, dtype=f32)[::step, ::step]
    H, W = np.asarray(disp).shape
    y, x = np.meshgrid(np.arange(0, H, step), np.arange(0, W, step), indexing="ij")
    num, fx, fy, cx, cy, z_min, z_max = (f32(v) for v in (num, fx, fy, cx, cy, z_min, z_max))
    with np.errstate(all="ignore"):
        Z = num / d
        X = x.astype(f32) - cx
        X = X * Z
        X = X / fx
        Y = y.astype(f32) - cy
        Y = Y * Z
        Y = Y / fy
        keep = (d > 0) & (Z >= z_min) & (Z <= z_max)
    assert Z.dtype == X.dtype == Y.dtype == f32
    if valid is not None:
        keep &= np.asarray(valid)[::step, ::step] != 0
    out = np.zeros(int(keep.sum()), dtype=record_dtype(color is not None, packing))
    out["x"], out["y"], out["z"] = X[keep], Y[keep], Z[keep]  # boolean indexing is raster order
    if color is not None:
        c = np.asarray(color, dtype=np.uint8)[::step, ::step][keep]
        red, green, blue = (c[:, 2], c[:, 1], c[:, 0]) if bgr else (c[:, 0], c[:, 1], c[:, 2])
        if packing == PLY:
            out["red"], out["green"], out["blue"], out["alpha"] = red, green, blue, 255
        else:
            out["rgb"] = red.astype(np.uint32) << 16 | green.astype(np.uint32) << 8 | blue.astype(np.uint32)
    return out


def cloud_batch(disp, *args, color=None, valid=None, **kw):
    """[B, H, W] (and [B, H, W, 3], [B, H, W]) -> one array per image."""
    return [cloud(disp[b], *args, color=None if color is None else color[b],
                  valid=None if valid is None else valid[b], **kw) for b in range(len(disp))]
