"""A numpy restatement of the rendering definitions of include/esmstereo_amd.h (esm_disp_colorize_u8,
esm_disp_to_depth_f32), written from the definitions and importing nothing from the package.

Every function takes fp32 maps ``[..., H, W]`` and returns the table index 0..255 per pixel; ``apply_lut`` and
``stack`` finish the frame.  fp32 arithmetic throughout, one rounding per operation."""
import numpy as np

F32 = np.float32


def to_u16(d):
    """The value esm_disp_to_u16 writes: rint(d * 256) (half to even), then the low 16 bits of the 32-bit integer.
    The conversion to int32 saturates and NaN gives 0 (the device's conversion; numpy's own cast is undefined
    outside int32, which only |d| >= 2^23 and inf reach)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(d, F32) * F32(256)).astype(np.float64)
        i = np.where(np.isnan(r), 0.0, np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
    return (i & 0xFFFF).astype(np.uint16)


def saturate_u8(r):
    """Clamp a rounded fp32 value to 0..255 (NaN gives 0)."""
    r = np.asarray(r, F32)
    return np.where(np.isnan(r), F32(0), np.minimum(np.maximum(r, F32(0)), F32(255))).astype(np.uint8)


def index_scale(d, alpha=0.01):
    """SCALE: saturate_u8(rint(float(u) * alpha)), alpha as fp32."""
    return saturate_u8(np.rint(to_u16(d).astype(F32) * F32(alpha)))


def range_u(m):
    """u of RANGE mode: min(rint(m * 256), 65535) where m > 0, else 0 (NaN is not > 0)."""
    m = np.asarray(m, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = m > 0
        r = np.minimum(np.rint(np.where(valid, m, F32(0)) * F32(256)), F32(65535))
    return np.where(valid, r, F32(0)).astype(np.uint32), valid


def range_coefficients(mn, mx):
    """(a, b) as fp32: -255 / (mx - mn) and 255 * mx / (mx - mn), computed in fp64 and rounded once."""
    span = float(mx) - float(mn)
    return F32(-255.0 / span), F32(255.0 * float(mx) / span)


def index_range_image(m):
    """RANGE for ONE image [H, W]: idx = saturate_u8(rint(float(u) * a + b)) for every pixel, the multiply and the
    add rounded separately; 0 everywhere when no pixel is valid or max == min."""
    u, valid = range_u(m)
    if not valid.any():
        return np.zeros(u.shape, np.uint8)
    mn, mx = int(u[valid].min()), int(u[valid].max())
    if mx == mn:
        return np.zeros(u.shape, np.uint8)
    a, b = range_coefficients(mn, mx)
    prod = u.astype(F32) * a
    return saturate_u8(np.rint(prod + b))


def index_range(m):
    m = np.asarray(m, F32)
    return np.stack([index_range_image(x) for x in m.reshape((-1,) + m.shape[-2:])]).reshape(m.shape)


def depth_map(d, num, max_depth):
    """clip(num / d, 0, max_depth): IEEE fp32 division, np.clip (a NaN stays)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.clip(F32(num) / np.asarray(d, F32), F32(0), F32(max_depth))


def index_depth(d, num, max_depth):
    """DEPTH: 255 - uint8(clip(depth / max_depth, 0, 1) * 255), truncated; NaN -> uint8 0."""
    with np.errstate(invalid="ignore"):
        n = np.clip(depth_map(d, num, max_depth) / F32(max_depth), F32(0), F32(1))
        v = n * F32(255)
        u8 = np.where(np.isnan(v), F32(0), v).astype(np.uint8)
    return (255 - u8.astype(np.int32)).astype(np.uint8)


def apply_lut(idx, lut):
    """[..., H, W] indices -> [..., H, W, 3] through a uint8 [256, 3] table."""
    lut = np.asarray(lut)
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    return lut[np.asarray(idx, np.intp)]


def stack(top, colour):
    """np.concatenate((left_img, disp_np), 0) per image: [B, H, W, 3] x 2 -> [B, 2H, W, 3]."""
    return np.concatenate((np.asarray(top, np.uint8), colour), axis=-3)


def render(d, lut, mode, top=None, alpha=0.01, num=None, max_depth=None):
    """The whole op for a batch [B, H, W]."""
    if mode == "scale":
        idx = index_scale(d, alpha)
    elif mode == "range":
        idx = index_range(d)
    elif mode == "depth":
        idx = index_depth(d, num, max_depth)
    else:
        raise ValueError(mode)
    img = apply_lut(idx, lut)
    return img if top is None else stack(top, img)
