"""TEST INFRASTRUCTURE: NumPy model of the half-size demosaic (include/mibayer.h, MIBAYER_FLAG_HALF).

Written from the header's text, not from the kernel.  One output pixel per CFA quad: output pixel (X, Y) reads the
samples S (2X + dx, 2Y + dy), dx, dy in {0, 1}; R is the quad's red sample, B its blue one, G = (Ga + Gb + 1) >> 1 of
its two greens at native depth.  The output is W // 2 by H >> 1 (the last row of an odd height has no quad).  From the
(R, G, B) values on nothing is new: highbit_model.to_output for the conversion and the 4- / 8-byte layouts,
colour_model.stage / pack for the colour stage, rgb24_model / planar_model for the 3-byte and planar layouts.
tests/test_half_model.py ties native_rgb_half to the reference-pinned full-resolution oracle."""
import numpy as np

import colour_model as cm
import highbit_model as hm
import planar_model as pm
import rgb24_model as rm

PATTERNS = hm.PATTERNS
# (dy, dx) of the quad's red, first green, second green and blue sample
SITES = {
    "bggr": ((1, 1), (0, 1), (1, 0), (0, 0)),
    "gbrg": ((1, 0), (0, 0), (1, 1), (0, 1)),
    "grbg": ((0, 1), (0, 0), (1, 1), (1, 0)),
    "rggb": ((0, 0), (0, 1), (1, 0), (1, 1)),
}
NAMES = {v: k for k, v in PATTERNS.items()}
GUARD = 0xA5


def out_size(width, height):
    return width // 2, height >> 1


def native_rgb_half(S, pattern):
    """(H, W) masked samples -> (H >> 1, W // 2, 3) int64 (R, G, B) at the native depth"""
    if not isinstance(pattern, str):
        pattern = NAMES[int(pattern)]
    S = np.asarray(S).astype(np.int64)
    H, W = S.shape
    if W < 4 or W % 2 or H < 3:
        raise ValueError("outside the defined domain")
    ow, oh = out_size(W, H)
    site = lambda dy, dx: S[dy:2 * oh:2, dx:2 * ow:2]          # noqa: E731
    r, ga, gb, b = (site(*d) for d in SITES[pattern])
    return np.stack([r, (ga + gb + 1) >> 1, b], axis=-1)


def samples(src, width, height, bits=0, src_big_endian=False, stride=None):
    """frame bytes -> ((H, W) int64 masked samples, depth)"""
    if bits in (0, 8):
        stride = width if stride is None else stride
        raw = np.frombuffer(np.ascontiguousarray(src).tobytes(), np.uint8)[:stride * height].reshape(height, stride)
        return raw[:, :width].astype(np.int64), 8
    return hm.unpack(src, width, height, stride, bits, src_big_endian), bits


def rows(src, width, height, pattern, fmt, bits=0, colour=None, src_big_endian=False, dst_big_endian=False,
         src_stride=None):
    """frame bytes -> (OH, px * OW) bytes of a 4- or 8-byte layout (a highbit_model.LAYOUTS name; a ...64 name is 16-bit
    channels).  colour: None, or the keywords of colour_model.stage (black= / matrix= / tone=)"""
    S, depth = samples(src, width, height, bits, src_big_endian, src_stride)
    out16 = fmt.endswith("64")
    rgb = native_rgb_half(S, pattern)
    if colour is not None:
        return cm.pack(cm.stage(rgb, depth, out16=out16, **colour), fmt, out16, dst_big_endian)
    return hm.to_output(rgb, depth, fmt, out16, dst_big_endian)


def default_stride(fmt, ow):
    px = 8 if fmt.endswith("64") else 3 if fmt in rm.FOUR_BYTE else 1 if fmt in pm.FORMATS else 4
    return (px * ow + 3) & ~3


def frame(src, width, height, pattern, fmt, bits=0, colour=None, src_big_endian=False, dst_big_endian=False,
          src_stride=None, dst_stride=None):
    """frame bytes -> the whole destination frame of a HALF context as (rows, dst_stride) bytes, padding GUARD: OH rows,
    3 OH rows (stacked planes) for a planar_model.FORMATS name; fmt may also be "RGB" / "BGR" (3-byte pixels)"""
    ow, oh = out_size(width, height)
    stride = dst_stride or default_stride(fmt, ow)
    kw = dict(bits=bits, colour=colour, src_big_endian=src_big_endian, src_stride=src_stride)
    if fmt in pm.FORMATS:
        return pm.deal(rows(src, width, height, pattern, "RGBx", **kw), ow, fmt, stride).reshape(3 * oh, stride)
    if fmt in rm.FOUR_BYTE:
        return rm.from_four_byte(rows(src, width, height, pattern, rm.FOUR_BYTE[fmt], **kw), ow, stride)
    body = rows(src, width, height, pattern, fmt, dst_big_endian=dst_big_endian, **kw)
    out = np.full((oh, stride), GUARD, np.uint8)
    out[:, :body.shape[1]] = body
    return out
