"""TEST INFRASTRUCTURE: model of packed 24-bit output (include/mibayer.h, MIBAYER_FLAG_DST_24BIT).

No arithmetic of its own: a 24-bit frame is the 4-byte models' frame of the SAME cfg with RGBx (for RGB) or BGRx (for
BGR) -- oracle/bayer2rgb_np.py for the reference's bilinear demosaic of an 8-bit mosaic, highbit_model for deep mosaics,
mhc_model for the MHC filters, colour_model for the colour stage -- with byte 3 of every pixel dropped, laid out at a
given stride.  The model's only job is that layout, so the pin to the reference is the 4-byte models'.  Only the first
3 * width bytes of a row are the model's; the rest of the row (the padding) keeps what the destination held."""
import numpy as np

import colour_model as cm
import highbit_model as hm
import mhc_model as mm
from oracle import bayer2rgb_np

FOUR_BYTE = {"RGB": "RGBx", "BGR": "BGRx"}      # the 4-byte layout whose first three bytes are the 24-bit pixel
OFFSETS = {"RGB": (0, 1, 2), "BGR": (2, 1, 0)}
GUARD = 0xA5


def default_stride(width):
    """GStreamer's RGB stride: ROUND_UP_4 (3 * width)"""
    return (3 * width + 3) & ~3


def drop_byte3(rows4, width):
    """(H, >= 4 * width) bytes of 4-byte pixels -> (H, 3 * width) bytes: bytes 0, 1, 2 of every pixel"""
    rows4 = np.asarray(rows4, np.uint8)
    h = rows4.shape[0]
    return np.ascontiguousarray(rows4[:, :4 * width].reshape(h, width, 4)[:, :, :3]).reshape(h, 3 * width)


def lay_out(rows3, stride=None, dst=None):
    """(H, 3 * width) bytes -> (H, stride): rows at `stride`, the padding as `dst` holds it (a fresh frame: GUARD)"""
    h, row = rows3.shape
    stride = default_stride(row // 3) if stride is None else stride
    assert stride >= row and stride % 4 == 0
    out = np.full((h, stride), GUARD, np.uint8) if dst is None else np.array(dst, np.uint8).reshape(h, stride)
    out[:, :row] = rows3
    return out


def from_four_byte(rows4, width, stride=None, dst=None):
    """a 4-byte model's RGBx / BGRx frame -> the RGB / BGR frame at `stride`"""
    return lay_out(drop_byte3(rows4, width), stride, dst)


def four_byte(src, width, height, pattern, fmt, bits=0, method="bilinear", colour=None, src_big_endian=False,
              src_stride=None):
    """the 4-byte models' frame of the same cfg: fmt "RGB" -> RGBx, "BGR" -> BGRx.  colour: None, or the keywords of
    colour_model.bayer2rgb_colour (black= / matrix= / tone=)"""
    layout = FOUR_BYTE[fmt]
    if colour is not None:
        return cm.bayer2rgb_colour(src, width, height, pattern, layout, bits=bits, out16=False, method=method,
                                   src_big_endian=src_big_endian, stride=src_stride, **colour)
    if method == "mhc":
        return mm.bayer2rgb_mhc(src, width, height, pattern, layout, bits=bits, out16=False,
                                src_big_endian=src_big_endian, stride=src_stride)
    if bits in (0, 8):
        stride = width if src_stride is None else src_stride
        raw = np.frombuffer(np.ascontiguousarray(src).tobytes(), np.uint8)[:stride * height].reshape(height, stride)
        return bayer2rgb_np.bayer2rgb(raw[:, :width], pattern, *hm.LAYOUTS[layout]).reshape(height, 4 * width)
    return hm.bayer2rgb_highbit(src, width, height, pattern, layout, bits, False, src_big_endian, stride=src_stride)


def bayer2rgb_rgb24(src, width, height, pattern, fmt, bits=0, method="bilinear", colour=None, src_big_endian=False,
                    src_stride=None, dst_stride=None, dst=None):
    """Frame bytes -> (height, dst_stride) bytes of a MIBAYER_FLAG_DST_24BIT context"""
    rows4 = four_byte(src, width, height, pattern, fmt, bits, method, colour, src_big_endian, src_stride)
    return from_four_byte(rows4, width, dst_stride, dst)
