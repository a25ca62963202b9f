"""TEST INFRASTRUCTURE: model of planar 8-bit output (include/mibayer.h, MIBAYER_FLAG_DST_PLANAR).

Layout only: a planar frame is the 4-byte models' RGBx frame of the SAME cfg (rgb24_model.four_byte (..., fmt="RGB"):
the oracle for the reference's bilinear demosaic of an 8-bit mosaic, highbit_model, mhc_model, colour_model) with byte
0 / 1 / 2 of every pixel dealt to plane r_off / g_off / b_off.  A plane is `height` rows of dst_stride bytes, plane k
starts k * dst_stride * height into the frame, and only the first `width` bytes of a row are the model's: the rest of
the row (the padding) keeps what the destination held.  The pin to the reference is the 4-byte models'."""
import itertools

import numpy as np

import rgb24_model as rm

FORMATS = {"RGBP": (0, 1, 2), "BGRP": (2, 1, 0), "GBR": (2, 0, 1)}      # GStreamer's names: plane indices of R, G, B
PERMUTATIONS = tuple(itertools.permutations((0, 1, 2)))
GUARD = 0xA5


def default_stride(width):
    """ROUND_UP_4 (width): GStreamer's stride of a plane of GBR / RGBP / BGRP"""
    return (width + 3) & ~3


def offsets_of(fmt):
    off = FORMATS[fmt] if isinstance(fmt, str) else tuple(fmt)
    assert sorted(off) == [0, 1, 2], off
    return off


def deal(rows4, width, fmt, stride=None, dst=None):
    """(H, >= 4 * width) bytes of RGBx pixels -> (3, H, stride): byte c of every pixel in plane fmt[c], the padding as
    `dst` holds it (a fresh frame: GUARD)"""
    rows4 = np.asarray(rows4, np.uint8)
    h = rows4.shape[0]
    off = offsets_of(fmt)
    stride = default_stride(width) if stride is None else stride
    assert stride >= width and stride % 4 == 0
    out = np.full((3, h, stride), GUARD, np.uint8) if dst is None else np.array(dst, np.uint8).reshape(3, h, stride)
    px = rows4[:, :4 * width].reshape(h, width, 4)
    for c in range(3):
        out[off[c], :, :width] = px[:, :, c]
    return out


def interleave(planes, width, fmt):
    """(3, H, >= width) -> (H, 4 * width) RGBx with byte 3 = 255: the inverse of deal"""
    off = offsets_of(fmt)
    h = planes.shape[1]
    px = np.full((h, width, 4), 255, np.uint8)
    for c in range(3):
        px[:, :, c] = planes[off[c], :, :width]
    return px.reshape(h, 4 * width)


def bayer2rgb_planar(src, width, height, pattern, fmt, bits=0, method="bilinear", colour=None, src_big_endian=False,
                     src_stride=None, dst_stride=None, dst=None):
    """Frame bytes -> (3, height, dst_stride) bytes of a MIBAYER_FLAG_DST_PLANAR context"""
    rows4 = rm.four_byte(src, width, height, pattern, "RGB", bits, method, colour, src_big_endian, src_stride)
    return deal(rows4, width, fmt, dst_stride, dst)
